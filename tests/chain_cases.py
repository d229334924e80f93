"""What tests/test_gpu_chains.py launches: one small class per device entry point.  An operation allocates its guarded, FILL-filled
outputs and uploads its own small inputs when it is MADE, so that a chain can be made completely, the device synchronised once, and
then launched call after call with nothing between the calls: launch() makes the library call and nothing else.  check() is for the
end: it copies the outputs back and compares them with the truth the operation was made with, exactly.

Every pointer an operation takes is a plain integer, so the output of one operation (op.out[name].ptr) is the input of the next before
anything has run.  Sizes are host arguments: the caller passes the truth's."""
from __future__ import annotations

import numpy as np

FILL = 0xA7   # every byte of every output before the launch
GUARD = 16    # elements in front of and behind every output that nobody may write


def dev():
    import torch
    return torch.device("cuda", 0)


def up(a, dtype, front=0, back=0, pad=0):
    """-> (the tensor, the pointer of a's first element): a on the device with `front` / `back` elements of `pad` around it."""
    import torch
    a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    t = torch.from_numpy(np.concatenate([np.full(front, pad, dtype), a, np.full(back, pad, dtype)])).to(dev())
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + front * a.itemsize


class Buf:
    """n elements of dtype between two guards, all FILL bytes; init: what the payload starts as (an in/out buffer)."""

    def __init__(self, n, dtype, init=None):
        import torch
        self.n, self.dtype = int(n), np.dtype(dtype)
        size = self.dtype.itemsize
        self.raw = torch.full(((self.n + 2 * GUARD) * size,), FILL, dtype=torch.uint8, device=dev())
        self.ptr = self.raw.data_ptr() + GUARD * size
        assert self.ptr % 8 == 0
        if init is not None:
            init = np.ascontiguousarray(init, dtype=self.dtype).reshape(-1)
            assert len(init) == self.n
            self.raw[GUARD * size:(GUARD + self.n) * size] = torch.from_numpy(init.view(np.uint8)).to(dev())

    def expect(self, want, what):
        """The first len(want) elements equal want; every other byte, the guards included, is still FILL.  want None: all of it is."""
        a = self.raw.cpu().numpy().view(self.dtype)
        fill = np.frombuffer(bytes([FILL]) * self.dtype.itemsize, dtype=self.dtype)[0]
        assert (a[:GUARD] == fill).all() and (a[GUARD + self.n:] == fill).all(), (what, "a guard element was written")
        got = a[GUARD:GUARD + self.n]
        if want is None:
            assert (got == fill).all(), (what, "written although the call was bad", np.flatnonzero(got != fill)[:8].tolist())
            return
        want = np.ascontiguousarray(want).reshape(-1)
        assert want.dtype.itemsize == self.dtype.itemsize and len(want) <= self.n, (what, want.dtype, len(want), self.n)
        want = want.view(self.dtype)
        bad = np.flatnonzero(got[:len(want)] != want)
        assert len(bad) == 0, (what, f"{len(bad)} of {len(want)} differ, first at {bad[:4].tolist()}", got[bad[:4]].tolist(), want[bad[:4]].tolist())
        assert (got[len(want):] == fill).all(), (what, "written behind the truth's end")


class Op:
    """out: name -> Buf; want: name -> array (the truth) or None for a call that must write nothing."""
    name = "op"

    def __init__(self):
        self.out, self.want, self.keep = {}, {}, []

    def add(self, name, n, dtype, want, init=None):
        self.out[name] = Buf(n, dtype, init)
        self.want[name] = want

    def ptr(self, name):
        return self.out[name].ptr

    def check(self, what, written=True):
        for name, b in self.out.items():
            b.expect(self.want[name] if written else None, (what, self.name, name))


class Utf8(Op):
    name = "utf8_device"

    def __init__(self, d_text, n_bytes, d_offs, n_docs, policy, want):
        """want: capi.utf8_host's (out, out_offsets, flags, first_bad, n_bad, counts)"""
        super().__init__()
        self.a = (d_text, n_bytes, d_offs, n_docs, policy)
        self.cap = len(want[0])
        for name, n, dt, w in (("text", max(self.cap, 1), np.uint8, want[0]), ("offsets", n_docs + 1, np.int64, want[1]), ("flags", n_docs, np.uint8, want[2]),
                               ("first_bad", n_docs, np.int64, want[3]), ("n_bad", n_docs, np.int64, want[4]), ("counts", 8, np.int64, want[5])):
            self.add(name, n, dt, w)

    def launch(self, tok, s):
        d_text, n_bytes, d_offs, n_docs, policy = self.a
        tok.utf8_device(d_text, n_bytes, d_offs, n_docs, policy, self.ptr("text"), self.cap, self.ptr("offsets"), self.ptr("flags"),
                        self.ptr("first_bad"), self.ptr("n_bad"), self.ptr("counts"), s)


class Nfc(Op):
    name = "nfc_device"

    def __init__(self, d_text, n_bytes, d_offs, n_docs, want):
        """want: capi.nfc_host's (out, out_offsets, flags, changed, counts)"""
        super().__init__()
        self.a = (d_text, n_bytes, d_offs, n_docs)
        self.cap = len(want[0])
        for name, n, dt, w in (("text", max(self.cap, 1), np.uint8, want[0]), ("offsets", n_docs + 1, np.int64, want[1]),
                               ("changed", n_docs, np.uint8, want[3]), ("counts", 8, np.int64, want[4])):
            self.add(name, n, dt, w)

    def launch(self, tok, s):
        tok.nfc_device(*self.a, self.ptr("text"), self.cap, self.ptr("offsets"), self.ptr("changed"), self.ptr("counts"), s)


class TextStats(Op):
    name = "text_stats_device"

    def __init__(self, d_text, n_bytes, d_offs, n_docs, groups, want):
        """want: textstats_truth.truth's (stats, totals) for `groups`"""
        super().__init__()
        self.a = (d_text, n_bytes, d_offs, n_docs, groups)
        self.add("stats", max(n_docs, 1) * want[0].shape[1], np.int64, want[0])
        self.add("totals", len(want[1]), np.int64, want[1])

    def launch(self, tok, s):
        tok.text_stats_device(*self.a, self.ptr("stats"), self.ptr("totals"), s)


class Encode(Op):
    name = "encode_device"

    def __init__(self, d_text, n_bytes, d_offs, n_docs, want):
        """want: (ids, token offsets)"""
        super().__init__()
        self.a = (d_text, n_bytes, d_offs, n_docs)
        self.cap = len(want[0])
        self.add("ids", max(self.cap, 1), np.int32, want[0])
        self.add("offsets", n_docs + 1, np.int64, want[1])

    def launch(self, tok, s):
        tok.encode_device(*self.a, self.ptr("ids"), self.cap, self.ptr("offsets"), s)


class Select(Op):
    name = "select_docs_device"

    def __init__(self, d_ids, n_tokens, d_offs, n_docs, sel, mn, mx, want):
        """want: select_truth.select_numpy's (ids, labels, offsets, docs, counts)"""
        from tokendagger_amd import capi
        super().__init__()
        t, d_sel = up(sel, np.int64)
        self.keep.append(t)
        self.a = (d_ids, n_tokens, d_offs, n_docs, d_sel, len(sel), capi.select_spec(mn, mx))
        self.cap = len(want[0])
        self.add("ids", max(self.cap, 1), np.int32, want[0])
        self.add("offsets", len(sel) + 1, np.int64, want[2])
        self.add("docs", max(len(sel), 1), np.int64, want[3])
        self.add("counts", 4, np.int64, want[4])

    def launch(self, tok, s):
        tok.select_docs_device(*self.a, self.ptr("ids"), self.cap, self.ptr("offsets"), self.ptr("docs"), self.ptr("counts"), 0, 0, s)


class SpanLabels(Op):
    name = "span_labels_device"

    def __init__(self, d_ids, n_tokens, d_offs, n_docs, open, close, want):
        """want: labels_truth.labels_numpy's (labels, mask, trained_offsets, counts)"""
        from tokendagger_amd import capi
        super().__init__()
        self.a = (d_ids, n_tokens, d_offs, n_docs, capi.labels_spec(open, close, -100, True))
        self.add("labels", max(n_tokens, 1), np.int32, want[0])
        self.add("mask", max(n_tokens, 1), np.uint8, want[1])
        self.add("trained_offsets", n_docs + 1, np.int64, want[2])
        self.add("counts", 4, np.int64, want[3])

    def launch(self, tok, s):
        tok.span_labels_device(*self.a, self.ptr("labels"), self.ptr("mask"), self.ptr("trained_offsets"), self.ptr("counts"), s)


class RowsLabeled(Op):
    name = "make_rows_labeled_device"

    def __init__(self, d_ids, n_tokens, d_offs, n_docs, d_src, S, bos, eos, pad, want, want_labels):
        """TD_ROWS_CONCAT.  want: rows_truth.rows_numpy's (ids, positions, cu_seqlens, counts); want_labels: labeled_rows_truth.label_rows'"""
        from tokendagger_amd import capi
        super().__init__()
        self.rows = want[0].size // S
        self.a = (d_ids, n_tokens, d_offs, n_docs, capi.rows_spec(S, capi.TD_ROWS_CONCAT, bos, eos, pad, False))
        slots = max(self.rows * S, 1)
        self.add("ids", slots, np.int32, want[0])
        self.add("positions", slots, np.int32, want[1])
        self.add("cu_seqlens", n_docs + self.rows + 1, np.int32, want[2])
        self.add("counts", 4, np.int64, want[3])
        self.add("labels", slots, np.int32, want_labels)
        self.lab = capi.rows_labels(d_src, self.ptr("labels"), -1, -2, -3)

    def launch(self, tok, s):
        tok.make_rows_labeled_device(*self.a, self.ptr("ids"), self.rows, self.lab, self.ptr("positions"), self.ptr("cu_seqlens"), self.ptr("counts"), s)


class PackRows(Op):
    name = "pack_rows_device"

    def __init__(self, d_ids, n_tokens, d_offs, n_docs, S, bos, eos, pad, want):
        """want: pack_truth.pack_runs' (ids, positions, cu_seqlens, row_lengths, seg_docs, counts).  The entry point waits once for the
        stream itself (it plans on the host) and returns its counts there."""
        from tokendagger_amd import capi
        super().__init__()
        self.rows = want[0].size // S
        self.a = (d_ids, n_tokens, d_offs, n_docs, capi.pack_spec(S, bos, eos, pad, False))
        slots = max(self.rows * S, 1)
        self.add("ids", slots, np.int32, want[0])
        self.add("positions", slots, np.int32, want[1])
        self.add("cu_seqlens", n_docs + 2 * self.rows + 1, np.int32, want[2])
        self.add("row_lengths", max(self.rows, 1), np.int32, want[3])
        self.add("seg_docs", n_docs + 2 * self.rows, np.int64, want[4])
        self.want_counts, self.counts = np.asarray(want[5], dtype=np.int64), None

    def launch(self, tok, s):
        self.counts = tok.pack_rows_device(*self.a, self.ptr("ids"), self.rows, self.ptr("positions"), self.ptr("cu_seqlens"), self.ptr("row_lengths"),
                                           self.ptr("seg_docs"), s)

    def check(self, what, written=True):
        super().check(what, written)
        assert np.array_equal(self.counts, self.want_counts), (what, self.name, "counts", self.counts, self.want_counts)


class Counts(Op):
    name = "token_counts_device"

    def __init__(self, d_ids, n_tokens, d_offs, n_docs, groups, n_bins, n_groups, want):
        """want: counts_truth.counts_numpy's (counts, info)"""
        from tokendagger_amd import capi
        super().__init__()
        t, d_grp = up(groups, np.int32)
        self.keep.append(t)
        self.a = (d_ids, n_tokens, d_offs, n_docs, d_grp, capi.counts_spec(n_bins, n_groups))
        self.add("counts", n_bins * n_groups, np.int64, want[0])
        self.add("info", 4, np.int64, want[1])

    def launch(self, tok, s):
        tok.token_counts_device(*self.a, self.ptr("counts"), self.ptr("info"), s)


class Minhash(Op):
    name = "minhash_device"

    def __init__(self, d_ids, n_tokens, d_offs, n_docs, k, num_perm, seed, bands, rows, want):
        """want: minhash_truth.minhash_numpy's (sig, band_keys, counts)"""
        from tokendagger_amd import capi
        super().__init__()
        self.a = (d_ids, n_tokens, d_offs, n_docs, capi.minhash_spec(k, num_perm, seed, bands, rows))
        self.add("sig", max(n_docs, 1) * num_perm, np.uint32, want[0])
        self.add("band_keys", max(n_docs, 1) * bands, np.uint64, want[1])
        self.add("counts", 4, np.int64, want[2])

    def launch(self, tok, s):
        tok.minhash_device(*self.a, self.ptr("sig"), self.ptr("band_keys") if self.a[4].bands else 0, self.ptr("counts"), s)


class Ngram(Op):
    name = "ngram_matches_device"

    def __init__(self, nset, n_pats, d_ids, n_tokens, d_offs, n_docs, labels_in, want):
        """want: ngram_truth.matches_numpy's (cover, labels, doc_stats, pattern_counts, counts) with labels=labels_in: the label stream the
        call reads and rewrites, uploaded here (the truth of what stands in d_ids)."""
        from tokendagger_amd import capi
        super().__init__()
        self.a = (nset, d_ids, n_tokens, d_offs, n_docs, capi.ngram_spec(-100))
        self.add("cover", max(n_tokens, 1), np.uint8, want[0])
        self.add("labels", n_tokens, np.int32, want[1], init=labels_in)
        self.add("doc_stats", max(n_docs, 1) * 2, np.int64, want[2])
        self.add("pattern_counts", n_pats, np.int64, want[3])
        self.add("counts", 4, np.int64, want[4])
        self.labels_in = np.ascontiguousarray(labels_in, dtype=np.int32)

    def launch(self, tok, s):
        tok.ngram_matches_device(*self.a, self.ptr("cover"), self.ptr("labels"), self.ptr("doc_stats"), self.ptr("pattern_counts"), self.ptr("counts"), s)

    def check(self, what, written=True):
        if written:
            return super().check(what)
        for name, b in self.out.items():  # (the label stream holds what was uploaded, not FILL)
            b.expect(self.labels_in if name == "labels" else None, (what, self.name, name))


class TokenStarts(Op):
    name = "token_starts_device"

    def __init__(self, d_ids, n_tokens, d_offs, n_docs, want):
        from tokendagger_amd import capi
        super().__init__()
        self.a = (d_ids, n_tokens, d_offs, n_docs)
        self.unit = capi.TD_UNIT_BYTES
        self.add("starts", max(n_tokens, 1), np.int64, want)

    def launch(self, tok, s):
        tok.token_starts_device(*self.a, self.ptr("starts"), self.unit, s)


class DecodeRows(Op):
    name = "decode_rows_device"

    def __init__(self, d_ids, n_tokens, d_offs, n_segs, want):
        """The offsets form.  want: decode_rows_truth.decode_numpy's (bytes, offsets, seg_ids, info)"""
        from tokendagger_amd import capi
        super().__init__()
        self.spec = capi.decode_spec(0, (), ())
        self.a = (d_ids, n_tokens, d_offs, 0, n_segs)
        self.cap = len(want[0])
        self.add("bytes", max(self.cap, 1), np.uint8, np.frombuffer(want[0], dtype=np.uint8))
        self.add("offsets", n_segs + 1, np.int64, want[1])
        self.add("seg_ids", max(n_segs, 1), np.int64, want[2])
        self.add("info", 4, np.int64, want[3])

    def launch(self, tok, s):
        tok.decode_rows_device(*self.a, self.spec, self.ptr("bytes"), self.cap, self.ptr("offsets"), self.ptr("seg_ids"), self.ptr("info"), s)


def swapped(offs, d):
    """offs with entries d and d + 1 exchanged: document d decreases, the library reports position d"""
    bad = np.array(offs, dtype=np.int64, copy=True)
    assert bad[d] < bad[d + 1] and 0 < d
    bad[d], bad[d + 1] = bad[d + 1], bad[d]
    return bad
