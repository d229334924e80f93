"""Line filtering on the GPU (td_line_filter_device, td_line_filter, Tokenizer.filter_lines) against the rule in plain Python
(tests/linefilter_truth.py): output bytes, offsets, stats and totals must be EQUAL.  The outputs lie in buffers filled with 0x77 that are
longer than the call may write.  No case here makes the device fault: every error is one the library reports by a status code."""
import numpy as np
import pytest

import helpers as H
import linefilter_truth as lt

pytestmark = pytest.mark.gpu

FILL, SLACK = 0x77, 9
CASES = lt.seam_cases()


@pytest.fixture(scope="module")
def tok():
    from tokendagger_amd import capi
    pat, mr, special = H.llama4()
    return capi.HipTokenizer(pat, mr, special, device=0)


@pytest.fixture(scope="module")
def side():
    import torch
    return torch.cuda.Stream(device=torch.device("cuda", 0))


class Call:
    """One td_line_filter_device call enqueued on `stream`, the text `shift` bytes off the 16-byte grid; result() waits and reads back."""

    def __init__(self, tok, stream, text, offs, kw, shift=0, cap=None, want_out=True, want_offs=True, want_totals=True, n_bytes=None):
        import torch
        dev = torch.device("cuda", 0)
        text, offs = np.frombuffer(bytes(text), dtype=np.uint8), np.asarray(offs, dtype=np.int64)
        self.n_docs, self.cap, self.stream = len(offs) - 1, len(text) if cap is None else cap, stream
        with torch.cuda.stream(stream):
            self.raw = torch.from_numpy(np.concatenate([np.full(16 + shift, 0x41, np.uint8), text, np.full(16, 0x41, np.uint8)])).to(dev)
            self.offs = torch.from_numpy(offs).to(dev)
            self.out = torch.full((self.cap + SLACK,), FILL, dtype=torch.uint8, device=dev)
            self.ooff = torch.full((self.n_docs + 1 + SLACK,), FILL, dtype=torch.int64, device=dev)
            self.stats = torch.full((self.n_docs * 8 + SLACK,), FILL, dtype=torch.int64, device=dev)
            self.totals = torch.full((8 + SLACK,), FILL, dtype=torch.int64, device=dev)
            self.counts = torch.full((8,), FILL, dtype=torch.int64, device=dev)
        tok.line_filter_device(self.raw.data_ptr() + 16 + shift, len(text) if n_bytes is None else n_bytes, self.offs.data_ptr(), self.n_docs,
                               lt.make_rules(kw), self.out.data_ptr() if want_out else 0, self.cap if want_out else 0,
                               self.ooff.data_ptr() if want_offs else 0, self.stats.data_ptr(), self.totals.data_ptr() if want_totals else 0,
                               self.counts.data_ptr(), stream.cuda_stream)

    def result(self):
        """-> ((text, offsets, stats, totals), counts, the slack behind every output is untouched, the whole buffers)"""
        self.stream.synchronize()
        out, ooff, stats, totals = (x.cpu().numpy() for x in (self.out, self.ooff, self.stats, self.totals))
        n = self.n_docs
        slack = bool((out[self.cap:] == FILL).all() and (ooff[n + 1:] == FILL).all() and (stats[8 * n:] == FILL).all() and (totals[8:] == FILL).all())
        need = min(int(ooff[n]), self.cap) if ooff[n] >= 0 else 0
        return (out[:need], ooff[:n + 1], stats[:8 * n].reshape(n, 8), totals[:8]), self.counts.cpu().numpy(), slack, (out, ooff, stats, totals)


@pytest.fixture(scope="module")
def want():
    """name -> the truth's answer, computed once a case and left unchanged"""
    memo = {}
    return lambda name: memo.setdefault(name, lt.filter_lines(CASES[name][0], CASES[name][1], **CASES[name][2]))


@pytest.mark.parametrize("name", list(CASES))
def test_seam_cases(tok, side, want, name):
    from tokendagger_amd import capi
    text, offs, kw = CASES[name]
    call = Call(tok, side, text, offs, kw)
    assert tok.device_status_pos(side.cuda_stream) == (capi.TD_OK, 0)
    got, counts, slack, _ = call.result()
    lt.same(got, want(name), name)
    assert slack and counts.tolist() == [len(want(name)[0])] + [0] * 7
    if not kw:
        assert bytes(got[0]) == text and got[1].tolist() == list(offs)
    if name == "everything dropped":
        assert got[1].tolist() == [0, 0, 0] and got[3][0] > 0


@pytest.mark.parametrize("shift", range(16))
def test_every_misalignment_of_the_text(tok, side, want, shift):
    name = "three tiles, no LF, decided middle"
    got, _, slack, _ = Call(tok, side, *CASES[name], shift=shift).result()
    lt.same(got, want(name), (name, shift))
    assert slack
    name = "the lengths between empty documents"
    lt.same(Call(tok, side, *CASES[name], shift=shift).result()[0], want(name), (name, shift))


def test_stats_only(tok, side, want):
    name = "more than 256 tiles"
    call = Call(tok, side, *CASES[name], want_out=False, want_offs=False, want_totals=False)
    assert tok.device_status_pos(side.cuda_stream)[0] == 0
    _, counts, _, (out, ooff, stats, totals) = call.result()
    n = call.n_docs
    assert stats[:8 * n].reshape(n, 8).tolist() == want(name)[2] and counts[0] == len(want(name)[0])
    assert (out == FILL).all() and (ooff == FILL).all() and (totals == FILL).all() and (stats[8 * n:] == FILL).all()


def test_capacity_one_byte_short(tok, side, want):
    from tokendagger_amd import capi
    name = "the lengths between empty documents"
    need = len(want(name)[0])
    call = Call(tok, side, *CASES[name], cap=need - 1)
    assert tok.device_status_pos(side.cuda_stream) == (capi.TD_E_CAPACITY, need)
    _, counts, _, (out, ooff, _, _) = call.result()
    assert counts[0] == need and (out == FILL).all() and (ooff == FILL).all()
    call = Call(tok, side, *CASES[name], cap=need)
    assert tok.device_status_pos(side.cuda_stream)[0] == capi.TD_OK
    lt.same(call.result()[0], want(name), "exactly enough")
    with pytest.raises(capi.TokenDaggerHipError) as e:
        tok.line_filter(CASES[name][0], CASES[name][1], lt.make_rules(CASES[name][2]), capacity=need - 1)
    assert e.value.code == capi.TD_E_CAPACITY and str(need) in str(e.value)


@pytest.mark.parametrize("offs, n_bytes, bad", [([0, 30, 20, 10, 40], 40, 1), ([1, 10, 40], 40, 0), ([0, 10, 50], 40, 1), ([0, -1, 40], 40, 0)])
def test_bad_offsets_write_nothing(tok, side, offs, n_bytes, bad):
    from tokendagger_amd import capi
    call = Call(tok, side, lt.prose(64), offs, lt.C4ISH, cap=64, n_bytes=n_bytes)
    assert tok.device_status_pos(side.cuda_stream) == (capi.TD_E_INVALID, bad)
    _, counts, _, whole = call.result()
    assert (counts == FILL).all() and all((x == FILL).all() for x in whole)


def test_two_calls_on_one_handle_without_a_host_wait(tok, side, want):
    """the second call's rules keep what the first dropped: nothing of the first's masks, carries or sums may reach it"""
    a, b = "three tiles, decided last", "empty rules"
    text, offs, _ = CASES[a]
    first = Call(tok, side, text, offs, CASES[a][2])
    second = Call(tok, side, text, offs, {})
    third = Call(tok, side, *CASES[b][:2], lt.C4ISH)
    assert tok.device_status_pos(side.cuda_stream)[0] == 0
    lt.same(first.result()[0], want(a), "first")
    lt.same(second.result()[0], lt.filter_lines(text, offs), "second")
    lt.same(third.result()[0], lt.filter_lines(*CASES[b][:2], **lt.C4ISH), "third")
    assert bytes(second.result()[0][0]) == text


def test_filter_lines_feeds_the_encode(tok, want):
    import tokendagger as tiktoken
    pat, mr, special = H.llama4()
    tk = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    name = "the lengths between empty documents"
    text, offs, kw = CASES[name]
    ft = tk.filter_lines(text, np.asarray(offs, dtype=np.int64), min_words=kw["min_words"], need_terminal=True, drop_line_phrases=("JavaScript",),
                         count_doc_phrases=(b"AA",))
    lt.same((ft.text, ft.offsets, ft.stats, ft.totals), want(name), "Tokenizer.filter_lines")
    assert np.array_equal(ft.kept_lines, ft.stats[:, 1]) and np.array_equal(ft.doc_phrase_hits, ft.stats[:, 7])
    lt.same(tok.line_filter(text, offs, lt.make_rules(kw)), want(name), "td_line_filter")
    ids, toff = tk.encode_batch_to_numpy(ft.text, ft.offsets)
    e_ids, e_off = tk.encode_batch_to_numpy(np.frombuffer(want(name)[0], dtype=np.uint8), np.asarray(want(name)[1], dtype=np.int64))
    assert np.array_equal(ids, e_ids) and np.array_equal(toff, e_off) and len(ids) > 0
