"""Label rows on the GPU (td_make_rows_labeled, td_pack_rows_labeled, td_window_rows_labeled, their device forms,
td_encode_batch_span_label_rows and the Python methods).  Every case checks the label rows against the truths of
tests/labeled_rows_truth.py AND every other output against the existing entry point called with the same arguments.  All comparisons
are exact.  No case here makes the device fault: every error is one the library reports by a status code."""
import ctypes

import numpy as np
import pytest

import helpers as H
import labeled_rows_truth as lr

pytestmark = pytest.mark.gpu

TILE = 4096  # td::RC_TILE
BOS, EOS, PAD = 5, 7, 3  # ids of the vocabulary (bos / eos are checked against it), any int32 (pad)
OPENER = "<|header_start|>assistant<|header_end|>"
CLOSERS = ["<|eot|>", "<|eom|>"]
I32_MIN, I32_MAX = lr.I32_MIN, lr.I32_MAX


@pytest.fixture(scope="module")
def tok():
    from tokendagger_amd import capi
    pat, mr, special = H.llama4()
    return capi.HipTokenizer(pat, mr, special, device=0)


@pytest.fixture(scope="module")
def wtok():
    from tokendagger_amd import wrapper
    return wrapper.llama4_scout(0)


def _rspec(layout, S, kw):
    from tokendagger_amd import capi
    b, e = BOS if kw.get("bos") else -1, EOS if kw.get("eos") else -1
    if layout == "concat":
        return capi.rows_spec(S, capi.TD_ROWS_CONCAT, b, e, PAD, kw.get("drop_last", False))
    if layout == "pad":
        return capi.rows_spec(S, capi.TD_ROWS_PAD, b, e, PAD)
    if layout == "bestfit":
        return capi.pack_spec(S, b, e, PAD, kw.get("truncate", False))
    return capi.windows_spec(S, b, e, PAD)


def _lab(kw, src=0, dst=0):
    from tokendagger_amd import capi
    return capi.rows_labels(src, dst, kw.get("bos_value", -100), kw.get("eos_value", -100), kw.get("pad_value", -100),
                            kw.get("mask_overlap", False))


def _eq(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), what


def _host(tok, layout, ids, src, offs, S, kw, want=None):
    """The labeled host call and its counterpart with the same arguments -> (counterpart's tuple, label rows)."""
    spec, lab = _rspec(layout, S, kw), _lab(kw)
    if layout in ("concat", "pad"):
        w = dict(positions=True, aux=True) if want is None else want
        base = tok.make_rows(ids, offs, spec, **w)
        got = tok.make_rows_labeled(ids, src, offs, spec, lab, **w)
    elif layout == "bestfit":
        w = dict(positions=True, cu_seqlens=True, lengths=True, docs=True) if want is None else want
        base = tok.pack_rows(ids, offs, spec, **w)
        got = tok.pack_rows_labeled(ids, src, offs, spec, lab, **w)
    else:
        w = dict(positions=True, lengths=True, docs=True, starts=True) if want is None else want
        base = tok.window_rows(ids, offs, spec, kw.get("overlap", 0), **w)
        got = tok.window_rows_labeled(ids, src, offs, spec, lab, kw.get("overlap", 0), **w)
    assert len(got) == len(base) + 1
    for k, (p, q) in enumerate(zip(got, base)):
        _eq(p, q, (layout, S, kw, "output", k))
    return base, got[-1]


def _check(tok, layout, ids, src, offs, S, kw, want=None):
    base, lab_rows = _host(tok, layout, ids, src, offs, S, kw, want)
    truth = lr.label_rows(layout, src, offs, S, **kw)
    _eq(lab_rows, truth, (layout, S, kw, offs[:8].tolist(), "labels"))
    return base, lab_rows


@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_random_small_cases(tok, layout):
    rng = np.random.default_rng(300 + lr.LAYOUTS.index(layout))
    empty = 0
    for it in range(200):
        src, ids, offs, S, kw = lr.random_case(rng, layout, max_docs=12 if it % 8 else 80)
        if it == 0:  # no documents at all, then documents without an id
            src, ids, offs = src[:0], ids[:0], np.zeros(1, np.int64)
        if it == 1:
            src, ids, offs = src[:0], ids[:0], np.zeros(6, np.int64)
        empty += len(ids) == 0
        _check(tok, layout, ids, src, offs, S, kw)
    assert empty >= 2


@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_output_combinations(tok, layout):
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 70, 40)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offs[-1])
    ids, src = rng.integers(0, 1000, n).astype(np.int32), rng.integers(I32_MIN, I32_MAX + 1, n).astype(np.int32)
    flag = {"concat": "drop_last", "bestfit": "truncate"}.get(layout)
    names = {"concat": ("positions", "aux"), "pad": ("positions", "aux"), "bestfit": ("positions", "cu_seqlens", "lengths", "docs"),
             "windows": ("positions", "lengths", "docs", "starts")}[layout]
    for bos in (False, True):
        for eos in (False, True):
            for fl in ((False, True) if flag else (False,)):
                kw = dict(bos=bos, eos=eos, bos_value=-1, eos_value=EOS, pad_value=-100)
                if flag:
                    kw[flag] = fl
                if layout == "windows":
                    kw["overlap"] = 3
                for m in range(1 << len(names)):
                    want = {nm: bool(m >> k & 1) for k, nm in enumerate(names)}
                    base, _ = _check(tok, layout, ids, src, offs, 24, kw, want)
                    for k, nm in enumerate(names):
                        assert (base[1 + k] is None) == (not want[nm])


def _edge_cases(layout, S, delta):
    """Documents whose start, BOS, EOS and first pad slot fall at TILE + delta (and around it)."""
    at = TILE + delta
    if layout == "concat":  # the stream is the same for every S: document 1 starts (BOS) at `at`, document 0's EOS in front of it
        for b, e in ((True, True), (False, False), (True, False)):
            k = b + e
            yield [at - k, 9, 0, 2 * TILE + delta - at - 9 - 3 * k - 1], dict(bos=b, eos=e)  # (the first pad slot at 2 * TILE + delta - 1)
    elif layout in ("pad", "windows"):
        for b, e in ((True, True), (False, False)):
            if S - b - e < 1:
                continue
            r, o = at // S, at % S  # the EOS (or the first pad slot) of row r at slot `at`
            L = max(o - b, 0)
            lens = [min(3, S - b - e)] * r + [min(L, S - b - e)] + [S + 3 if layout == "pad" or S < 2000 else 1, 0, 1]
            yield lens, dict(bos=b, eos=e)
            if layout == "windows" and S - b - e > 1:
                yield [at + 7, 2], dict(bos=b, eos=e, overlap=min(2, S - b - e - 1), mask_overlap=True)  # one document of many windows
    else:
        for b, e in ((True, True), (False, False)):
            k = b + e
            yield [at - k, 5, max(S - k - 1, 0), 1, 0, S // 2, at % 97], dict(bos=b, eos=e)  # split documents and remainders
            if S >= k:
                yield [at, S + 1, 3], dict(bos=b, eos=e, truncate=True)


@pytest.mark.parametrize("layout", lr.LAYOUTS)
@pytest.mark.parametrize("S", [1, 3, 4, 5, 64, 4095, 4096, 4097])
def test_tile_edges(tok, layout, S):
    rng = np.random.default_rng(S)
    ran = 0
    for delta in range(-5, 6):
        for lens, kw in _edge_cases(layout, S, delta):
            if layout == "windows" and S - kw["bos"] - kw["eos"] < 1:
                continue
            lens = [max(int(x), 0) for x in lens]
            assert sum(lens) + 2 * len(lens) <= 4 * TILE  # (three tiles and a remainder at the most)
            offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            n = int(offs[-1])
            ids, src = rng.integers(0, 1000, n).astype(np.int32), (np.arange(n) + 1000).astype(np.int32)
            kw = dict(bos_value=-1, eos_value=-2, pad_value=-3, **kw)
            base, lab_rows = _check(tok, layout, ids, src, offs, S, kw)
            ran += 1
    assert ran >= 11, (layout, S, ran)  # (every combination here has a valid spec: a case at each of the eleven offsets at least)


def test_concat_more_documents_than_the_lds_table(tok):
    """More than ROWS_LDS_DOCS (4352) documents inside one tile: the slots search global memory."""
    rng = np.random.default_rng(2)
    lens = rng.integers(0, 2, 5000)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offs[-1])
    ids, src = rng.integers(0, 1000, n).astype(np.int32), rng.integers(I32_MIN, I32_MAX + 1, n).astype(np.int32)
    for b, e in ((False, False), (True, False), (True, True)):
        _check(tok, "concat", ids, src, offs, 512, dict(bos=b, eos=e, bos_value=1, eos_value=2, pad_value=3))


def test_window_and_bestfit_table_limits(tok):
    rng = np.random.default_rng(3)
    kw = dict(bos=True, eos=True, bos_value=-1, eos_value=-2, pad_value=-3)
    lens = rng.integers(0, 3, 6000)  # rows == n_docs: a row per document, S = 4 -> 1024 rows a tile
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offs[-1])
    ids, src = rng.integers(0, 1000, n).astype(np.int32), rng.integers(I32_MIN, I32_MAX + 1, n).astype(np.int32)
    base, _ = _check(tok, "windows", ids, src, offs, 4, kw)
    assert base[-1][0] == 6000
    offs = np.asarray([0, 3, 3 + 9000, 3 + 9000 + 2], np.int64)  # one document of many windows
    n = int(offs[-1])
    ids, src = rng.integers(0, 1000, n).astype(np.int32), rng.integers(I32_MIN, I32_MAX + 1, n).astype(np.int32)
    base, _ = _check(tok, "windows", ids, src, offs, 7, dict(kw, overlap=2, mask_overlap=True))
    assert base[-1][3] > 2000
    lens = [5000, 3, 700, 64, 129, 0, 1] + rng.integers(0, 90, 100).tolist()  # split documents
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offs[-1])
    ids, src = rng.integers(0, 1000, n).astype(np.int32), rng.integers(I32_MIN, I32_MAX + 1, n).astype(np.int32)
    base, _ = _check(tok, "bestfit", ids, src, offs, 64, kw)
    assert base[-1][3] >= 4


def test_overlap_mask_trains_every_id_exactly_once(tok):
    rng = np.random.default_rng(4)
    lens = [0, 5, 300, 41, 1, 1000, 17]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offs[-1])
    ids, src = rng.integers(0, 1000, n).astype(np.int32), (np.arange(n) + 1000).astype(np.int32)  # (none of the fill values)
    for S, b, e in ((16, True, True), (9, False, True), (33, False, False)):
        C = S - b - e
        for overlap in (0, 1, C - 1):
            kw = dict(bos=b, eos=e, bos_value=-1, eos_value=-2, pad_value=-3, overlap=overlap)
            base, on = _check(tok, "windows", ids, src, offs, S, dict(kw, mask_overlap=True))
            _, off = _check(tok, "windows", ids, src, offs, S, dict(kw, mask_overlap=False))
            docs = base[3]
            for d in range(len(lens)):
                mine = on[docs == d]
                assert np.array_equal(np.sort(mine[mine != -3]), np.sort(np.concatenate([src[offs[d]:offs[d + 1]], [-1] * (b * len(mine)), [-2] * (e * len(mine))]).astype(np.int32)))
            assert ((off >= 1000).sum() > n) == (overlap > 0)


# ---- device forms -------------------------------------------------------------------------------------------------------------
def _dev_call(tok, layout, d_ids, n, d_offs, n_docs, spec, overlap, lab, out, cap, stream, labeled=True):
    """out: dict of torch tensors (ids, pos, and the layout's).  Returns the host counts of BESTFIT, else None."""
    p = lambda k: out[k].data_ptr() if out.get(k) is not None else 0
    if layout in ("concat", "pad"):
        if labeled:
            return tok.make_rows_labeled_device(d_ids, n, d_offs, n_docs, spec, p("ids"), cap, lab, p("pos"), p("aux"), p("counts"), stream)
        return tok.make_rows_device(d_ids, n, d_offs, n_docs, spec, p("ids"), cap, p("pos"), p("aux"), p("counts"), stream)
    if layout == "bestfit":
        if labeled:
            return tok.pack_rows_labeled_device(d_ids, n, d_offs, n_docs, spec, p("ids"), cap, lab, p("pos"), p("aux"), p("len"), p("docs"), stream)
        return tok.pack_rows_device(d_ids, n, d_offs, n_docs, spec, p("ids"), cap, p("pos"), p("aux"), p("len"), p("docs"), stream)
    if labeled:
        return tok.window_rows_labeled_device(d_ids, n, d_offs, n_docs, spec, overlap, p("ids"), cap, lab, p("pos"), p("len"), p("docs"),
                                              p("starts"), p("counts"), stream)
    return tok.window_rows_device(d_ids, n, d_offs, n_docs, spec, overlap, p("ids"), cap, p("pos"), p("len"), p("docs"), p("starts"),
                                  p("counts"), stream)


def _dev_out(layout, cap, S, n_docs, dev, shift=0, fill=77):
    import torch
    slots, nseg = max(cap * S, 1), n_docs + 2 * cap + 2
    out = {"ids": torch.full((slots + 8,), fill, dtype=torch.int32, device=dev)[shift:],
           "pos": torch.full((slots + 8,), fill, dtype=torch.int32, device=dev)[shift:],
           "counts": torch.full((4,), fill, dtype=torch.int64, device=dev)}
    if layout in ("concat", "pad"):
        out["aux"] = torch.full((n_docs + cap + 2,), fill, dtype=torch.int32, device=dev)
    elif layout == "bestfit":
        out.update(aux=torch.full((nseg,), fill, dtype=torch.int32, device=dev), len=torch.full((cap + 1,), fill, dtype=torch.int32, device=dev),
                   docs=torch.full((nseg,), fill, dtype=torch.int64, device=dev))
    else:
        out.update(len=torch.full((cap + 1,), fill, dtype=torch.int32, device=dev), docs=torch.full((cap + 1,), fill, dtype=torch.int64, device=dev),
                   starts=torch.full((cap + 1,), fill, dtype=torch.int64, device=dev))
    return out


def _case(rng, n_docs=30, hi=400):
    lens = rng.integers(0, hi, n_docs)
    lens[::7] = 0
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offs[-1])
    return rng.integers(0, 1000, n).astype(np.int32), rng.integers(I32_MIN, I32_MAX + 1, n).astype(np.int32), offs


@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_device_forms_with_pointers_off_the_16_byte_grid(tok, layout):
    """ids and src offset by 0 .. 3 elements independently, dst and the id rows likewise: the four-dword loads, the funnel and the
    int4 stores each take their aligned and their unaligned path per stream.  The slots around the outputs keep their fill."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    ids, src, offs = _case(rng, 200, 120)
    n, n_docs, S = len(ids), len(offs) - 1, 48
    kw = dict(bos=True, eos=True, bos_value=-1, eos_value=-2, pad_value=-3, overlap=5 if layout == "windows" else 0)
    spec = _rspec(layout, S, kw)
    truth = lr.label_rows(layout, src, offs, S, **kw)
    rows = truth.shape[0]
    assert rows * S > 2 * TILE
    stream = torch.cuda.current_stream(dev).cuda_stream
    d_offs = torch.from_numpy(offs).to(dev)
    ref = None
    for s_ids, s_src, s_out, s_dst in ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 2, 3, 0), (3, 1, 0, 2), (2, 2, 1, 1), (0, 3, 2, 3)):
        d_ids = torch.full((n + 8,), -7, dtype=torch.int32, device=dev)[s_ids:s_ids + n]
        d_ids.copy_(torch.from_numpy(ids))
        d_src = torch.full((n + 8,), -7, dtype=torch.int32, device=dev)[s_src:s_src + n]
        d_src.copy_(torch.from_numpy(src))
        dst = torch.full((rows * S + 8,), 77, dtype=torch.int32, device=dev)
        out = _dev_out(layout, rows, S, n_docs, dev, shift=s_out)
        assert d_ids.data_ptr() % 16 == 4 * s_ids and d_src.data_ptr() % 16 == 4 * s_src and dst[s_dst:].data_ptr() % 16 == 4 * s_dst
        lab = _lab(kw, d_src.data_ptr(), dst[s_dst:].data_ptr())
        _dev_call(tok, layout, d_ids.data_ptr(), n, d_offs.data_ptr(), n_docs, spec, kw["overlap"], lab, out, rows, stream)
        assert tok.device_status_pos(stream)[0] == 0
        h = dst.cpu().numpy()
        assert np.array_equal(h[s_dst:s_dst + rows * S].reshape(rows, S), truth), (s_ids, s_src, s_out, s_dst)
        assert (h[:s_dst] == 77).all() and (h[s_dst + rows * S:] == 77).all()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        assert (got["ids"][rows * S:] == 77).all()
        if ref is None:  # the counterpart, aligned, once
            base = _dev_out(layout, rows, S, n_docs, dev)
            _dev_call(tok, layout, d_ids.data_ptr(), n, d_offs.data_ptr(), n_docs, spec, kw["overlap"], None, base, rows, stream, labeled=False)
            assert tok.device_status_pos(stream)[0] == 0
            ref = {k: v.cpu().numpy() for k, v in base.items()}
        for k in ref:
            if layout == "bestfit" and k == "counts":
                continue  # (BESTFIT's counts are the host's)
            m = rows * S if k in ("ids", "pos") else len(ref[k])
            assert np.array_equal(got[k][:m], ref[k][:m]), (k, s_ids, s_src, s_out, s_dst)


def test_funnel_loads_are_chosen_per_stream():
    """TD_ROWS_FUNNEL=1 (read once a process, so a child process): CONCAT and PAD read an ALIGNED stream as two int4 and a funnel and a
    misaligned one as four dwords.  The misalignment cases above offset ids and src independently, so the child covers ids by the
    funnel with src by dwords, the reverse, and both either way."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, TD_ROWS_FUNNEL="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", __file__, "-k",
                        "off_the_16_byte_grid and (concat or pad)"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "2 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]


@pytest.mark.parametrize("layout", ["concat", "pad", "windows"])
def test_device_forms_are_asynchronous_on_a_side_stream(tok, layout):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(12)
    ids, src, offs = _case(rng, 60, 600)
    n, n_docs, S = len(ids), len(offs) - 1, 64
    kw = dict(bos=True, eos=False, bos_value=-1, eos_value=-2, pad_value=-3, overlap=9 if layout == "windows" else 0, mask_overlap=layout == "windows")
    truth = lr.label_rows(layout, src, offs, S, **kw)
    rows = truth.shape[0]
    d_ids, d_src, d_offs = torch.from_numpy(ids).to(dev), torch.from_numpy(src).to(dev), torch.from_numpy(offs).to(dev)
    dst = torch.full((rows * S,), 77, dtype=torch.int32, device=dev)
    out = _dev_out(layout, rows, S, n_docs, dev)
    side = torch.cuda.Stream(device=dev)
    x = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize()
    for _ in range(10):  # torch's default stream is busy meanwhile
        x = x @ x * 1e-3
    rc = _dev_call(tok, layout, d_ids.data_ptr(), n, d_offs.data_ptr(), n_docs, _rspec(layout, S, kw), kw["overlap"],
                   _lab(kw, d_src.data_ptr(), dst.data_ptr()), out, rows, side.cuda_stream)
    assert rc is None  # (nothing comes back but through device_status)
    tok.device_status(side.cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy().reshape(rows, S), truth)
    assert out["counts"].cpu().numpy()[0] == rows


@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_capacity_and_bad_offsets_are_status_codes_and_write_nothing(tok, layout):
    import torch
    from tokendagger_amd import capi
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(13)
    ids, src, offs = _case(rng)
    n, n_docs, S = len(ids), len(offs) - 1, 32
    kw = dict(bos=True, eos=True, overlap=0)
    spec = _rspec(layout, S, kw)
    rows = lr.label_rows(layout, src, offs, S, **kw).shape[0]
    stream = torch.cuda.current_stream(dev).cuda_stream
    d_ids, d_src = torch.from_numpy(ids).to(dev), torch.from_numpy(src).to(dev)
    # host form: capacity
    host = {"concat": tok.make_rows_labeled, "pad": tok.make_rows_labeled, "bestfit": tok.pack_rows_labeled, "windows": tok.window_rows_labeled}[layout]
    with pytest.raises(capi.TokenDaggerHipError) as e:
        host(ids, src, offs, spec, _lab(kw), rows_capacity=rows - 1)
    assert e.value.code == capi.TD_E_CAPACITY and e.value.counts[0] == rows
    # device form: capacity, then bad offsets (decreasing; CONCAT and PAD, whose counterparts take such offsets as they come: an end
    # beyond n_tokens); dst keeps its fill both times
    bad = offs.copy()
    bad[3] = bad[2] - 1
    beyond = layout in ("concat", "pad")
    for d_offs_np, want in ((offs, capi.TD_E_CAPACITY), (offs if beyond else bad, capi.TD_E_INVALID)):
        cap = rows - 1 if want == capi.TD_E_CAPACITY else rows
        n = len(ids) - (5 if beyond and want == capi.TD_E_INVALID else 0)
        d_offs = torch.from_numpy(d_offs_np).to(dev)
        dst = torch.full((rows * S,), 77, dtype=torch.int32, device=dev)
        out = _dev_out(layout, rows, S, n_docs, dev)
        lab = _lab(kw, d_src.data_ptr(), dst.data_ptr())
        if layout == "bestfit":
            with pytest.raises(capi.TokenDaggerHipError) as e:
                _dev_call(tok, layout, d_ids.data_ptr(), n, d_offs.data_ptr(), n_docs, spec, 0, lab, out, cap, stream)
            assert e.value.code == want and (want != capi.TD_E_CAPACITY or e.value.counts[0] == rows)
        else:
            _dev_call(tok, layout, d_ids.data_ptr(), n, d_offs.data_ptr(), n_docs, spec, 0, lab, out, cap, stream)
            code, pos = tok.device_status_pos(stream)
            assert code == want, (code, pos)
            if want == capi.TD_E_CAPACITY:
                assert pos == rows and out["counts"].cpu().numpy()[0] == rows
        torch.cuda.synchronize()
        assert (dst.cpu().numpy() == 77).all(), (layout, want)
        assert (out["ids"].cpu().numpy() == 77).all()
    _check(tok, layout, ids, src, offs, S, kw)  # the handle is fine afterwards


def test_spec_errors(tok):
    import torch
    from tokendagger_amd import capi
    dev = torch.device("cuda", 0)
    ids, src, offs = np.arange(10, dtype=np.int32), np.arange(10, dtype=np.int32), np.asarray([0, 4, 10], np.int64)
    d_ids, d_src, d_offs = torch.from_numpy(ids).to(dev), torch.from_numpy(src).to(dev), torch.from_numpy(offs).to(dev)
    dst = torch.full((64,), 77, dtype=torch.int32, device=dev)
    out = _dev_out("concat", 4, 8, 2, dev)
    spec, wspec = capi.rows_spec(8), capi.windows_spec(8)
    good = dict(bos_value=-100, eos_value=-100, pad_value=-100)

    h_dst, h_out, h_counts = np.full(64, 77, np.int32), np.full(64, 77, np.int32), np.zeros(4, np.int64)

    def host_call(layout, sp, **kw):  # the C entry point itself: src / dst as given, NULL included
        lab = capi.rows_labels(kw.pop("src", src.ctypes.data), kw.pop("dst", h_dst.ctypes.data), **{**good, **kw})
        head = (tok._h, ids.ctypes.data, 10, offs.ctypes.data, 2, ctypes.byref(sp))
        if layout == "concat":
            rc = tok._lib.td_make_rows_labeled(*head, h_out.ctypes.data, 4, None, None, h_counts.ctypes.data, ctypes.byref(lab))
        elif layout == "bestfit":
            outs = capi.PackOutputs(h_out.ctypes.data, None, None, None, None)
            rc = tok._lib.td_pack_rows_labeled(*head, ctypes.byref(outs), 4, h_counts.ctypes.data, ctypes.byref(lab))
        else:
            outs = capi.WindowOutputs(h_out.ctypes.data, None, None, None, None)
            rc = tok._lib.td_window_rows_labeled(*head, 0, ctypes.byref(outs), 4, h_counts.ctypes.data, ctypes.byref(lab))
        return rc, tok._lib.td_last_error(tok._h).decode()

    rc, _ = host_call("concat", spec)
    assert rc == 0 and (h_dst[:16] != 77).all() and (h_dst[16:] == 77).all()  # (the helper's good call works)
    h_dst[:], h_out[:] = 77, 77

    def dev_lab(**kw):
        return capi.rows_labels(kw.pop("src", d_src.data_ptr()), kw.pop("dst", dst.data_ptr()), **{**good, **kw})

    bad = [dict(bos_value=1 << 31), dict(eos_value=-(1 << 31) - 1), dict(pad_value=1 << 40), dict(flags=2), dict(flags=1), dict(src=0), dict(dst=0)]
    for kw in bad:
        rc, msg = host_call("concat", spec, **kw)
        assert rc == capi.TD_E_INVALID and "td_make_rows_labeled:" in msg, (kw, msg)
        with pytest.raises(capi.TokenDaggerHipError) as e:
            tok.make_rows_labeled_device(d_ids.data_ptr(), 10, d_offs.data_ptr(), 2, spec, out["ids"].data_ptr(), 4, dev_lab(**kw),
                                         d_counts=out["counts"].data_ptr())
        assert e.value.code == capi.TD_E_INVALID and "td_make_rows_labeled_device" in str(e.value), kw
        if kw != dict(flags=1):  # (TD_ROWLAB_MASK_OVERLAP is the windows' own flag)
            rc, msg = host_call("windows", wspec, **kw)
            assert rc == capi.TD_E_INVALID and "td_window_rows_labeled:" in msg, (kw, msg)
    rc, msg = host_call("bestfit", capi.pack_spec(8), flags=1)
    assert rc == capi.TD_E_INVALID and "TD_ROWS_WINDOWS" in msg
    # the counterpart's own checks come first: its message, not the label spec's
    rc, msg = host_call("concat", capi.rows_spec(8, pad=1 << 40), flags=2)
    assert rc == capi.TD_E_INVALID and "pad_id" in msg
    torch.cuda.synchronize()
    assert (h_dst == 77).all() and (h_out == 77).all()
    assert (dst.cpu().numpy() == 77).all() and (out["ids"].cpu().numpy() == 77).all()
    assert tok.device_status_pos(torch.cuda.current_stream(dev).cuda_stream)[0] == 0


# ---- the fused entry ----------------------------------------------------------------------------------------------------------
def _chat(n_conv, rng, long=False):
    words = ["hello", " world", " what", " is", " the", " answer", "?", " 42", "\n", " sure", " thing", "!"]
    docs = []
    for c in range(n_conv):
        turns = []
        for t in range(int(rng.integers(0, 5))):
            role = "assistant" if t % 2 else "user"
            body = "".join(rng.choice(words, int(rng.integers(0, 400 if long else 12))))
            turns.append(f"<|header_start|>{role}<|header_end|>{body}" + ("<|eot|>" if rng.random() < 0.85 else ""))
        docs.append(("<|begin_of_text|>" + "".join(turns)).encode() if turns else b"")
    offs = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    return np.frombuffer(b"".join(docs), dtype=np.uint8), offs


def _fused_parts(tok, wtok, text, doffs, layout, S, kw, lspec):
    specials = sorted(wtok._special_tokens)
    e_ids, e_offs, labels, _, _, lcounts = tok.encode_batch_span_labels(text, doffs, specials, lspec)
    base, lab_rows = _host(tok, layout, e_ids, labels, e_offs, S, kw)
    return e_ids, e_offs, labels, lcounts, base, lab_rows


@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_fused_entry_equals_labels_then_labeled_rows(tok, wtok, layout):
    from tokendagger_amd import capi
    rng = np.random.default_rng(20 + lr.LAYOUTS.index(layout))
    specials = sorted(wtok._special_tokens)
    opener = tok.encode_with_special_strs(OPENER.encode(), specials)[0].tolist()
    closers = [wtok.encode_single_token(c) for c in CLOSERS]
    lspec = capi.labels_spec([opener], closers, -100, True)
    S = 64
    kw = dict(bos=True, eos=True, bos_value=-100, eos_value=EOS, pad_value=-100)
    if layout == "windows":
        kw.update(overlap=8, mask_overlap=True)
    for text, doffs in (_chat(40, rng), _chat(3, rng), (np.zeros(0, np.uint8), np.zeros(3, np.int64)), _chat(1500, rng, long=True)):
        e_ids, e_offs, labels, lcounts, base, lab_rows = _fused_parts(tok, wtok, text, doffs, layout, S, kw, lspec)
        _eq(lab_rows, lr.label_rows(layout, labels, e_offs, S, **kw), (layout, "parts"))
        want = {"concat": {}, "pad": {}, "bestfit": dict(lengths=True, docs=True), "windows": {}}[layout]
        r = tok.encode_batch_span_label_rows(text, doffs, specials, lspec, _rspec(layout, S, kw), _lab(kw), overlap=kw.get("overlap", 0),
                                             positions=True, **want)
        assert len(r) == len(base) + 2
        for k, (p, q) in enumerate(zip(r, base)):
            _eq(p, q, (layout, "fused output", k))
        _eq(r[-2], lab_rows, (layout, "fused labels"))
        assert np.array_equal(r[-1], lcounts)
    assert len(text) > (1 << 20) and lcounts[1] > 100  # the last case: the device search for the specials is the path taken
    # the Tokenizer method
    w = wtok.encode_batch_to_labeled_rows(text, doffs, S, layout=layout, open=[OPENER], close=CLOSERS, bos=BOS, eos=EOS, pad=PAD,
                                          label_eos=EOS, overlap=kw.get("overlap", 0), mask_overlap=kw.get("mask_overlap", False),
                                          positions=True, docs=layout == "bestfit")
    _eq(w.labels, lab_rows, (layout, "wrapper labels"))
    _eq(w.rows.ids, base[0], (layout, "wrapper ids"))
    _eq(w.rows.counts, base[-1], (layout, "wrapper counts"))
    w2 = wtok.ids_to_labeled_rows(e_ids, labels, e_offs, S, layout=layout, bos=BOS, eos=EOS, pad=PAD, label_eos=EOS,
                                  overlap=kw.get("overlap", 0), mask_overlap=kw.get("mask_overlap", False), positions=True)
    _eq(w2.labels, lab_rows, (layout, "ids_to_labeled_rows labels"))
    _eq(w2.rows.ids, base[0], (layout, "ids_to_labeled_rows ids"))
    _eq(w2.rows.positions, base[1], (layout, "ids_to_labeled_rows positions"))


def test_fused_entry_errors(tok, wtok):
    from tokendagger_amd import capi, wrapper
    rng = np.random.default_rng(5)
    text, doffs = _chat(30, rng)
    specials = sorted(wtok._special_tokens)
    lspec = capi.labels_spec([[1, 2]], [3], -100, True)
    kw = dict(bos=True, eos=True)
    with pytest.raises(capi.TokenDaggerHipError) as e:
        tok.encode_batch_span_label_rows(text, doffs, specials, lspec, _rspec("pad", 16, kw), _lab(kw), rows_capacity=7)
    assert e.value.code == capi.TD_E_CAPACITY and e.value.counts[0] == 30
    with pytest.raises(capi.TokenDaggerHipError) as e:
        tok.encode_batch_span_label_rows(text, doffs, specials, lspec, _rspec("concat", 16, kw), capi.rows_labels(0, 0, mask_overlap=True))
    assert e.value.code == capi.TD_E_INVALID
    # a field that the layout does not have
    outs = capi.LabelRowsOutputs(*([np.empty(4096, np.int64).ctypes.data] * 8))
    counts = np.zeros(8, np.int64)
    o = np.ascontiguousarray(doffs)
    rc = tok._lib.td_encode_batch_span_label_rows(tok._h, text.ctypes.data, o.ctypes.data, len(o) - 1, None, None, 0, ctypes.byref(lspec),
                                                  ctypes.byref(_rspec("concat", 16, kw)), 0, ctypes.byref(_lab(kw)), ctypes.byref(outs), 1,
                                                  counts.ctypes.data, counts[4:].ctypes.data)
    assert rc == capi.TD_E_INVALID
    with pytest.raises(wrapper.TokenDaggerError):
        wtok.encode_batch_to_labeled_rows(text, doffs, 1, layout="windows", open=[OPENER], close=CLOSERS, bos=BOS, eos=EOS)


def test_equals_the_two_call_recipe_without_bos_and_eos(tok, golden):
    """Without BOS / EOS, dst is what the existing call makes of the labels with pad = pad_value (test_label_rows_align_with_id_rows
    of tests/test_gpu_labels.py)."""
    from tokendagger_amd import capi
    ids, offs = golden["enc"].astype(np.int32), golden["enc_offsets"].astype(np.int64)
    f = np.argsort(-np.bincount(ids))[:6].tolist()
    IGN, S = -100, 512
    labels = tok.span_labels(ids, offs, capi.labels_spec([[f[1]], [f[2], f[3]]], [f[0]], IGN, True))[0]
    assert (labels != IGN).sum() > 1000
    lab = capi.rows_labels(0, 0, IGN, IGN, IGN)
    two = {"concat": tok.make_rows(labels, offs, capi.rows_spec(S, capi.TD_ROWS_CONCAT, -1, -1, IGN))[0],
           "pad": tok.make_rows(labels, offs, capi.rows_spec(S, capi.TD_ROWS_PAD, -1, -1, IGN))[0],
           "bestfit": tok.pack_rows(labels, offs, capi.pack_spec(S, -1, -1, IGN))[0],
           "windows": tok.window_rows(labels, offs, capi.windows_spec(S, -1, -1, IGN), 64)[0]}
    one = {"concat": tok.make_rows_labeled(ids, labels, offs, capi.rows_spec(S, capi.TD_ROWS_CONCAT, -1, -1, PAD), lab)[-1],
           "pad": tok.make_rows_labeled(ids, labels, offs, capi.rows_spec(S, capi.TD_ROWS_PAD, -1, -1, PAD), lab)[-1],
           "bestfit": tok.pack_rows_labeled(ids, labels, offs, capi.pack_spec(S, -1, -1, PAD), lab)[-1],
           "windows": tok.window_rows_labeled(ids, labels, offs, capi.windows_spec(S, -1, -1, PAD), lab, 64)[-1]}
    for name in lr.LAYOUTS:
        _eq(one[name], two[name], name)
