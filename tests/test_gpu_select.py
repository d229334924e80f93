"""Document selection on the GPU (td_select_docs, td_select_docs_device, td_encode_batch_select, the Python methods) against the
truth of tests/select_truth.py.  All comparisons are exact.  No case here makes the device fault: every error is one the library
reports by a status code."""
import numpy as np
import pytest

import helpers as H
import labeled_rows_truth as lt
import rows_truth as rt
import select_truth as st

pytestmark = pytest.mark.gpu

BOS, EOS = 200000, 200001  # Llama-4 <|begin_of_text|>, <|end_of_text|>
TILE = 4096                # output slots a workgroup writes per tile
CHUNK, PASS = 1024, 1024   # selection entries per chunk of the scan, chunks per pass of the chunk scan


@pytest.fixture(scope="module")
def tok():
    from tokendagger_amd import capi
    pat, mr, special = H.llama4()
    return capi.HipTokenizer(pat, mr, special, device=0)


@pytest.fixture(scope="module")
def golden_labels(golden):
    return np.random.default_rng(9).integers(-(1 << 31), 1 << 31, len(golden["enc"])).astype(np.int32)


def _spec(mn=0, mx=-1):
    from tokendagger_amd import capi
    return capi.select_spec(mn, mx)


def _check(tok, ids, offs, sel, mn=0, mx=-1, labels=None, truth=st.select_numpy, t=None, docs=True):
    t = t if t is not None else truth(ids, offs, sel, mn, mx, labels=labels)
    g = tok.select_docs(ids, offs, sel, _spec(mn, mx), labels=labels, docs=docs)
    assert np.array_equal(g[4], t[4]), (g[4], t[4])
    assert g[0].dtype == np.int32 and np.array_equal(g[0], t[0])
    if labels is None:
        assert g[1] is None
    else:
        assert g[1].dtype == np.int32 and np.array_equal(g[1], t[1])
    assert g[2].dtype == np.int64 and np.array_equal(g[2], t[2])
    if docs:
        assert g[3].dtype == np.int64 and np.array_equal(g[3], t[3])
    else:
        assert g[3] is None
    return t


def test_golden_ids(tok, golden, golden_labels):
    ids, offs = golden["enc"], golden["enc_offsets"]
    n_docs = len(offs) - 1
    assert n_docs > 3 * CHUNK and len(ids) > 100 * TILE
    rng = np.random.default_rng(21)
    L = np.diff(offs)
    q = [int(x) for x in np.quantile(L, [0.25, 0.5, 0.75])]
    assert 0 < q[0] < q[2] < L.max()
    for sel in (None, rng.permutation(n_docs), rng.integers(0, n_docs, 2 * n_docs)):
        for mn, mx in ((0, -1), (q[0], q[2]), (q[1], -1), (0, q[1]), (q[1], q[1])):
            t = _check(tok, ids, offs, sel, mn, mx, labels=golden_labels)
            if (mn, mx) == (q[0], q[2]):
                assert t[4][0] > 0 and t[4][2] > 0 and t[4][3] > 0  # kept, short and long are all there
            _check(tok, ids, offs, sel, mn, mx, t=(t[0], None, t[2], t[3], t[4]), docs=False)
    t = _check(tok, ids, offs, None)
    assert np.array_equal(t[0], ids) and np.array_equal(t[2], offs)


def test_small_cases_against_brute_force(tok):
    rng = np.random.default_rng(5)
    for it in range(60):
        ids, labels, offs, sel, mn, mx = st.random_case(rng)
        _check(tok, ids, offs, sel, mn, mx, labels=labels if it % 2 else None, truth=st.select_brute, docs=it % 3 != 0)


def _docs_at_borders():
    """Lengths whose documents, in this order, are 4095, 4096, 4097 and 9000 ids long and then begin 1, 2 and 3 ids before a tile
    border (a filler in front of each)."""
    lengths, at = [], 0
    for n in (4095, 4096, 4097, 9000):
        lengths.append(n)
        at += n
    for before, n in ((1, 6), (2, 5), (3, 11)):
        filler = (TILE - before - at % TILE) % TILE or TILE  # (what is missing to `before` ids in front of a border; never 0)
        lengths += [filler, n]
        at += filler
        assert at % TILE == TILE - before
        at += n
    return np.array(lengths, np.int64)


def test_tile_and_chunk_edges(tok):
    rng = np.random.default_rng(6)

    def case(lengths):
        offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        ids = rng.integers(0, 200000, int(offs[-1])).astype(np.int32)
        return ids, rng.integers(-5, 5, int(offs[-1])).astype(np.int32), offs

    # documents of a tile's length and around it, one longer than two tiles, documents that begin just before a border
    lengths = _docs_at_borders()
    ids, labels, offs = case(lengths)
    n = len(lengths)
    _check(tok, ids, offs, None, labels=labels)                          # aligned sources, partial int4 at the documents' ends
    _check(tok, ids, offs, np.arange(n)[::-1].copy(), labels=labels)     # the same documents at other shifts
    ids2, labels2, offs2 = case(np.concatenate([[1], lengths, [2]]))     # every source one id further: misaligned reads
    _check(tok, ids2, offs2, np.arange(1, n + 1), labels=labels2)
    _check(tok, ids2, offs2, np.concatenate([[n + 1], np.arange(1, n + 1), [0]]))  # ... and every destination two further
    _check(tok, ids, offs, rng.integers(0, n, 3 * n), mx=5000)
    # 5 000 kept empty documents between two non-empty ones (more than LDS holds), 4 000 (LDS, several loads), both in one tile
    for empties, a, b in ((5000, 10, 10), (4000, 3, 5), (5000, 5000, 4097), (4351, 1, 1), (4352, 1, 1), (4350, 1, 1)):
        ids, labels, offs = case([a] + [0] * empties + [b])
        t = _check(tok, ids, offs, None, labels=labels)
        assert t[4].tolist() == [empties + 2, a + b, 0, 0]
    ids, labels, offs = case([0] * 3000 + [7] + [0] * 6000 + [4096, 1] + [0] * 5000)  # empty runs at both ends and in between
    _check(tok, ids, offs, None, labels=labels)
    _check(tok, ids, offs, rng.permutation(len(offs) - 1))
    # only the last entry is kept
    ids, labels, offs = case(np.concatenate([rng.integers(0, 50, 3000), [50]]))
    t = _check(tok, ids, offs, None, 50, -1, labels=labels)
    assert t[4].tolist() == [1, 50, 3000, 0] and t[3].tolist() == [3000]
    # nothing kept, nothing listed, no documents
    t = _check(tok, ids, offs, None, 51, -1, labels=labels)
    assert t[4].tolist() == [0, 0, 3001, 0] and t[2].tolist() == [0]
    t = _check(tok, ids, offs, None, 0, 0)  # only the empty ones
    assert t[4][1] == 0 and t[4][0] > 0 and t[4][3] > 0
    t = _check(tok, ids, offs, np.zeros(0, np.int64), labels=labels)
    assert t[4].tolist() == [0, 0, 0, 0] and t[2].tolist() == [0]
    t = _check(tok, np.zeros(0, np.int32), np.zeros(1, np.int64), None)
    assert t[4].tolist() == [0, 0, 0, 0] and t[2].tolist() == [0]


def test_more_entries_than_one_pass_of_the_chunk_scan(tok):
    rng = np.random.default_rng(7)
    lengths = rng.integers(0, 2, 5000)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ids = rng.integers(0, 200000, int(offs[-1])).astype(np.int32)
    sel = rng.integers(0, 5000, CHUNK * PASS + 5)
    t = _check(tok, ids, offs, sel)
    assert t[4][0] == len(sel) and t[4][1] > 400000
    t = _check(tok, ids, offs, sel, 1, 1)
    assert t[4][0] == t[4][1] and t[4][2] > 400000


def _device_call(tok, ids, offs, sel, mn, mx, cap, labels=None, n_tokens=None, want_docs=True, fill=77):
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d_ids, d_offs = up(ids, np.int32), up(offs, np.int64)
    d_sel = up(sel, np.int64) if sel is not None else None
    d_lab = up(labels, np.int32) if labels is not None else None
    n_sel = len(offs) - 1 if sel is None else len(sel)
    stream = torch.cuda.current_stream(dev).cuda_stream
    bufs = {"ids": torch.full((max(cap, 1),), fill, dtype=torch.int32, device=dev),
            "labels": torch.full((max(cap, 1),), fill, dtype=torch.int32, device=dev),
            "offsets": torch.full((n_sel + 1,), fill, dtype=torch.int64, device=dev),
            "docs": torch.full((max(n_sel, 1),), fill, dtype=torch.int64, device=dev)}
    counts = torch.full((4,), fill, dtype=torch.int64, device=dev)
    tok.select_docs_device(d_ids.data_ptr() if len(ids) else 0, len(ids) if n_tokens is None else n_tokens, d_offs.data_ptr(), len(offs) - 1,
                           d_sel.data_ptr() if d_sel is not None else 0, n_sel, _spec(mn, mx),
                           bufs["ids"].data_ptr(), cap, bufs["offsets"].data_ptr(), bufs["docs"].data_ptr() if want_docs else 0,
                           counts.data_ptr(), d_lab.data_ptr() if d_lab is not None else 0,
                           bufs["labels"].data_ptr() if d_lab is not None else 0, stream)
    return bufs, counts, stream


def _untouched(bufs):
    return all((b == 77).all().item() for b in bufs.values())


def test_device_form_on_torch_equals_host(tok, golden, golden_labels):
    ids, offs = golden["enc"], golden["enc_offsets"]
    n_docs = len(offs) - 1
    rng = np.random.default_rng(8)
    med = int(np.median(np.diff(offs)))
    for sel, mn, mx, labels, want_docs in ((None, 0, -1, None, True), (rng.permutation(n_docs), med, -1, golden_labels, True),
                                           (rng.integers(0, n_docs, 2 * n_docs), 3, 4 * med, golden_labels, False)):
        h = tok.select_docs(ids, offs, sel, _spec(mn, mx), labels=labels)
        K, T = int(h[4][0]), int(h[4][1])
        bufs, counts, stream = _device_call(tok, ids, offs, sel, mn, mx, T + 5, labels=labels, want_docs=want_docs)
        tok.device_status(stream)
        assert np.array_equal(counts.cpu().numpy(), h[4])
        want = {"ids": (h[0], T), "labels": (h[1], T if labels is not None else 0), "offsets": (h[2], K + 1), "docs": (h[3], K if want_docs else 0)}
        for k, (ref, n) in want.items():
            got = bufs[k].cpu().numpy()
            assert n == 0 or np.array_equal(got[:n], ref), k
            assert (got[n:] == 77).all(), k


def test_errors_host_and_device(tok, golden, golden_labels):
    from tokendagger_amd import capi
    ids, offs = golden["enc"][:50000], golden["enc_offsets"]
    offs = np.concatenate([offs[:int(np.searchsorted(offs, 50000, side="right"))], [50000]]).astype(np.int64)
    labels = golden_labels[:50000]
    n_docs = len(offs) - 1
    rng = np.random.default_rng(10)
    sel = rng.permutation(n_docs).astype(np.int64)
    t = st.select_numpy(ids, offs, sel, 2, -1, labels=labels)
    T = int(t[4][1])

    def good_call_follows():  # the next good call on the same handle
        bufs, counts, stream = _device_call(tok, ids, offs, sel, 2, -1, T, labels=labels)
        tok.device_status(stream)
        assert np.array_equal(counts.cpu().numpy(), t[4]) and np.array_equal(bufs["ids"].cpu().numpy()[:T], t[0])
        assert np.array_equal(bufs["labels"].cpu().numpy()[:T], t[1])

    # capacity one below T
    with pytest.raises(capi.TokenDaggerHipError) as ei:
        tok.select_docs(ids, offs, sel, _spec(2), labels=labels, ids_capacity=T - 1)
    assert ei.value.code == capi.TD_E_CAPACITY and ei.value.counts[1] == T
    bufs, counts, stream = _device_call(tok, ids, offs, sel, 2, -1, T - 1, labels=labels)
    rc, where = tok.device_status_pos(stream)
    assert rc == capi.TD_E_CAPACITY and where == T
    assert counts.cpu().tolist()[1] == T and _untouched(bufs)
    tok.device_status(stream)  # (cleared)
    good_call_follows()
    # an entry that is no document, with its position
    for pos, v in ((0, n_docs), (n_docs // 2, -1), (n_docs - 1, n_docs)):
        bad = sel.copy()
        bad[pos] = v
        with pytest.raises(capi.TokenDaggerHipError) as ei:
            tok.select_docs(ids, offs, bad, _spec(2), labels=labels, ids_capacity=T)
        assert ei.value.code == capi.TD_E_INVALID and f"sel[{pos}]" in str(ei.value)
        bufs, counts, stream = _device_call(tok, ids, offs, bad, 2, -1, T, labels=labels)
        rc, where = tok.device_status_pos(stream)
        assert rc == capi.TD_E_INVALID and where == pos and _untouched(bufs)
        good_call_follows()
    # offsets: a decreasing pair inside a listed document, and n_tokens below the last offset
    d = 1 + int(np.flatnonzero(np.diff(offs[1:]) > 0)[0])  # document d is not empty
    dec = offs.copy()
    dec[d], dec[d + 1] = offs[d + 1], offs[d]              # documents d - 1 and d + 1 grow, d decreases
    pos = int(np.flatnonzero(sel == d)[0])
    bufs, counts, stream = _device_call(tok, ids, dec, sel, 0, -1, 2 * len(ids), labels=labels)
    rc, where = tok.device_status_pos(stream)
    assert rc == capi.TD_E_INVALID and where == pos and _untouched(bufs)
    last = int(np.flatnonzero(sel == n_docs - 1)[0])
    assert offs[n_docs - 1] < 49999  # (only the last document reaches beyond 49 999 ids)
    bufs, counts, stream = _device_call(tok, ids, offs, sel, 0, -1, 2 * len(ids), labels=labels, n_tokens=49999)
    rc, where = tok.device_status_pos(stream)
    assert rc == capi.TD_E_INVALID and where == last and _untouched(bufs)
    good_call_follows()
    # the same bad pair in a document that is NOT listed: fine
    rest = sel[sel != d]
    bufs, counts, stream = _device_call(tok, ids, dec, rest, 0, -1, 2 * len(ids))
    tok.device_status(stream)
    K, T2 = [int(x) for x in counts.cpu().tolist()[:2]]
    assert K == n_docs - 1
    o = bufs["offsets"].cpu().numpy()[:K + 1]
    got = bufs["ids"].cpu().numpy()[:T2]
    for k in range(K):  # the documents of the result, from the offsets as they are
        src = int(rest[k])
        assert np.array_equal(got[o[k]:o[k + 1]], ids[dec[src]:dec[src + 1]])
    assert np.array_equal(np.diff(o), (dec[1:] - dec[:-1])[rest])
    # spec and argument errors, before any launch
    for bad in (capi.select_spec(-1), capi.select_spec(0, -2), capi.select_spec(3, 2), capi.select_spec(0, flags=1)):
        with pytest.raises(capi.TokenDaggerHipError) as ei:
            tok.select_docs(ids, offs, sel, bad, ids_capacity=T)
        assert ei.value.code == capi.TD_E_INVALID
    import ctypes
    c = np.zeros(4, np.int64)
    o_out = np.full(n_docs + 1, 77, np.int64)
    out = np.full(len(ids), 77, np.int32)
    sp = _spec()
    rc = tok._lib.td_select_docs(tok._h, ids.ctypes.data, None, len(ids), offs.ctypes.data, n_docs, None, n_docs - 1, ctypes.byref(sp),
                                 out.ctypes.data, None, len(ids), o_out.ctypes.data, None, c.ctypes.data)
    assert rc == capi.TD_E_INVALID and (out == 77).all() and (o_out == 77).all()
    rc = tok._lib.td_select_docs(tok._h, ids.ctypes.data, labels.ctypes.data, len(ids), offs.ctypes.data, n_docs, None, n_docs, ctypes.byref(sp),
                                 out.ctypes.data, None, len(ids), o_out.ctypes.data, None, c.ctypes.data)  # labels without out_labels
    assert rc == capi.TD_E_INVALID and (out == 77).all() and (o_out == 77).all()


def test_composition_with_the_row_layouts(tok, golden, golden_labels):
    from tokendagger_amd import capi
    ids, offs, labels = golden["enc"], golden["enc_offsets"], golden_labels
    n_docs = len(offs) - 1
    p = np.random.default_rng(12).permutation(n_docs)
    s_ids, s_lab, s_offs, s_docs, _ = tok.select_docs(ids, offs, p, labels=labels)
    n_ids, n_lab, n_offs, _, _ = st.select_numpy(ids, offs, p, labels=labels)  # the numpy-permuted input
    S = 512
    spec = capi.rows_spec(S, capi.TD_ROWS_CONCAT, BOS, EOS, 0)
    truth = rt.rows_numpy(n_ids, n_offs, S, rt.CONCAT, BOS, EOS, 0)
    got = tok.make_rows(s_ids, s_offs, spec, positions=True)
    for g, w in zip(got, truth):
        assert np.array_equal(g, w)
    lab = capi.rows_labels(0, 0, -100, EOS, -100)
    got = tok.make_rows_labeled(s_ids, s_lab, s_offs, spec, lab, positions=True)
    for g, w in zip(got[:4], truth):
        assert np.array_equal(g, w)
    assert np.array_equal(got[4], lt.label_rows("concat", n_lab, n_offs, S, bos=True, eos=True, bos_value=-100, eos_value=EOS, pad_value=-100))


def test_fused_equals_encode_then_select(tok, golden):
    text, offs = golden["text"], golden["offsets"]
    ids, toffs = tok.encode_batch(text, offs)
    n_docs = len(offs) - 1
    p = np.random.default_rng(13).permutation(n_docs)
    for sel, mn, mx in ((p, 8, -1), (None, 0, -1), (p[:100], 0, 300)):
        t = st.select_numpy(ids, toffs, sel, mn, mx)
        g = tok.encode_batch_select(text, offs, sel, _spec(mn, mx))
        assert np.array_equal(g[0], t[0]) and np.array_equal(g[1], t[2]) and np.array_equal(g[2], t[3]) and np.array_equal(g[3], t[4])
    assert t[4][2] == 0 and t[4][3] > 0
    e = tok.encode_batch_select(b"", np.zeros(4, np.int64), [2, 0, 0])  # three empty documents
    assert len(e[0]) == 0 and e[1].tolist() == [0, 0, 0, 0] and e[2].tolist() == [2, 0, 0] and e[3].tolist() == [3, 0, 0, 0]


def test_tokenizer_methods(golden):
    import tokendagger as tiktoken
    pat, mr, special = H.llama4()
    tk = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    text, offs = golden["text"], golden["offsets"]
    ids, toffs = tk.encode_batch_to_numpy(text, offs)
    labels = np.random.default_rng(15).integers(-100, 200000, len(ids)).astype(np.int32)
    p = np.random.default_rng(14).permutation(len(offs) - 1)
    t = st.select_numpy(ids, toffs, p, 8, 2000, labels=labels)
    r = tk.select_docs(ids, toffs, p, min_len=8, max_len=2000)
    assert len(r) == 3 and np.array_equal(r[0], t[0]) and np.array_equal(r[1], t[2]) and np.array_equal(r[2], t[3])
    r = tk.select_docs(ids, toffs, p, min_len=8, max_len=2000, labels=labels)
    assert len(r) == 4 and np.array_equal(r[0], t[0]) and np.array_equal(r[1], t[1]) and np.array_equal(r[2], t[2]) and np.array_equal(r[3], t[3])
    r = tk.encode_batch_select(text, offs, p, min_len=8, max_len=2000)
    assert np.array_equal(r[0], t[0]) and np.array_equal(r[1], t[2]) and np.array_equal(r[2], t[3])
    r = tk.select_docs(ids, toffs)
    assert np.array_equal(r[0], ids) and np.array_equal(r[1], toffs)
    # shuffle, then labeled rows: the composition through the Tokenizer
    s_ids, s_lab, s_offs, _ = tk.select_docs(ids, toffs, p, labels=labels)
    n = st.select_numpy(ids, toffs, p, labels=labels)
    lr = tk.ids_to_labeled_rows(s_ids, s_lab, s_offs, 512, bos=BOS, eos=EOS)
    assert np.array_equal(lr.rows.ids, rt.rows_numpy(n[0], n[2], 512, rt.CONCAT, BOS, EOS, EOS)[0])
    assert np.array_equal(lr.labels, lt.label_rows("concat", n[1], n[2], 512, bos=True, eos=True, bos_value=-100, eos_value=EOS, pad_value=-100))
    with pytest.raises(tiktoken.TokenDaggerError):
        tk.select_docs(ids, toffs, [len(toffs) - 1])
    with pytest.raises(tiktoken.TokenDaggerError):
        tk.select_docs(ids, toffs, p, min_len=5, max_len=4)
