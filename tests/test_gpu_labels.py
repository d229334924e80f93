"""Loss labels on the GPU (td_span_labels, td_span_labels_device, td_encode_batch_span_labels, the Python methods) against the
truths of tests/labels_truth.py.  All comparisons are exact.  No case here makes the device fault: every error is one the
library reports by a status code."""
import numpy as np
import pytest

import helpers as H
import labels_truth as lt

pytestmark = pytest.mark.gpu

TILE = 4096  # td::LAB_TILE
OPENER = "<|header_start|>assistant<|header_end|>"
CLOSERS = ["<|eot|>", "<|eom|>"]


@pytest.fixture(scope="module")
def tok():
    from tokendagger_amd import capi
    pat, mr, special = H.llama4()
    return capi.HipTokenizer(pat, mr, special, device=0)


@pytest.fixture(scope="module")
def wtok():
    from tokendagger_amd import wrapper
    return wrapper.llama4_scout(0)


def _spec(open, close, ignore=-100, tc=True):
    from tokendagger_amd import capi
    return capi.labels_spec(open, close, ignore, tc)


def _same(got, want, what=""):
    for k, (p, q) in enumerate(zip(got, want)):
        assert p.dtype == q.dtype and p.shape == q.shape and np.array_equal(p, q), (what, k)


def _check(tok, ids, offs, open, close, ignore=-100, tc=True, truth=lt.labels_walk, t=None, combos=((True, True),)):
    t = t if t is not None else truth(ids, offs, open, close, ignore, tc)
    for mask, toff in combos:
        g = tok.span_labels(ids, offs, _spec(open, close, ignore, tc), mask=mask, trained_offsets=toff)
        assert np.array_equal(g[3], t[3]), (g[3], t[3])
        assert g[0].dtype == np.int32 and np.array_equal(g[0], t[0])
        assert (g[1] is None) == (not mask) and (g[2] is None) == (not toff)
        if mask:
            assert g[1].dtype == np.uint8 and np.array_equal(g[1], t[1])
        if toff:
            assert g[2].dtype == np.int64 and np.array_equal(g[2], t[2])
    return t


def test_golden_ids_every_output_combination(tok, golden):
    ids, offs = golden["enc"].astype(np.int32), golden["enc_offsets"].astype(np.int64)
    f = np.argsort(-np.bincount(ids))[:8].tolist()   # the most frequent ids
    pairs = ids[:-1].astype(np.int64) << 32 | ids[1:]
    keep = ~np.isin(ids[:-1], [f[0], f[3]]) & ~np.isin(ids[1:], [f[0], f[3]])
    u, c = np.unique(pairs[keep], return_counts=True)
    big = int(u[np.argmax(c)])
    open, close = [[f[1]], [big >> 32, big & 0xFFFFFFFF], [f[2], f[4], f[5]]], [f[0], f[3]]
    combos = [(m, o) for m in (False, True) for o in (False, True)]
    for tc in (True, False):
        t = _check(tok, ids, offs, open, close, -100, tc, combos=combos)
        _same(t, lt.labels_numpy(ids, offs, open, close, -100, tc))
        assert t[3][0] > 1000 and t[3][1] > 100
    _check(tok, ids, offs, [[big >> 32, big & 0xFFFFFFFF]], [], 7, True, truth=lt.labels_numpy)


def test_random_small_cases(tok):
    rng = np.random.default_rng(21)
    for it in range(200):
        ids, offs, open, close, tc = lt.random_case(rng, max_docs=12 if it % 8 else 300)
        _check(tok, ids, offs, open, close, int(rng.integers(-5, 3)), tc)


def test_tile_edges(tok):
    n = 3 * TILE + 100
    open, close = [[1, 2, 4], [5]], [9, 8]
    for off in range(-9, 10):  # the opener's last id at every alignment around the first tile border: before, astride, behind
        ids = np.full(n, 3, dtype=np.int32)
        q = TILE + off
        ids[q - 2:q + 1] = [1, 2, 4]
        ids[2 * TILE - 1] = 9            # a closer as the last id of a tile
        ids[2 * TILE + 7] = 5            # the one-id opener
        ids[3 * TILE - 1] = 4            # the last id of an opener alone at a tile's end
        for offs in ([0, n], [0, TILE + 1, n], [0, q - 1, n], [0, q, n], [0, q + 1, 2 * TILE + 1, 2 * TILE + 1, n]):
            _check(tok, ids, np.asarray(offs, dtype=np.int64), open, close)
    ids = np.full(n, 3, dtype=np.int32)  # the opener of 8 ids astride the border, the document start one id behind the border
    ids[TILE - 3:TILE + 5] = [1, 2, 3, 4, 5, 6, 7, 1]
    for offs in ([0, n], [0, TILE + 1, n], [0, TILE - 3, n], [0, TILE - 2, n]):
        _check(tok, ids, np.asarray(offs, dtype=np.int64), [[1, 2, 3, 4, 5, 6, 7, 1]], [9], tc=False)


def test_one_giant_document(tok):
    n = 6_000_000 + 13  # ~1465 tiles in one document
    offs = np.asarray([0, n], dtype=np.int64)
    rng = np.random.default_rng(3)
    base = rng.integers(100, 200000, n).astype(np.int32)
    open, close = [[7, 8, 9]], [5]
    variants = {}
    variants["no event"] = base.copy()
    v = base.copy(); v[3:6] = [7, 8, 9]; variants["one opener near the start"] = v
    v = base.copy(); v[n - 4] = 5; variants["one closer near the end"] = v
    v = base.copy(); v[10:13] = [7, 8, 9]; v[2000] = 5; v[3000:3003] = [7, 8, 9]; variants["events in the first tile only"] = v
    want_trained = {"no event": 0, "one opener near the start": n - 6, "one closer near the end": 0,
                    "events in the first tile only": (2000 - 12) + (n - 3003)}
    for name, ids in variants.items():
        t = _check(tok, ids, offs, open, close, truth=lt.labels_numpy, combos=((True, True), (False, False)))
        assert int(t[3][0]) == want_trained[name], name


def test_empty_documents_by_the_hundred_thousand(tok):
    rng = np.random.default_rng(8)
    real = [rng.integers(0, 6, k).astype(np.int32) for k in (50, 1, 5000, 9000)]
    lens = [0] * 30000 + [50] + [0] * 40000 + [1, 5000] + [0] * 30000 + [9000] + [0] * 5
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate(real)
    t = _check(tok, ids, offs, [[1, 2], [3]], [0], truth=lt.labels_numpy)
    _same(t, lt.labels_walk(ids, offs, [[1, 2], [3]], [0]))
    assert len(t[2]) == len(offs) == 100010 and t[3][0] > 100


def test_chat_text_to_labels(tok, wtok):
    import td_corpus
    text, doffs = td_corpus.chat(8 << 20, seed=5)
    r = wtok.encode_batch_to_labels(text, doffs, open=[OPENER], close=CLOSERS, mask=True, trained_offsets=True)
    specials = sorted(wtok._special_tokens)
    e_ids, e_offs = tok.encode_batch_with_special_strs(text, doffs, specials)
    assert np.array_equal(r.ids, e_ids) and np.array_equal(r.tok_offsets, e_offs)
    opener = tok.encode_with_special_strs(OPENER.encode(), specials)[0].tolist()
    closers = [wtok.encode_single_token(c) for c in CLOSERS]
    assert len(opener) == 3
    t = lt.labels_walk(e_ids, e_offs, [opener], closers)
    print("chat 8 MiB: ids", len(e_ids), "docs", len(e_offs) - 1, "counts", t[3].tolist())
    assert t[3][1] >= 1000
    _same((r.labels, r.mask, r.trained_offsets, r.counts), t)
    # no id of an opener that starts a span is trained
    hits = np.flatnonzero((e_ids[2:] == opener[2]) & (e_ids[1:-1] == opener[1]) & (e_ids[:-2] == opener[0])) + 2
    starts = hits[t[1][hits] == 0]  # (an opener while already inside is content)
    assert len(starts) >= t[3][1]
    for j in range(3):
        assert (r.labels[starts - j] == -100).all()
    # the ids form gives the same, and the labels-only form too
    r2 = wtok.ids_to_labels(e_ids, e_offs, open=[opener], close=CLOSERS)
    assert np.array_equal(r2.labels, t[0]) and r2.mask is None and r2.trained_offsets is None and np.array_equal(r2.counts, t[3])
    with pytest.raises(ValueError, match="at most 8"):
        wtok.ids_to_labels(e_ids[:10], [0, 10], open=["one two three four five six seven eight nine ten"], close=CLOSERS)


def _device_alloc(n, n_docs, dev, fill=77):
    import torch
    return (torch.full((max(n, 1),), fill, dtype=torch.int32, device=dev), torch.full((max(n, 1),), fill, dtype=torch.uint8, device=dev),
            torch.full((n_docs + 1,), fill, dtype=torch.int64, device=dev), torch.full((4,), fill, dtype=torch.int64, device=dev))


def _device_call(tok, d_ids, n, d_offs, n_docs, spec, stream, fill=77, mask=True, toff=True, bufs=None):
    lab, m, to, counts = bufs if bufs is not None else _device_alloc(n, n_docs, d_offs.device, fill)
    tok.span_labels_device(d_ids.data_ptr(), n, d_offs.data_ptr(), n_docs, spec, lab.data_ptr(), m.data_ptr() if mask else 0,
                           to.data_ptr() if toff else 0, counts.data_ptr(), stream)
    return lab, m, to, counts


def test_device_form_on_a_side_stream_two_specs_back_to_back(tok, golden):
    import torch
    dev = torch.device("cuda", 0)
    ids, offs = golden["enc"].astype(np.int32), golden["enc_offsets"].astype(np.int64)
    f = np.argsort(-np.bincount(ids))[:6].tolist()
    specs = [([[f[1]]], [f[0]], -100, True), ([[f[2]], [f[3], f[1]]], [f[4]], -1, False)]
    d_ids, d_offs = torch.from_numpy(ids).to(dev), torch.from_numpy(offs).to(dev)
    bufs = [_device_alloc(len(ids), len(offs) - 1, dev) for _ in specs]  # (filled on torch's stream: before it gets busy)
    side = torch.cuda.Stream(device=dev)
    x = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    for _ in range(20):  # torch's default stream is busy meanwhile
        x = x @ x * 1e-3
    outs = [_device_call(tok, d_ids, len(ids), d_offs, len(offs) - 1, _spec(*s), side.cuda_stream, bufs=b) for s, b in zip(specs, bufs)]
    tok.device_status(side.cuda_stream)
    torch.cuda.synchronize()
    for s, o in zip(specs, outs):
        _same([v.cpu().numpy() for v in o], lt.labels_numpy(ids, offs, *s), s)


def test_device_form_with_pointers_off_the_16_byte_grid(tok):
    """d_ids, d_labels and d_mask one element behind an aligned allocation: td_lab_apply's dword loads and stores and its mask
    bytes one by one, instead of int4 / sixteen bytes a lane.  The slots around the outputs keep their fill."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(17)
    n = 3 * TILE + 37
    ids = rng.integers(0, 7, n).astype(np.int32)
    offs = np.asarray([0, 5, 5, TILE + 1, 2 * TILE - 3, n], dtype=np.int64)
    open, close = [[1, 2], [3], [4, 4, 5]], [0, 6]
    stream = torch.cuda.current_stream(dev).cuda_stream
    for shift_ids, shift_lab, shift_mask in ((1, 1, 1), (1, 0, 0), (0, 3, 0), (0, 0, 5), (2, 1, 3)):
        big = torch.full((n + 8,), -7, dtype=torch.int32, device=dev)
        d_ids = big[shift_ids:shift_ids + n]
        d_ids.copy_(torch.from_numpy(ids))
        lab = torch.full((n + 8,), 77, dtype=torch.int32, device=dev)
        m = torch.full((n + 24,), 77, dtype=torch.uint8, device=dev)
        to = torch.full((len(offs),), 77, dtype=torch.int64, device=dev)
        counts = torch.full((4,), 77, dtype=torch.int64, device=dev)
        d_offs = torch.from_numpy(offs).to(dev)
        assert d_ids.data_ptr() % 16 == 4 * shift_ids and lab[shift_lab:].data_ptr() % 16 == 4 * shift_lab
        tok.span_labels_device(d_ids.data_ptr(), n, d_offs.data_ptr(), len(offs) - 1, _spec(open, close, -100, True),
                               lab[shift_lab:].data_ptr(), m[shift_mask:].data_ptr(), to.data_ptr(), counts.data_ptr(), stream)
        assert tok.device_status_pos(stream)[0] == 0
        t = lt.labels_numpy(ids, offs, open, close, -100, True)
        lab, m = lab.cpu().numpy(), m.cpu().numpy()
        _same((lab[shift_lab:shift_lab + n], m[shift_mask:shift_mask + n], to.cpu().numpy(), counts.cpu().numpy()), t, (shift_ids, shift_lab))
        assert (lab[:shift_lab] == 77).all() and (lab[shift_lab + n:] == 77).all()
        assert (m[:shift_mask] == 77).all() and (m[shift_mask + n:] == 77).all()
        assert t[3][0] > 100


@pytest.mark.parametrize("kind", ["decreasing", "negative", "beyond", "nonzero start"])
def test_bad_offsets_raise_through_device_status_and_write_nothing(tok, kind):
    import torch
    from tokendagger_amd import capi
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(4)
    ids = rng.integers(0, 6, 3 * TILE).astype(np.int32)
    offs = np.asarray([0, 100, 5000, 9000, 3 * TILE], dtype=np.int64)
    n = len(ids)
    if kind == "decreasing":
        offs[2] = 50
    elif kind == "negative":
        offs[1] = -3
    elif kind == "beyond":
        n = 3 * TILE - 5
    else:
        offs[0] = 2
    d_ids, d_offs = torch.from_numpy(ids).to(dev), torch.from_numpy(offs).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    outs = _device_call(tok, d_ids, n, d_offs, len(offs) - 1, _spec([[1, 2]], [0]), stream, fill=77)
    code, pos = tok.device_status_pos(stream)
    assert code == capi.TD_E_INVALID and 0 <= pos < len(offs) - 1, (code, pos)
    for o in outs:
        assert (o.cpu().numpy() == 77).all()
    # the handle is fine afterwards
    good = np.asarray([0, 100, 5000, 9000, 3 * TILE], dtype=np.int64)
    _check(tok, ids, good, [[1, 2]], [0])


def test_host_form_rejects_bad_offsets(tok):
    from tokendagger_amd import capi
    ids = np.arange(10, dtype=np.int32)
    for offs, n in (([0, 7, 5, 10], None), ([1, 5, 10], None), ([0, 5, 10], 8)):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            tok.span_labels(ids, np.asarray(offs, dtype=np.int64), _spec([[1]], [2]), n_tokens=n)
        assert e.value.code == capi.TD_E_INVALID


def test_label_rows_align_with_id_rows(tok, golden):
    """rows(labels) with pad = ignore_index and no BOS / EOS: equal to rows(ids) wherever it is not ignore_index, and equal to the
    truth's labels gathered by the same placement (the rows of the stream 0, 1, 2, ... with pad -1 are that placement)."""
    from tokendagger_amd import capi
    ids, offs = golden["enc"].astype(np.int32), golden["enc_offsets"].astype(np.int64)
    f = np.argsort(-np.bincount(ids))[:6].tolist()
    open, close, IGN = [[f[1]], [f[2], f[3]]], [f[0]], -100
    t = lt.labels_numpy(ids, offs, open, close, IGN, True)
    labels = tok.span_labels(ids, offs, _spec(open, close, IGN, True))[0]
    assert np.array_equal(labels, t[0]) and (labels != IGN).sum() > 1000
    index = np.arange(len(ids), dtype=np.int32)
    S = 512
    layouts = {"concat": lambda x, pad: tok.make_rows(x, offs, capi.rows_spec(S, capi.TD_ROWS_CONCAT, -1, -1, pad))[0],
               "bestfit": lambda x, pad: tok.pack_rows(x, offs, capi.pack_spec(S, -1, -1, pad))[0],
               "windows": lambda x, pad: tok.window_rows(x, offs, capi.windows_spec(S, -1, -1, pad), 64)[0]}
    for name, rows in layouts.items():
        r_ids, r_lab, r_idx = rows(ids, IGN), rows(labels, IGN), rows(index, -1)
        assert r_ids.shape == r_lab.shape == r_idx.shape, name
        on = r_lab != IGN
        assert on.sum() >= (labels != IGN).sum() and np.array_equal(r_lab[on], r_ids[on]), name
        want = np.where(r_idx >= 0, t[0][np.maximum(r_idx, 0)], IGN)
        assert np.array_equal(r_lab, want), name
