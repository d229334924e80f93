"""Overlapping window rows on the GPU (td_window_rows, td_window_rows_device, td_encode_batch_window_rows, the Python methods)
against the truth of tests/windows_truth.py."""
import numpy as np
import pytest

import helpers as H
import windows_truth as wt

pytestmark = pytest.mark.gpu

BOS, EOS = 200000, 200001  # Llama-4 <|begin_of_text|>, <|end_of_text|>
FRAMES = [(-1, -1), (BOS, -1), (-1, EOS), (BOS, EOS)]
PAD = -5
ALL = (True, True, True, True)  # positions, lengths, docs, starts


@pytest.fixture(scope="module")
def tok():
    from tokendagger_amd import capi
    pat, mr, special = H.llama4()
    return capi.HipTokenizer(pat, mr, special, device=0)


def _spec(S, bos, eos, pad=PAD):
    from tokendagger_amd import capi
    return capi.windows_spec(S, bos, eos, pad)


def _check(tok, ids, offs, S, overlap, bos, eos, truth=wt.windows_brute, outputs=ALL, t=None):
    t = t if t is not None else truth(ids, offs, S, overlap, bos, eos, PAD)
    g = tok.window_rows(ids, offs, _spec(S, bos, eos), overlap, positions=outputs[0], lengths=outputs[1], docs=outputs[2], starts=outputs[3])
    assert np.array_equal(g[5], t[5]), (g[5], t[5])
    assert g[0].shape == t[0].shape and np.array_equal(g[0], t[0])
    for k, want in enumerate(outputs):
        if want:
            assert g[1 + k].dtype == t[1 + k].dtype and np.array_equal(g[1 + k], t[1 + k]), k
        else:
            assert g[1 + k] is None
    return t


@pytest.mark.parametrize("S,overlap", [(1, 0), (7, 2), (128, 0), (128, 32), (512, 64), (2048, 128), (8192, 0)])
def test_golden_ids(tok, golden, S, overlap):
    ids, offs = golden["enc"], golden["enc_offsets"]
    ran = 0
    for bos, eos in FRAMES:
        C = S - (bos >= 0) - (eos >= 0)
        if C < 1 or overlap >= C:
            continue
        t = _check(tok, ids, offs, S, overlap, bos, eos, truth=wt.windows_numpy)
        assert t[5][2] >= 7 and t[5][0] > len(offs) - 1  # (documents are split in every case)
        _check(tok, ids, offs, S, overlap, bos, eos, outputs=(False, False, False, False), t=t)
        _check(tok, ids, offs, S, overlap, bos, eos, outputs=(False, True, False, True), t=t)
        _check(tok, ids, offs, S, overlap, bos, eos, outputs=(True, False, True, False), t=t)
        ran += 1
    assert ran >= 1


def test_small_cases_against_brute_force(tok):
    rng = np.random.default_rng(5)
    for it in range(60):
        lengths = rng.integers(0, 41, rng.integers(0, 30))
        offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        ids = rng.integers(0, 200000, int(offs[-1])).astype(np.int32)
        bos, eos = FRAMES[int(rng.integers(0, 4))]
        k = (bos >= 0) + (eos >= 0)
        S = int(rng.integers(1 + k, 21))
        C = S - k
        overlap = C - 1 if it % 5 == 4 else int(rng.integers(0, C))
        _check(tok, ids, offs, S, overlap, bos, eos)


def test_equals_pad_where_it_must(tok, golden):
    from tokendagger_amd import capi
    ids, offs = golden["enc"], golden["enc_offsets"]
    S, C = 128, 126
    L = np.diff(offs)
    keep = np.flatnonzero(L <= C)
    assert len(keep) >= 3000
    k_offs = np.concatenate([[0], np.cumsum(L[keep])]).astype(np.int64)
    k_ids = np.concatenate([ids[offs[d]:offs[d + 1]] for d in keep]).astype(np.int32)
    w = tok.window_rows(k_ids, k_offs, _spec(S, BOS, EOS), 0, positions=True)
    p_ids, p_pos, p_len, p_counts = tok.make_rows(k_ids, k_offs, capi.rows_spec(S, capi.TD_ROWS_PAD, BOS, EOS, PAD), positions=True)
    assert w[0].tobytes() == p_ids.tobytes() and w[1].tobytes() == p_pos.tobytes() and w[2].tobytes() == p_len.tobytes()
    assert w[5][2] == 0 and w[5][3] == 1 and w[5][0] == len(keep) and w[5][1] == p_counts[1]
    assert np.array_equal(w[3], np.arange(len(keep))) and not w[4].any()


def _device_call(tok, ids, offs, S, overlap, bos, eos, cap, fill=77, n_tokens=None):
    import torch
    dev = torch.device("cuda", 0)
    d_ids = torch.from_numpy(np.ascontiguousarray(ids)).to(dev)
    d_offs = torch.from_numpy(np.ascontiguousarray(offs)).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    bufs = [torch.full((max(cap * S, 1),), fill, dtype=torch.int32, device=dev), torch.full((max(cap * S, 1),), fill, dtype=torch.int32, device=dev),
            torch.full((max(cap, 1),), fill, dtype=torch.int32, device=dev), torch.full((max(cap, 1),), fill, dtype=torch.int64, device=dev),
            torch.full((max(cap, 1),), fill, dtype=torch.int64, device=dev)]
    counts = torch.full((4,), fill, dtype=torch.int64, device=dev)
    tok.window_rows_device(d_ids.data_ptr(), len(ids) if n_tokens is None else n_tokens, d_offs.data_ptr(), len(offs) - 1, _spec(S, bos, eos),
                           overlap, bufs[0].data_ptr(), cap, bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), bufs[4].data_ptr(),
                           counts.data_ptr(), stream)
    return bufs, counts, stream


def test_device_form_on_torch_equals_host(tok, golden):
    ids, offs = golden["enc"], golden["enc_offsets"]
    for S, overlap, bos, eos in ((2048, 128, BOS, EOS), (512, 64, -1, EOS), (7, 2, BOS, -1)):
        h = tok.window_rows(ids, offs, _spec(S, bos, eos), overlap, positions=True)
        r = int(h[5][0])
        cap = r + 3
        bufs, counts, stream = _device_call(tok, ids, offs, S, overlap, bos, eos, cap)
        tok.device_status(stream)
        assert np.array_equal(counts.cpu().numpy(), h[5])
        for k, per in enumerate((S, S, 1, 1, 1)):
            got = bufs[k].cpu().numpy()
            assert np.array_equal(got[:r * per], h[k].reshape(-1)), k
            assert (got[r * per:] == 77).all(), k


def test_capacity_host_and_device(tok, golden):
    from tokendagger_amd import capi
    ids, offs = golden["enc"], golden["enc_offsets"]
    S, overlap = 128, 32
    need = int(capi.window_plan(offs, _spec(S, BOS, EOS), overlap)[0])
    with pytest.raises(capi.TokenDaggerHipError) as ei:
        tok.window_rows(ids, offs, _spec(S, BOS, EOS), overlap, rows_capacity=need - 1)
    assert ei.value.code == capi.TD_E_CAPACITY and ei.value.counts[0] == need
    bufs, counts, stream = _device_call(tok, ids, offs, S, overlap, BOS, EOS, need - 1)
    rc, where = tok.device_status_pos(stream)
    assert rc == capi.TD_E_CAPACITY and where == need
    assert counts.cpu().tolist()[0] == need
    for b in bufs:
        assert (b == 77).all().item()
    tok.device_status(stream)  # (cleared)
    _check(tok, ids, offs, S, overlap, BOS, EOS, truth=wt.windows_numpy)


def test_bad_offsets_on_the_device(tok, golden):
    from tokendagger_amd import capi
    ids, offs = golden["enc"][:50000], golden["enc_offsets"]
    offs = offs[:int(np.searchsorted(offs, 50000, side="right"))].copy()
    good = np.concatenate([offs, [50000]]).astype(np.int64)
    S, overlap = 64, 8
    cap = int(capi.window_plan(good, _spec(S, BOS, EOS), overlap)[0]) + 8
    i = 1 + int(np.flatnonzero(np.diff(good[1:]) > 0)[0])
    dec = good.copy()
    dec[i], dec[i + 1] = good[i + 1], good[i]   # decreasing
    neg = good.copy()
    neg[0] = -3                                 # negative
    for bad, n_tokens in ((dec, 50000), (neg, 50000), (good, 49999)):  # ... and the last offset above n_tokens
        bufs, counts, stream = _device_call(tok, ids, bad, S, overlap, BOS, EOS, cap, n_tokens=n_tokens)
        rc, _ = tok.device_status_pos(stream)
        assert rc == capi.TD_E_INVALID
        for b in bufs:
            assert (b == 77).all().item()  # nothing is written on an error
        t = wt.windows_numpy(ids, good, S, overlap, BOS, EOS, PAD)
        bufs, counts, stream = _device_call(tok, ids, good, S, overlap, BOS, EOS, cap)  # the next good call on the same handle
        tok.device_status(stream)
        assert np.array_equal(counts.cpu().numpy(), t[5])
        r = int(t[5][0])
        assert np.array_equal(bufs[0].cpu().numpy()[:r * S].reshape(r, S), t[0])
        assert np.array_equal(bufs[3].cpu().numpy()[:r], t[3]) and np.array_equal(bufs[4].cpu().numpy()[:r], t[4])


def test_one_giant_document(tok):
    rng = np.random.default_rng(1)
    ids = rng.integers(0, 200000, 16 << 20).astype(np.int32)
    t = _check(tok, ids, np.array([0, len(ids)], np.int64), 8192, 512, BOS, EOS, truth=wt.windows_numpy)
    assert t[5][2] == 1 and t[5][3] == t[5][0] == -(-(len(ids) - 512) // (8190 - 512))
    # the same document between small ones, unaligned
    offs2 = np.array([0, 3, 3, len(ids) - 5, len(ids)], np.int64)
    _check(tok, ids, offs2, 8192, 512, BOS, -1, truth=wt.windows_numpy)
    _check(tok, ids, offs2, 8192, 512, -1, -1, truth=wt.windows_numpy, outputs=(False, True, True, True))


def test_wide_and_shallow(tok):
    rng = np.random.default_rng(2)
    lengths = rng.integers(0, 4, 2_000_000)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ids = rng.integers(0, 200000, int(offs[-1])).astype(np.int32)
    _check(tok, ids, offs, 4, 0, -1, -1, truth=wt.windows_numpy)       # nothing is split
    _check(tok, ids, offs, 4, 1, BOS, EOS, truth=wt.windows_numpy)     # C = 2, step 1: the documents of 3 ids have two rows
    _check(tok, ids, offs, 4, 0, BOS, -1, truth=wt.windows_numpy, outputs=(False, False, True, False))


def test_fused_equals_encode_then_windows(tok, golden):
    text, offs = golden["text"], golden["offsets"]
    ids, toffs = tok.encode_batch(text, offs)
    for S, overlap, bos, eos in ((2048, 128, BOS, EOS), (100, 90, -1, -1), (256, 0, BOS, -1)):
        if overlap == 90:  # (a step of 10 ids makes ten slots of every id: a few documents only)
            t, o = text[:int(offs[40])], offs[:41]
            i, to = tok.encode_batch(t, o)
        else:
            t, o, i, to = text, offs, ids, toffs
        a = tok.encode_batch_window_rows(t, o, _spec(S, bos, eos, 0), overlap, positions=True)
        b = tok.window_rows(i, to, _spec(S, bos, eos, 0), overlap, positions=True)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    e = tok.encode_batch_window_rows(b"", np.zeros(4, np.int64), _spec(4, BOS, EOS), 1)  # three empty documents
    assert e[0].tolist() == [[BOS, EOS, PAD, PAD]] * 3 and e[2].tolist() == [2, 2, 2] and e[3].tolist() == [0, 1, 2]
    assert e[4].tolist() == [0, 0, 0] and e[5].tolist() == [3, 6, 0, 1]


def test_span_recipe_end_to_end(tok, golden):
    from tokendagger_amd import capi
    text, offs = golden["text"], golden["offsets"]
    raw = np.asarray(text, np.uint8).tobytes()
    ids, toffs, starts = tok.encode_batch_with_starts(text, offs, unit=capi.TD_UNIT_BYTES)
    S, overlap = 128, 32
    r_ids, _, lens, docs, rstarts, counts = tok.window_rows(ids, toffs, _spec(S, BOS, EOS), overlap)
    assert counts[2] >= 7
    for r in range(len(lens)):
        d, body = int(docs[r]), r_ids[r, 1:lens[r] - 1]
        if len(body) == 0:
            assert toffs[d + 1] == toffs[d]
            continue
        first = int(toffs[d] + rstarts[r])  # the recipe: the row's first body id among the document's ids
        last = first + len(body) - 1
        assert np.array_equal(ids[first:last + 1], body)
        lo = int(offs[d] + starts[first])
        hi = int(offs[d] + starts[last + 1]) if last + 1 < toffs[d + 1] else int(offs[d + 1])
        assert tok.decode_bytes(body) == raw[lo:hi], r


def test_tokenizer_methods(golden):
    import tokendagger as tiktoken
    pat, mr, special = H.llama4()
    tk = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    text, offs = golden["text"], golden["offsets"]
    ids, toffs = tk.encode_batch_to_numpy(text, offs)
    t = wt.windows_numpy(ids, toffs, 512, 64, BOS, EOS, EOS)
    for r in (tk.encode_batch_to_window_rows(text, offs, 512, overlap=64, bos="<|begin_of_text|>", eos="<|end_of_text|>", positions=True),
              tk.ids_to_window_rows(ids, toffs, 512, overlap=64, bos=BOS, eos=EOS, positions=True)):
        assert np.array_equal(r.ids, t[0]) and np.array_equal(r.positions, t[1]) and np.array_equal(r.lengths, t[2])
        assert np.array_equal(r.docs, t[3]) and np.array_equal(r.starts, t[4]) and np.array_equal(r.counts, t[5])
    p = tk.ids_to_window_rows(ids, toffs, 256, bos=BOS, pad=0)
    t = wt.windows_numpy(ids, toffs, 256, 0, BOS, -1, 0)
    assert np.array_equal(p.ids, t[0]) and p.positions is None and np.array_equal(p.lengths, t[2])
    with pytest.raises(ValueError):
        tk.ids_to_window_rows(ids, toffs, 256, overlap=16, bos=BOS)  # padding needed, no pad and no eos
    with pytest.raises(ValueError):
        tk.encode_batch_to_window_rows(text, offs, 256, bos=BOS)
    with pytest.raises(tiktoken.TokenDaggerError):
        tk.ids_to_window_rows(ids, toffs, 16, overlap=14, bos=BOS, eos=EOS)  # overlap >= C
    with pytest.raises(tiktoken.TokenDaggerError):
        tk.encode_batch_to_window_rows(text, offs, 16, overlap=14, bos=BOS, eos=EOS)


def test_other_layouts_reject_windows(tok, golden):
    from tokendagger_amd import capi
    ids, offs = golden["enc"][:5000], golden["enc_offsets"][:4]
    for call in (tok.make_rows, tok.pack_rows):
        with pytest.raises(capi.TokenDaggerHipError) as ei:
            call(ids, offs, _spec(64, BOS, EOS), rows_capacity=1000)
        assert ei.value.code == capi.TD_E_INVALID
    for bad in (10 ** 7, -2):
        with pytest.raises(capi.TokenDaggerHipError) as ei:
            tok.window_rows(ids, offs, _spec(64, bad, EOS), 0, rows_capacity=1000)
        assert ei.value.code == capi.TD_E_BAD_TOKEN
