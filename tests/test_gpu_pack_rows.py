"""Best-fit-decreasing rows on the GPU (td_pack_rows, td_pack_rows_device, td_encode_batch_pack_rows, the Python methods) against
the truth of tests/pack_truth.py."""
import time

import numpy as np
import pytest

import helpers as H
import pack_truth as pt
import td_corpus

pytestmark = pytest.mark.gpu

BOS, EOS = 200000, 200001  # Llama-4 <|begin_of_text|>, <|end_of_text|>
FRAMES = [(-1, -1), (BOS, -1), (-1, EOS), (BOS, EOS)]
PAD = -5


@pytest.fixture(scope="module")
def tok():
    from tokendagger_amd import capi
    pat, mr, special = H.llama4()
    return capi.HipTokenizer(pat, mr, special, device=0)


def _spec(S, bos, eos, pad=PAD, truncate=False):
    from tokendagger_amd import capi
    return capi.pack_spec(S, bos, eos, pad, truncate)


def _check(tok, ids, offs, S, bos, eos, truncate=False, truth=pt.pack_runs, positions=True):
    t = truth(ids, offs, S, bos, eos, PAD, truncate)
    g = tok.pack_rows(ids, offs, _spec(S, bos, eos, PAD, truncate), positions=positions, lengths=True, docs=True)
    assert np.array_equal(g[5], t[5]), (g[5], t[5])
    assert g[0].shape == t[0].shape and np.array_equal(g[0], t[0])
    if positions:
        assert np.array_equal(g[1], t[1])
    else:
        assert g[1] is None
    for k in (2, 3, 4):
        assert np.array_equal(g[k], t[k]), k
    return g


@pytest.mark.parametrize("S", [7, 512, 2048])
def test_golden_all_frames(tok, golden, S):
    ids, offs = golden["enc"], golden["enc_offsets"]
    for bos, eos in FRAMES:
        for trunc in (False, True):
            if trunc and S < (bos >= 0) + (eos >= 0):
                continue
            _check(tok, ids, offs, S, bos, eos, trunc, positions=S >= 512)


def test_small_cases_against_brute_force(tok):
    rng = np.random.default_rng(5)
    for _ in range(60):
        S = int(rng.integers(1, 20))
        special = [0, 1, max(S - 1, 0), S, S + 1, 2 * S]
        lengths = np.where(rng.random(int(rng.integers(0, 30))) < 0.4, rng.choice(special, 1)[0], rng.integers(0, 3 * S + 2, 1)[0])
        lengths = np.where(rng.random(len(lengths)) < 0.5, lengths, rng.integers(0, 3 * S + 2, len(lengths)))
        offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        ids = rng.integers(0, 200000, int(offs[-1])).astype(np.int32)
        bos, eos = FRAMES[int(rng.integers(0, 4))]
        trunc = bool(rng.integers(0, 2)) and S >= (bos >= 0) + (eos >= 0)
        _check(tok, ids, offs, S, bos, eos, trunc, truth=pt.pack_brute)


def test_edges(tok):
    z = np.zeros(0, np.int32)
    g = tok.pack_rows(z, np.zeros(1, np.int64), _spec(8, BOS, EOS), docs=True, lengths=True)  # no documents
    assert g[0].shape == (0, 8) and g[2].tolist() == [0] and g[3].tolist() == [] and g[5].tolist() == [0, 0, 0, 0]
    g = tok.pack_rows(z, np.zeros(4, np.int64), _spec(4, -1, -1))  # empty documents without BOS / EOS: nothing
    assert g[0].shape == (0, 4) and g[2].tolist() == [0] and g[5].tolist() == [0, 0, 0, 0]
    _check(tok, z, np.zeros(5001, np.int64), 3, BOS, EOS, truth=pt.pack_runs)  # only empty documents, framed
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 1000, 1 << 20).astype(np.int32)
    offs = np.array([0, 3, 3, len(ids) - 5, len(ids)], np.int64)  # one giant document between small ones, unaligned
    for trunc in (False, True):
        _check(tok, ids, offs, 8192, BOS, EOS, trunc)
        _check(tok, ids, offs, 1000, -1, EOS, trunc)
    lengths = np.where(rng.random(20000) < 0.9, 0, rng.integers(1, 9, 20000))
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ids = rng.integers(0, 1000, int(offs[-1])).astype(np.int32)
    for S in (1, 5, 64):
        for bos, eos in FRAMES:
            _check(tok, ids, offs, S, bos, eos)
    # S large: more distinct lengths than one read-back carries (PACK_RUNS_FIRST)
    lengths = rng.permutation(np.arange(1, 12001))
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ids = rng.integers(0, 1000, int(offs[-1])).astype(np.int32)
    _check(tok, ids, offs, 20000, -1, -1, positions=False)


def test_device_form_on_torch_equals_host(tok, golden):
    import torch
    from tokendagger_amd import capi
    text, doffs = golden["text"], golden["offsets"]
    dev = torch.device("cuda", 0)
    d_text = torch.from_numpy(np.frombuffer(bytes(text), np.uint8).copy()).to(dev)
    d_doffs = torch.from_numpy(np.asarray(doffs, np.int64).copy()).to(dev)
    n_docs = len(doffs) - 1
    cap_ids = len(d_text)
    d_ids = torch.empty(cap_ids, dtype=torch.int32, device=dev)
    d_toffs = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ids, offs = golden["enc"], golden["enc_offsets"]
    for S, trunc in ((2048, False), (512, True), (7, False)):
        sp = _spec(S, BOS, EOS, PAD, trunc)
        # encode on the device and pack right behind it on the same stream: td_pack_rows_device waits for the encode itself
        tok.encode_device(d_text.data_ptr(), len(d_text), d_doffs.data_ptr(), n_docs, d_ids.data_ptr(), cap_ids, d_toffs.data_ptr(),
                          stream=stream)
        need = int(capi.pack_plan(offs, sp)[0])
        cap = need + 3
        out = torch.full((cap * S,), 77, dtype=torch.int32, device=dev)
        pos = torch.full((cap * S,), 77, dtype=torch.int32, device=dev)
        cu = torch.full((n_docs + 2 * cap + 1,), 77, dtype=torch.int32, device=dev)
        lens = torch.full((cap,), 77, dtype=torch.int32, device=dev)
        docs = torch.full((n_docs + 2 * cap,), 77, dtype=torch.int64, device=dev)
        c = tok.pack_rows_device(d_ids.data_ptr(), cap_ids, d_toffs.data_ptr(), n_docs, sp, out.data_ptr(), cap, pos.data_ptr(),
                                 cu.data_ptr(), lens.data_ptr(), docs.data_ptr(), stream)
        tok.device_status(stream)
        torch.cuda.synchronize()
        h = tok.pack_rows(ids, offs, sp, positions=True, lengths=True, docs=True)
        assert np.array_equal(c, h[5])
        r, ns = int(c[0]), int(c[2])
        assert r == need
        assert np.array_equal(out[:r * S].cpu().numpy().reshape(r, S), h[0])
        assert np.array_equal(pos[:r * S].cpu().numpy().reshape(r, S), h[1])
        assert np.array_equal(cu[:ns + 1].cpu().numpy(), h[2])
        assert np.array_equal(lens[:r].cpu().numpy(), h[3])
        assert np.array_equal(docs[:ns].cpu().numpy(), h[4])
        assert (out[r * S:] == 77).all().item() and (pos[r * S:] == 77).all().item() and (cu[ns + 1:] == 77).all().item()
        assert (lens[r:] == 77).all().item() and (docs[ns:] == 77).all().item()
    # only ids: every other output NULL
    sp = _spec(2048, BOS, EOS)
    r = int(capi.pack_plan(offs, sp)[0])
    out = torch.full((r * 2048,), 77, dtype=torch.int32, device=dev)
    d_ids2 = torch.from_numpy(ids.copy()).to(dev)
    d_offs2 = torch.from_numpy(offs.copy()).to(dev)
    tok.pack_rows_device(d_ids2.data_ptr(), len(ids), d_offs2.data_ptr(), n_docs, sp, out.data_ptr(), r, stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(r, 2048), tok.pack_rows(ids, offs, sp)[0])


def test_encode_batch_pack_rows_equals_encode_then_pack(tok, golden):
    from tokendagger_amd import capi
    text, offs = golden["text"], golden["offsets"]
    for mode in (capi.TD_MODE_ENCODE, capi.TD_MODE_ORDINARY):
        ids, toffs = tok.encode_batch(text, offs, mode=mode)
        for S, trunc in ((2048, False), (100, True)):
            sp = _spec(S, BOS, EOS, 0, trunc)
            a = tok.encode_batch_pack_rows(text, offs, sp, mode=mode, positions=True, lengths=True, docs=True)
            b = tok.pack_rows(ids, toffs, sp, positions=True, lengths=True, docs=True)
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
    e = tok.encode_batch_pack_rows(b"", np.zeros(4, np.int64), _spec(4, BOS, EOS), docs=True)  # three empty documents
    assert e[0].tolist() == [[BOS, EOS, BOS, EOS], [BOS, EOS, PAD, PAD]] and e[2].tolist() == [0, 2, 4, 6, 8]
    assert e[4].tolist() == [0, 1, 2, -1]


def test_capacity_host_and_device(tok, golden):
    import torch
    from tokendagger_amd import capi
    ids, offs = golden["enc"], golden["enc_offsets"]
    n_docs = len(offs) - 1
    sp = _spec(128, BOS, EOS)
    need = int(capi.pack_plan(offs, sp)[0])
    with pytest.raises(capi.TokenDaggerHipError) as ei:
        tok.pack_rows(ids, offs, sp, rows_capacity=need - 1)
    assert ei.value.code == capi.TD_E_CAPACITY
    dev = torch.device("cuda", 0)
    d_ids = torch.from_numpy(ids.copy()).to(dev)
    d_offs = torch.from_numpy(offs.copy()).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    cap, guard = need - 1, 4096
    out = torch.full((cap * 128 + guard,), 55, dtype=torch.int32, device=dev)
    pos = torch.full((cap * 128 + guard,), 55, dtype=torch.int32, device=dev)
    cu = torch.full((n_docs + 2 * cap + 1 + guard,), 55, dtype=torch.int32, device=dev)
    lens = torch.full((cap + guard,), 55, dtype=torch.int32, device=dev)
    docs = torch.full((n_docs + 2 * cap + guard,), 55, dtype=torch.int64, device=dev)
    with pytest.raises(capi.TokenDaggerHipError) as ei:
        tok.pack_rows_device(d_ids.data_ptr(), len(ids), d_offs.data_ptr(), n_docs, sp, out.data_ptr(), cap, pos.data_ptr(), cu.data_ptr(),
                             lens.data_ptr(), docs.data_ptr(), stream)
    assert ei.value.code == capi.TD_E_CAPACITY and int(ei.value.counts[0]) == need
    torch.cuda.synchronize()
    for x in (out, pos, cu, lens, docs):
        assert (x == 55).all().item()
    # tok_offsets[n_docs] > n_tokens, and decreasing offsets: errors, nothing written
    with pytest.raises(capi.TokenDaggerHipError) as ei:
        tok.pack_rows_device(d_ids.data_ptr(), len(ids) - 1, d_offs.data_ptr(), n_docs, sp, out.data_ptr(), need + 10, stream=stream)
    assert ei.value.code == capi.TD_E_INVALID
    bad = offs.copy()
    bad[5] = bad[7] + 1
    d_bad = torch.from_numpy(bad).to(dev)
    with pytest.raises(capi.TokenDaggerHipError) as ei:
        tok.pack_rows_device(d_ids.data_ptr(), len(ids), d_bad.data_ptr(), n_docs, sp, out.data_ptr(), need + 10, stream=stream)
    assert ei.value.code == capi.TD_E_INVALID
    torch.cuda.synchronize()
    assert (out == 55).all().item()
    tok.device_status(stream)
    g = tok.pack_rows(ids, offs, sp)  # (the handle works on afterwards)
    assert int(g[5][0]) == need


def test_bad_ids_specs_and_clone(tok, golden):
    from tokendagger_amd import capi
    ids, offs = golden["enc"][:5000], golden["enc_offsets"][:4]
    for bad in (10 ** 7, -2):
        with pytest.raises(capi.TokenDaggerHipError) as ei:
            tok.pack_rows(ids, offs, _spec(64, bad, EOS))
        assert ei.value.code == capi.TD_E_BAD_TOKEN
    with pytest.raises(capi.TokenDaggerHipError) as ei:
        tok.pack_rows(ids, offs, _spec(1, BOS, EOS, truncate=True))
    assert ei.value.code == capi.TD_E_INVALID
    with pytest.raises(capi.TokenDaggerHipError) as ei:  # cu_seqlens entries are int32
        tok.pack_rows(ids, offs, _spec(1 << 20, BOS, EOS), rows_capacity=1 << 12)
    assert ei.value.code == capi.TD_E_INVALID
    with pytest.raises(capi.TokenDaggerHipError) as ei:  # the existing entry points keep rejecting the layout
        tok.make_rows(ids, offs, _spec(64, BOS, EOS))
    assert ei.value.code == capi.TD_E_INVALID
    ids, offs = golden["enc"], golden["enc_offsets"]
    a = tok.pack_rows(ids, offs, _spec(333, BOS, EOS), positions=True, lengths=True, docs=True)
    b = tok.pack_rows(ids, offs, _spec(333, BOS, EOS), positions=True, lengths=True, docs=True)
    c = tok.clone()
    try:
        cc = c.pack_rows(ids, offs, _spec(333, BOS, EOS), positions=True, lengths=True, docs=True)
    finally:
        c.close()
    for x, y, z in zip(a, b, cc):
        assert np.array_equal(x, y) and np.array_equal(x, z)


def test_tokenizer_methods(golden):
    import tokendagger as tiktoken
    pat, mr, special = H.llama4()
    tk = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    text, offs = golden["text"], golden["offsets"]
    r = tk.encode_batch_to_packed_rows(text, offs, 512, bos="<|begin_of_text|>", eos="<|end_of_text|>", positions=True, docs=True)
    ids, toffs = tk.encode_batch_to_numpy(text, offs)
    t = pt.pack_runs(ids, toffs, 512, BOS, EOS, EOS)
    assert np.array_equal(r.ids, t[0]) and np.array_equal(r.positions, t[1]) and np.array_equal(r.cu_seqlens, t[2])
    assert np.array_equal(r.lengths, t[3]) and np.array_equal(r.docs, t[4]) and np.array_equal(r.counts, t[5])
    p = tk.ids_to_packed_rows(ids, toffs, 256, bos=BOS, eos=EOS, pad=0, truncate=True)
    t = pt.pack_runs(ids, toffs, 256, BOS, EOS, 0, True)
    assert np.array_equal(p.ids, t[0]) and np.array_equal(p.cu_seqlens, t[2]) and p.positions is None and p.docs is None
    assert np.array_equal(p.lengths, t[3])
    with pytest.raises(ValueError):
        tk.ids_to_packed_rows(ids, toffs, 256, bos=BOS)  # padding needed, no pad and no eos
    one = np.array([0, 4, 8], np.int64)
    d = tk.ids_to_packed_rows(ids[:8], one, 4)  # no padding needed: fine without pad
    assert d.ids.tolist() == [ids[:4].tolist(), ids[4:8].tolist()]


def test_one_gib_english(tok):
    import torch
    from tokendagger_amd import capi
    text, offs = td_corpus.english(1 << 30, seed=0)
    offs = np.asarray(offs, np.int64)
    dev = torch.device("cuda", 0)
    d_text = torch.from_numpy(text).to(dev)
    d_offs = torch.from_numpy(offs).to(dev)
    n_docs = len(offs) - 1
    cap = len(text) // 3
    d_ids = torch.empty(cap, dtype=torch.int32, device=dev)
    d_toffs = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    tok.encode_device(d_text.data_ptr(), len(text), d_offs.data_ptr(), n_docs, d_ids.data_ptr(), cap, d_toffs.data_ptr(), stream=stream)
    tok.device_status(stream)
    del d_text
    toffs = d_toffs.cpu().numpy()
    ids = d_ids[:int(toffs[-1])].cpu().numpy()
    S = 8192
    sp = _spec(S, BOS, EOS, 0)
    rows = int(capi.pack_plan(toffs, sp)[0])
    out = torch.empty(rows * S, dtype=torch.int32, device=dev)
    pos = torch.empty(rows * S, dtype=torch.int32, device=dev)
    cu = torch.empty(n_docs + 2 * rows + 1, dtype=torch.int32, device=dev)
    lens = torch.empty(rows, dtype=torch.int32, device=dev)
    docs = torch.empty(n_docs + 2 * rows, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c = tok.pack_rows_device(d_ids.data_ptr(), cap, d_toffs.data_ptr(), n_docs, sp, out.data_ptr(), rows, pos.data_ptr(), cu.data_ptr(),
                             lens.data_ptr(), docs.data_ptr(), stream)
    tok.device_status(stream)
    torch.cuda.synchronize()
    print(f"\n1 GiB English, S={S}: {n_docs} documents, {len(ids)} ids -> {int(c[0])} rows, fill {c[1] / (c[0] * S):.4%}, "
          f"pack_rows_device {1e3 * (time.perf_counter() - t0):.2f} ms (first call, host wall time)")
    t = pt.pack_runs(ids, toffs, S, BOS, EOS, 0)
    assert np.array_equal(c, t[5])
    assert np.array_equal(out.cpu().numpy().reshape(rows, S), t[0])
    assert np.array_equal(pos.cpu().numpy().reshape(rows, S), t[1])
    assert np.array_equal(cu[:int(c[2]) + 1].cpu().numpy(), t[2])
    assert np.array_equal(lens.cpu().numpy(), t[3])
    assert np.array_equal(docs[:int(c[2])].cpu().numpy(), t[4])
