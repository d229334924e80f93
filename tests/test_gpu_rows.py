"""Training rows on the GPU (td_make_rows, td_make_rows_device, td_encode_batch_rows, the Python methods) against the truth of
tests/rows_truth.py."""
import numpy as np
import pytest

import helpers as H
import rows_truth as rt
import td_corpus

pytestmark = pytest.mark.gpu

BOS, EOS = 200000, 200001  # Llama-4 <|begin_of_text|>, <|end_of_text|>
FRAMES = [(-1, -1), (BOS, -1), (-1, EOS), (BOS, EOS)]


@pytest.fixture(scope="module")
def tok():
    from tokendagger_amd import capi
    pat, mr, special = H.llama4()
    return capi.HipTokenizer(pat, mr, special, device=0)


def _spec(S, layout, bos, eos, pad=-5, drop=False):
    from tokendagger_amd import capi
    return capi.rows_spec(S, layout, bos, eos, pad, drop)


def _check(tok, ids, offs, S, layout, bos, eos, drop=False, truth=rt.rows_brute, outputs=(True, True)):
    t_ids, t_pos, t_aux, t_counts = truth(ids, offs, S, layout, bos, eos, -5, drop)
    g_ids, g_pos, g_aux, g_counts = tok.make_rows(ids, offs, _spec(S, layout, bos, eos, -5, drop), positions=outputs[0], aux=outputs[1])
    assert np.array_equal(g_counts, t_counts), (g_counts, t_counts)
    assert g_ids.shape == t_ids.shape and np.array_equal(g_ids, t_ids)
    if outputs[0]:
        assert np.array_equal(g_pos, t_pos)
    else:
        assert g_pos is None
    if outputs[1]:
        assert np.array_equal(g_aux, t_aux)
    return g_ids


@pytest.mark.parametrize("S", [1, 7, 128, 2048, 8192])
def test_golden_both_layouts(tok, golden, S):
    ids, offs = golden["enc"], golden["enc_offsets"]
    for bos, eos in FRAMES:
        _check(tok, ids, offs, S, rt.CONCAT, bos, eos, truth=rt.rows_numpy)
        _check(tok, ids, offs, S, rt.CONCAT, bos, eos, drop=True, truth=rt.rows_numpy, outputs=(False, True))
        if S >= (bos >= 0) + (eos >= 0):
            _check(tok, ids, offs, S, rt.PAD, bos, eos, truth=rt.rows_numpy, outputs=(S <= 2048, True))
    _check(tok, ids, offs, S, rt.CONCAT, BOS, EOS, truth=rt.rows_numpy, outputs=(False, False))


def test_small_cases_against_brute_force(tok):
    rng = np.random.default_rng(5)
    for _ in range(60):
        lengths = rng.integers(0, 40, rng.integers(0, 30))
        offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        ids = rng.integers(0, 200000, int(offs[-1])).astype(np.int32)
        S = int(rng.integers(1, 20))
        bos, eos = FRAMES[int(rng.integers(0, 4))]
        _check(tok, ids, offs, S, rt.CONCAT, bos, eos, drop=bool(rng.integers(0, 2)))
        if S >= (bos >= 0) + (eos >= 0):
            _check(tok, ids, offs, S, rt.PAD, bos, eos)


def test_device_form_on_torch_equals_host(tok, golden):
    import torch
    from tokendagger_amd import capi
    ids, offs = golden["enc"], golden["enc_offsets"]
    dev = torch.device("cuda", 0)
    d_ids = torch.from_numpy(ids.copy()).to(dev)
    d_offs = torch.from_numpy(offs.copy()).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n_docs = len(offs) - 1
    for layout, S in ((rt.CONCAT, 2048), (rt.PAD, 512), (rt.CONCAT, 7)):
        sp = _spec(S, layout, BOS, EOS)
        cap = capi.rows_capacity_of(sp, len(ids), n_docs) + 3
        out = torch.full((cap * S,), 77, dtype=torch.int32, device=dev)
        pos = torch.full((cap * S,), 77, dtype=torch.int32, device=dev)
        aux = torch.full((n_docs + cap + 1,), 77, dtype=torch.int32, device=dev)
        counts = torch.zeros(4, dtype=torch.int64, device=dev)
        tok.make_rows_device(d_ids.data_ptr(), len(ids), d_offs.data_ptr(), n_docs, sp, out.data_ptr(), cap, pos.data_ptr(),
                             aux.data_ptr(), counts.data_ptr(), stream)
        tok.device_status(stream)
        h_ids, h_pos, h_aux, h_counts = tok.make_rows(ids, offs, sp, positions=True)
        c = counts.cpu().numpy()
        assert np.array_equal(c, h_counts)
        r = int(c[0])
        assert np.array_equal(out[:r * S].cpu().numpy().reshape(r, S), h_ids)
        assert np.array_equal(pos[:r * S].cpu().numpy().reshape(r, S), h_pos)
        assert (out[r * S:] == 77).all().item() and (pos[r * S:] == 77).all().item()
        na = int(c[2]) + 1 if layout == rt.CONCAT else n_docs
        assert np.array_equal(aux[:na].cpu().numpy(), h_aux)
        assert (aux[na:] == 77).all().item()


def test_encode_batch_rows_equals_encode_then_rows(tok, golden):
    text, offs = golden["text"], golden["offsets"]
    ids, toffs = tok.encode_batch(text, offs)
    for layout, S, drop in ((rt.CONCAT, 2048, False), (rt.CONCAT, 100, True), (rt.PAD, 256, False)):
        sp = _spec(S, layout, BOS, EOS, 0, drop)
        a = tok.encode_batch_rows(text, offs, sp, positions=True)
        b = tok.make_rows(ids, toffs, sp, positions=True)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    e = tok.encode_batch_rows(b"", np.zeros(4, np.int64), _spec(4, rt.CONCAT, BOS, EOS))  # three empty documents
    assert e[0].tolist() == [[BOS, EOS, BOS, EOS], [BOS, EOS, -5, -5]] and e[2].tolist() == [0, 2, 4, 6]


def test_one_giant_document(tok):
    n = 64 << 20
    rng = np.random.default_rng(1)
    ids = rng.integers(0, 200000, n // 4).astype(np.int32)  # (a 64 MiB document's worth of ids)
    offs = np.array([0, len(ids)], np.int64)
    for S in (8192, 1000):
        _check(tok, ids, offs, S, rt.CONCAT, BOS, EOS, truth=rt.rows_numpy)
    g_ids, _, lens, counts = tok.make_rows(ids, offs, _spec(4096, rt.PAD, BOS, EOS))
    assert g_ids.shape == (1, 4096) and lens.tolist() == [4096] and counts.tolist() == [1, 4096, 1, 1]
    assert g_ids[0, 0] == BOS and g_ids[0, -1] == EOS and np.array_equal(g_ids[0, 1:-1], ids[:4094])
    # the same document between small ones, unaligned
    offs2 = np.array([0, 3, 3, len(ids) - 5, len(ids)], np.int64)
    _check(tok, ids, offs2, 8192, rt.CONCAT, BOS, -1, truth=rt.rows_numpy)
    _check(tok, ids, offs2, 8192, rt.PAD, -1, EOS, truth=rt.rows_numpy)


def test_empty_documents_and_edges(tok):
    rng = np.random.default_rng(2)
    lengths = np.where(rng.random(20000) < 0.9, 0, rng.integers(1, 9, 20000))
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ids = rng.integers(0, 1000, int(offs[-1])).astype(np.int32)
    for S in (1, 5, 64):
        for bos, eos in FRAMES:
            _check(tok, ids, offs, S, rt.CONCAT, bos, eos, truth=rt.rows_numpy)
    only_empty = np.zeros(50001, np.int64)
    _check(tok, np.zeros(0, np.int32), only_empty, 3, rt.CONCAT, -1, -1)
    _check(tok, np.zeros(0, np.int32), only_empty, 3, rt.CONCAT, BOS, -1, truth=rt.rows_numpy)
    _check(tok, np.zeros(0, np.int32), only_empty, 2, rt.PAD, -1, -1, truth=rt.rows_numpy)
    g = tok.make_rows(np.zeros(0, np.int32), np.zeros(1, np.int64), _spec(8, rt.CONCAT, BOS, EOS))  # n_docs = 0
    assert g[0].shape == (0, 8) and g[2].tolist() == [0] and g[3].tolist() == [0, 0, 0, 0]
    ids5 = np.arange(5, dtype=np.int32)
    g = tok.make_rows(ids5, np.array([0, 5], np.int64), _spec(8, rt.CONCAT, -1, -1, 0, True))  # T < S with DROP_LAST
    assert g[0].shape == (0, 8) and g[2].tolist() == [0] and g[3].tolist() == [0, 0, 0, 0]


def test_concat_at_the_boundary_of_the_lds_table(tok):
    """One tile whose documents fill the LDS table (4352 entries) to its last entry and just beyond: a document, E empty ones
    and a document need E + 3 entries with the sentinel, so E = 4349 is the last that fits and 4350 the first that searches
    global memory."""
    rng = np.random.default_rng(9)
    for E in (4348, 4349, 4350, 4351, 4352, 4353, 5000):
        offs = np.concatenate([[0], np.cumsum([3] + [0] * E + [7])]).astype(np.int64)
        ids = rng.integers(0, 1000, int(offs[-1])).astype(np.int32)
        _check(tok, ids, offs, 8, rt.CONCAT, -1, -1, truth=rt.rows_numpy)


def test_capacity_host_and_device(tok, golden):
    import torch
    from tokendagger_amd import capi
    ids, offs = golden["enc"], golden["enc_offsets"]
    n_docs = len(offs) - 1
    sp = _spec(128, rt.CONCAT, BOS, EOS)
    need = capi.rows_capacity_of(sp, len(ids), n_docs)
    with pytest.raises(capi.TokenDaggerHipError) as ei:
        tok.make_rows(ids, offs, sp, rows_capacity=need - 1)
    assert ei.value.code == capi.TD_E_CAPACITY
    dev = torch.device("cuda", 0)
    d_ids = torch.from_numpy(ids.copy()).to(dev)
    d_offs = torch.from_numpy(offs.copy()).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    cap, guard = need - 1, 4096
    out = torch.full((cap * 128 + guard,), 55, dtype=torch.int32, device=dev)
    pos = torch.full((cap * 128 + guard,), 55, dtype=torch.int32, device=dev)
    aux = torch.full((n_docs + cap + 1 + guard,), 55, dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    tok.make_rows_device(d_ids.data_ptr(), len(ids), d_offs.data_ptr(), n_docs, sp, out.data_ptr(), cap, pos.data_ptr(), aux.data_ptr(),
                         counts.data_ptr(), stream)
    rc, where = tok.device_status_pos(stream)
    assert rc == capi.TD_E_CAPACITY and where == need
    assert counts.cpu().tolist()[0] == need
    assert (out == 55).all().item() and (pos == 55).all().item() and (aux == 55).all().item()
    # tok_offsets[n_docs] > n_tokens: an error on the device too, nothing written
    tok.make_rows_device(d_ids.data_ptr(), len(ids) - 1, d_offs.data_ptr(), n_docs, sp, out.data_ptr(), need + 10, 0, 0, counts.data_ptr(), stream)
    rc, where = tok.device_status_pos(stream)
    assert rc == capi.TD_E_INVALID and where == len(ids)
    assert (out == 55).all().item()
    tok.device_status(stream)  # (cleared)


def test_bad_ids_clone_and_specs(tok, golden):
    from tokendagger_amd import capi
    ids, offs = golden["enc"][:5000], golden["enc_offsets"][:4]
    for bad in (10 ** 7, -2):
        with pytest.raises(capi.TokenDaggerHipError) as ei:
            tok.make_rows(ids, offs, _spec(64, rt.CONCAT, bad, EOS))
        assert ei.value.code == capi.TD_E_BAD_TOKEN
    with pytest.raises(capi.TokenDaggerHipError) as ei:
        tok.make_rows(ids, offs, _spec(1, rt.PAD, BOS, EOS))
    assert ei.value.code == capi.TD_E_INVALID
    with pytest.raises(capi.TokenDaggerHipError) as ei:  # cu_seqlens entries are int32
        tok.make_rows(ids, offs, _spec(1 << 20, rt.CONCAT, BOS, EOS), rows_capacity=1 << 12)
    assert ei.value.code == capi.TD_E_INVALID
    c = tok.clone()
    try:
        for layout in (rt.CONCAT, rt.PAD):
            a = c.make_rows(ids, offs, _spec(33, layout, BOS, EOS), positions=True)
            b = tok.make_rows(ids, offs, _spec(33, layout, BOS, EOS), positions=True)
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
    finally:
        c.close()


def test_tokenizer_methods(golden):
    import tokendagger as tiktoken
    pat, mr, special = H.llama4()
    tk = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    text, offs = golden["text"], golden["offsets"]
    r = tk.encode_batch_to_rows(text, offs, 512, bos="<|begin_of_text|>", eos="<|end_of_text|>", positions=True)
    ids, toffs = tk.encode_batch_to_numpy(text, offs)
    t_ids, t_pos, t_cu, t_counts = rt.rows_numpy(ids, toffs, 512, rt.CONCAT, BOS, EOS, EOS)
    assert np.array_equal(r.ids, t_ids) and np.array_equal(r.positions, t_pos) and np.array_equal(r.cu_seqlens, t_cu)
    assert r.lengths is None and np.array_equal(r.counts, t_counts)
    p = tk.ids_to_rows(ids, toffs, 256, layout="pad", bos=BOS, eos=EOS, pad=0)
    t = rt.rows_numpy(ids, toffs, 256, rt.PAD, BOS, EOS, 0)
    assert np.array_equal(p.ids, t[0]) and np.array_equal(p.lengths, t[2]) and p.cu_seqlens is None and p.positions is None
    with pytest.raises(ValueError):
        tk.ids_to_rows(ids, toffs, 256, layout="pad", bos=BOS)  # padding needed, no pad and no eos
    d = tk.ids_to_rows(ids, toffs, 256, bos=BOS, drop_last=True)  # no padding needed: fine without pad
    assert int(d.counts[1]) == d.ids.size


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
    sp = _spec(8192, rt.CONCAT, BOS, EOS, 0)
    rows = capi.rows_capacity_of(sp, len(ids), n_docs)
    out = torch.empty(rows * 8192, dtype=torch.int32, device=dev)
    pos = torch.empty(rows * 8192, dtype=torch.int32, device=dev)
    cu = torch.empty(n_docs + rows + 1, dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    tok.make_rows_device(d_ids.data_ptr(), cap, d_toffs.data_ptr(), n_docs, sp, out.data_ptr(), rows, pos.data_ptr(), cu.data_ptr(),
                         counts.data_ptr(), stream)
    tok.device_status(stream)
    t_ids, t_pos, t_cu, t_counts = rt.rows_numpy(ids, toffs, 8192, rt.CONCAT, BOS, EOS, 0)
    c = counts.cpu().numpy()
    assert np.array_equal(c, t_counts)
    assert np.array_equal(out.cpu().numpy().reshape(rows, 8192), t_ids)
    assert np.array_equal(pos.cpu().numpy().reshape(rows, 8192), t_pos)
    assert np.array_equal(cu[:int(c[2]) + 1].cpu().numpy(), t_cu)
