"""Token counts on the GPU (td_counts.hip) against tests/counts_truth.py: exact comparisons throughout.  The contract is the
section "token counts" of include/tokendagger_hip.h; every error is a status code, no case makes the device fault."""
import numpy as np
import pytest

import counts_truth as ct
import helpers as H

pytestmark = pytest.mark.gpu

TILE = 4096
FILL = -7777  # the guard elements around counts and info in the device form
GUARD = 64


@pytest.fixture(scope="module")
def tok():
    from tokendagger_amd import capi
    pat, mr, special = H.llama4()
    return capi.HipTokenizer(pat, mr, special, device=0)


@pytest.fixture(scope="module")
def golden_truth(golden):
    """Computed once, shared and left unchanged: (ids, offsets, n_bins, counts of one group, groups d % 7, their counts)."""
    ids, offs = golden["enc"].astype(np.int32), golden["enc_offsets"].astype(np.int64)
    n_bins = 201088
    assert len(ids) == 828407 and len(offs) - 1 == 3335 and int(ids.max()) < n_bins
    groups = (np.arange(len(offs) - 1) % 7).astype(np.int32)
    return ids, offs, n_bins, ct.counts_numpy(ids, n_bins), groups, ct.counts_numpy(ids, n_bins, offs, groups, 7)


def _spec(n_bins, n_groups=1, accumulate=False):
    from tokendagger_amd import capi
    return capi.counts_spec(n_bins, n_groups, accumulate=accumulate)


def _same(got, want, what=""):
    assert got[0].dtype == np.int64 and got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), what
    assert np.array_equal(np.asarray(got[1]), want[1]), (what, got[1], want[1])


def _host(tok, ids, n_bins, offs=None, groups=None, n_groups=1, what=""):
    want = ct.counts_numpy(ids, n_bins, offs, groups, n_groups)
    got = tok.token_counts(ids, offs if groups is not None else None, groups, _spec(n_bins, n_groups))
    _same(got, want, what)
    return got


def _device_setup(tok, ids, n_bins, offs=None, groups=None, n_groups=1, preset=None, accumulate=False, shift=0, n_tokens=None):
    """Everything td_token_counts_device needs, uploaded and synchronised: counts and info lie inside larger FILL-filled tensors.
    -> (call(stream): the call alone, nothing else touches the device; result() -> (counts, info, guards untouched)).
    shift: the ids pointer is advanced by that many elements off the 16-byte grid."""
    import torch
    dev = torch.device("cuda", 0)
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    d_buf = torch.from_numpy(np.concatenate([np.full(shift, 12345, dtype=np.int32), ids])).to(dev)
    assert d_buf.data_ptr() % 16 == 0
    d_offs = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).to(dev) if groups is not None else None
    d_grp = torch.from_numpy(np.ascontiguousarray(groups, dtype=np.int32)).to(dev) if groups is not None else None
    size = n_bins * n_groups
    d_counts = torch.full((size + 2 * GUARD,), FILL, dtype=torch.int64, device=dev)
    if preset is not None:
        d_counts[GUARD:GUARD + size] = torch.from_numpy(np.ascontiguousarray(preset, dtype=np.int64).reshape(-1)).to(dev)
    d_info = torch.full((4 + 2 * GUARD,), FILL, dtype=torch.int64, device=dev)
    spec = _spec(n_bins, n_groups, accumulate)
    torch.cuda.synchronize()

    def call(stream):
        rc = tok.token_counts_device(d_buf.data_ptr() + 4 * shift if len(ids) else 0, len(ids) if n_tokens is None else n_tokens,
                                     d_offs.data_ptr() if d_offs is not None else 0, len(offs) - 1 if groups is not None else 0,
                                     d_grp.data_ptr() if d_grp is not None and len(groups) else (d_offs.data_ptr() if d_grp is not None else 0),
                                     spec, d_counts.data_ptr() + 8 * GUARD, d_info.data_ptr() + 8 * GUARD, stream)
        assert rc is None  # (nothing comes back but through device_status)

    def result():
        c, i = d_counts.cpu().numpy(), d_info.cpu().numpy()
        guards = bool((c[:GUARD] == FILL).all() and (c[GUARD + size:] == FILL).all() and (i[:GUARD] == FILL).all() and (i[GUARD + 4:] == FILL).all())
        return c[GUARD:GUARD + size].reshape(n_groups, n_bins), i[GUARD:GUARD + 4], guards
    return call, result


def _device(tok, ids, n_bins, offs=None, groups=None, n_groups=1, **kw):
    """-> (result, stream): the call on torch's current stream."""
    import torch
    call, result = _device_setup(tok, ids, n_bins, offs, groups, n_groups, **kw)
    stream = torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream
    call(stream)
    return result, stream


def _device_ok(tok, ids, n_bins, offs=None, groups=None, n_groups=1, what="", **kw):
    result, stream = _device(tok, ids, n_bins, offs, groups, n_groups, **kw)
    tok.device_status(stream)
    c, i, guards = result()
    assert guards, what
    _same((c, i), ct.counts_numpy(ids, n_bins, offs, groups, n_groups), what)
    return c, i


@pytest.mark.parametrize("seats", [2, 64, 0])
def test_golden_ids(tok, golden_truth, seats):
    from tokendagger_amd import capi
    ids, offs, n_bins, one, groups, seven = golden_truth
    tok.set_option(capi.TD_OPT_COUNTS_SEATS, seats)
    try:
        _same(tok.token_counts(ids, spec=_spec(n_bins)), one, "one group")
        _same(tok.token_counts(ids, offs, groups, _spec(n_bins, 7)), seven, "d % 7")
        result, stream = _device(tok, ids, n_bins, offs, groups, 7)
        tok.device_status(stream)
        c, i, guards = result()
        assert guards
        _same((c, i), seven, "device form")
    finally:
        tok.set_option(capi.TD_OPT_COUNTS_SEATS, 0)
    assert int(one[0].max()) > 0.15 * len(ids)  # the skew the table is there for
    for bad in (1, 3, 48, 8192, -2):
        with pytest.raises(capi.TokenDaggerHipError):
            tok.set_option(capi.TD_OPT_COUNTS_SEATS, bad)


def test_small_cases_against_brute_force(tok):
    from tokendagger_amd import capi
    rng = np.random.default_rng(4)
    raised = hosted = 0
    for it in range(60):
        c = ct.random_case(rng)
        grouped = c["n_groups"] > 1
        offs, groups = (c["tok_offsets"], c["groups"]) if grouped else (None, None)
        want = ct.counts_brute(c["ids"], c["n_bins"], offs, groups, c["n_groups"])
        result, stream = _device(tok, c["ids"], c["n_bins"], offs, groups, c["n_groups"])
        rc, where = tok.device_status_pos(stream)
        got_c, got_i, guards = result()
        assert guards, it
        _same((got_c, got_i), want, it)
        if want[1][3]:  # a document with ids and a bad group: raised with its index, the rest is counted
            raised += 1
            assert rc == capi.TD_E_INVALID and not 0 <= groups[where] < c["n_groups"] and offs[where + 1] > offs[where], it
            assert tok.device_status_pos(stream)[0] == capi.TD_OK  # cleared
        else:
            assert rc == capi.TD_OK, it
        bad_any = grouped and bool(np.any((groups < 0) | (groups >= c["n_groups"])))
        if grouped and offs[0] == 0 and not bad_any:
            hosted += 1
            _same(tok.token_counts(c["ids"], offs, groups, _spec(c["n_bins"], c["n_groups"])), want, it)
        elif not grouped:
            _same(tok.token_counts(c["ids"], spec=_spec(c["n_bins"])), want, it)
    assert raised >= 3 and hosted >= 10


def test_documents_at_tile_borders_and_empty_documents(tok):
    for case in (ct.border_documents(), ct.empty_documents_tile()):
        ids, offs, groups, n_bins, n_groups = case
        _host(tok, ids, n_bins, offs, groups, n_groups)
        _device_ok(tok, ids, n_bins, offs, groups, n_groups)


def test_one_document_over_several_tiles_between_other_groups(tok):
    lens = [100, 5 * TILE + 17, 0, 30]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.random.default_rng(5).integers(0, 1000, size=int(offs[-1])).astype(np.int32)
    groups = np.asarray([2, 0, 1, 1], dtype=np.int32)
    c, _ = _host(tok, ids, 1000, offs, groups, 3)
    assert c[0].sum() == lens[1] and c[2].sum() == 100 and c[1].sum() == 30
    # tok_offsets[0] > 0 and ids behind the last document: only the device form takes them
    _device_ok(tok, ids, 1000, offs[1:], groups[1:], 3)
    _device_ok(tok, ids, 1000, offs[:-1], groups[:-1], 3)


def test_shaped_streams(tok):
    n_bins = 50000
    c, i = _host(tok, np.full(64 * TILE, 4321, dtype=np.int32), n_bins, what="64 * 4096 copies of one id")
    assert c[0, 4321] == 64 * TILE and i.tolist() == [64 * TILE, 0, 0, 0]
    c, _ = _host(tok, np.random.default_rng(6).permutation(n_bins).astype(np.int32), n_bins, what="a permutation")
    assert (c == 1).all()
    cold_hot = np.concatenate([np.arange(1000, 1000 + TILE), np.full(9 * TILE + 5, 5)]).astype(np.int32)
    _host(tok, cold_hot, n_bins, what="cold ids first, then a hot one")
    from tokendagger_amd import capi
    tok.set_option(capi.TD_OPT_COUNTS_SEATS, 2)
    try:
        _host(tok, cold_hot, n_bins, what="cold ids first, then a hot one, two seats")
    finally:
        tok.set_option(capi.TD_OPT_COUNTS_SEATS, 0)


def test_interval_flush(tok, golden_truth):
    """The flush behind every flush_tiles tiles of a workgroup (production: 64, which a call reaches above 268 M ids): with the
    interval at 1, 2 and 3 every workgroup of the golden ids (8 tiles each) flushes and clears its table several times on its way."""
    from tokendagger_amd import capi
    ids, offs, n_bins, one, groups, seven = golden_truth
    try:
        for tiles, seats in ((1, 0), (2, 64), (3, 2)):
            tok.set_option(capi.TD_OPT_COUNTS_FLUSH_TILES, tiles)
            tok.set_option(capi.TD_OPT_COUNTS_SEATS, seats)
            _same(tok.token_counts(ids, spec=_spec(n_bins)), one, (tiles, seats))
            _same(tok.token_counts(ids, offs, groups, _spec(n_bins, 7)), seven, (tiles, seats))
        hot = np.concatenate([np.arange(1000, 1000 + TILE), np.full(20 * TILE + 5, 5)]).astype(np.int32)
        tok.set_option(capi.TD_OPT_COUNTS_FLUSH_TILES, 1)
        _host(tok, hot, 50000, what="cold ids first, then a hot one, flushed behind every tile")
    finally:
        tok.set_option(capi.TD_OPT_COUNTS_FLUSH_TILES, 0)
        tok.set_option(capi.TD_OPT_COUNTS_SEATS, 0)
    for bad in (-1, 65, 1 << 20):
        with pytest.raises(capi.TokenDaggerHipError):
            tok.set_option(capi.TD_OPT_COUNTS_FLUSH_TILES, bad)


def test_values_outside_the_bins(tok):
    rng = np.random.default_rng(7)
    ids = rng.integers(0, 300, size=3 * TILE + 11).astype(np.int32)
    lab = np.where(rng.random(len(ids)) < 0.6, -100, ids).astype(np.int32)  # a label-like stream
    c, i = _host(tok, lab, 300)
    assert i[1] == int((lab == -100).sum()) and i[0] + i[1] == len(lab) and i[2] == 0
    n_bins = 1000
    edge = np.asarray([n_bins - 1, n_bins, 2**31 - 1, n_bins - 1, -1, -2**31, 0] * 700, dtype=np.int32)
    c, i = _host(tok, edge, n_bins)
    assert i.tolist() == [2100, 1400, 1400, 0] and c[0, n_bins - 1] == 1400 and c[0, 0] == 700
    c, i = _host(tok, np.asarray([0, 0, 1, -1, 0, 5], dtype=np.int32), 1, what="n_bins = 1")
    assert c.tolist() == [[3]] and i.tolist() == [3, 1, 2, 0]
    c, i = _host(tok, np.zeros(0, dtype=np.int32), 10, what="no ids")
    assert not c.any() and not i.any()
    c, i = _device_ok(tok, np.zeros(0, dtype=np.int32), 10, what="no ids, device form")
    assert not c.any() and not i.any()


def test_sixteen_million_bins(tok):
    n_bins = 1 << 24
    ids = np.random.default_rng(8).integers(0, n_bins, size=50 * TILE + 3).astype(np.int32)
    ids[::9] = n_bins - 1
    c, i = _host(tok, ids, n_bins)
    assert c[0, n_bins - 1] >= len(ids) // 9 and i[0] == len(ids)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_ids_off_the_16_byte_grid(tok, golden_truth, shift):
    ids, offs, n_bins, one, groups, seven = golden_truth
    n = 9 * TILE + 77
    sub_offs = np.concatenate([offs[:int(np.searchsorted(offs, n, side="right"))], [n]]).astype(np.int64)
    g = groups[:len(sub_offs) - 1]
    _device_ok(tok, ids[:n], n_bins, shift=shift)
    _device_ok(tok, ids[:n], n_bins, sub_offs, g, 7, shift=shift)


def test_accumulate(tok, golden_truth):
    ids, offs, n_bins, one, groups, seven = golden_truth
    first = tok.token_counts(ids, offs, groups, _spec(n_bins, 7))
    acc = first[0].copy()
    second = tok.token_counts(ids, offs, groups, _spec(n_bins, 7, accumulate=True), counts=acc.reshape(-1))
    assert np.array_equal(second[0], 2 * seven[0]) and np.array_equal(second[1], seven[1])  # info is never accumulated
    # the device form twice, and onto 2^32 - 5: the sum carries into the upper word
    sub = ids[:3 * TILE]
    want = ct.counts_numpy(sub, n_bins)
    preset = np.full(n_bins, 2**32 - 5, dtype=np.int64)
    result, stream = _device(tok, sub, n_bins, preset=preset, accumulate=True)
    tok.device_status(stream)
    c, i, guards = result()
    assert guards and np.array_equal(c, want[0] + (2**32 - 5)) and np.array_equal(i, want[1]) and int(c.max()) > 2**32
    result, stream = _device(tok, sub, n_bins, preset=c, accumulate=True)
    tok.device_status(stream)
    c2, i2, guards = result()
    assert guards and np.array_equal(c2, 2 * want[0] + (2**32 - 5)) and np.array_equal(i2, want[1])


def test_device_form_errors_are_status_codes(tok):
    import torch
    from tokendagger_amd import capi
    dev = torch.device("cuda", 0)
    ids, offs, groups, n_bins, n_groups = ct.border_documents()
    want_ok = ct.counts_numpy(ids, n_bins, offs, groups, n_groups)
    bad = groups.copy()
    bad[3], bad[5] = n_groups, -1  # the 9000-id document and a ten-id one
    want = ct.counts_numpy(ids, n_bins, offs, bad, n_groups)
    # host forms: before any launch, counts untouched
    for call in (lambda: tok.token_counts(ids, offs, bad, _spec(n_bins, n_groups)),
                 lambda: tok.token_counts(ids, offs, bad, _spec(n_bins, n_groups, accumulate=True), counts=np.full(n_bins * n_groups, 3, dtype=np.int64))):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            call()
        assert e.value.code == capi.TD_E_INVALID and "doc_group[3]" in str(e.value)
    # device form: nothing synchronises.  Buffers first; then long work on the side stream in front of the call (and on torch's own
    # stream beside it); when the call has returned, the work in front of it has not finished, so the call waited for nothing on
    # its stream and read nothing back
    call, result = _device_setup(tok, ids, n_bins, offs, bad, n_groups)
    side = torch.cuda.Stream(device=dev)
    x = torch.randn(4096, 4096, device=dev)
    y = x @ x  # (the first product loads its library: before anything is timed against it)
    torch.cuda.synchronize()
    for _ in range(10):
        y = y @ x * 1e-3
    with torch.cuda.stream(side):
        z = x
        for _ in range(40):
            z = z @ x * 1e-3
        front = torch.cuda.Event()
        front.record(side)
    stream = side.cuda_stream
    call(stream)
    behind = torch.cuda.Event()
    behind.record(side)
    assert not front.query() and not behind.query() and not side.query(), "td_token_counts_device waited for its stream"
    rc, where = tok.device_status_pos(stream)  # (this one synchronises)
    assert behind.query()
    torch.cuda.synchronize()
    c, i, guards = result()
    assert rc == capi.TD_E_INVALID and where in (3, 5) and guards
    assert i[3] == 9000 + 10 and np.array_equal(i, want[1]) and np.array_equal(c, want[0])
    assert tok.device_status_pos(stream)[0] == capi.TD_OK  # cleared; and the next good call on the same handle
    c, i = _device_ok(tok, ids, n_bins, offs, groups, n_groups)
    assert np.array_equal(c, want_ok[0])
    # offsets that decrease, and offsets that end above n_tokens: a status, nothing outside counts / info written
    down = offs.copy()
    down[4] = down[3] - 50
    for o, n_tok in ((down, None), (offs, int(offs[-1]) - 5000)):
        result, stream = _device(tok, ids, n_bins, o, groups, n_groups, n_tokens=n_tok)
        rc, where = tok.device_status_pos(stream)
        c, i, guards = result()
        assert rc == capi.TD_E_INVALID and guards and 0 <= int(i.sum()) <= len(ids) and int(c.sum()) == int(i[0])
    _device_ok(tok, ids, n_bins, offs, groups, n_groups)
    # a bad spec: before any launch
    for spec in (_spec(0), _spec(8, 0), _spec(1 << 27, 4), capi.CountsSpec(8, 1, 2), _spec(8, 2)):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            tok.token_counts(ids, spec=spec)
        assert e.value.code == capi.TD_E_INVALID


def test_fused_equals_encode_then_count(tok, golden, golden_truth):
    ids, offs, n_bins, one, groups, seven = golden_truth
    text, doc_offs = golden["text"], golden["offsets"]
    c, i, total = tok.encode_batch_token_counts(text, doc_offs, None, _spec(n_bins))
    assert total == len(ids)
    _same((c, i), one)
    c, i, total = tok.encode_batch_token_counts(text, doc_offs, groups, _spec(n_bins, 7))
    assert total == len(ids)
    _same((c, i), seven)
    acc = c.copy().reshape(-1)
    c2, _, _ = tok.encode_batch_token_counts(text, doc_offs, groups, _spec(n_bins, 7, accumulate=True), counts=acc)
    assert np.array_equal(c2, 2 * seven[0])
    e = tok.encode_batch_token_counts(b"", np.zeros(4, np.int64), np.asarray([1, 0, 1], dtype=np.int32), _spec(5, 2))
    assert not e[0].any() and not e[1].any() and e[2] == 0


def test_tokenizer_methods(golden, golden_truth):
    import tokendagger as tiktoken
    ids, offs, n_bins, one, groups, seven = golden_truth
    pat, mr, special = H.llama4()
    tk = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    nv = tk.n_vocab
    want = ct.counts_numpy(ids, nv)
    r = tk.ids_to_counts(ids)
    assert r.counts.shape == (nv,) and np.array_equal(r.counts, want[0][0]) and (r.counted, r.negative, r.too_large) == (len(ids), 0, 0)
    r = tk.ids_to_counts(ids, offs, groups=groups)
    assert r.counts.shape == (7, nv) and np.array_equal(r.counts[:, :n_bins], seven[0]) and not r.counts[:, n_bins:].any()
    r = tk.ids_to_counts(ids, offs, groups=groups, n_groups=9, n_bins=n_bins)
    assert r.counts.shape == (9, n_bins) and np.array_equal(r.counts[:7], seven[0]) and not r.counts[7:].any()
    out = seven[0].copy()
    r = tk.ids_to_counts(ids, offs, groups=groups, n_bins=n_bins, out=out)
    assert r.counts is out and np.array_equal(out, 2 * seven[0])
    # strict: ids above n_bins are not this vocabulary's
    with pytest.raises(tiktoken.TokenDaggerError):
        tk.ids_to_counts(ids, n_bins=1000)
    acc = np.full(1000, 11, dtype=np.int64)
    with pytest.raises(tiktoken.TokenDaggerError):
        tk.ids_to_counts(ids, n_bins=1000, out=acc)
    assert (acc == 11).all()  # a strict call that raises leaves out= as it was
    r = tk.ids_to_counts(ids, n_bins=1000, out=acc, strict=False)
    assert r.counts is acc and np.array_equal(acc, want[0][0][:1000] + 11)
    r = tk.ids_to_counts(ids, n_bins=1000, strict=False)
    assert r.too_large == int((ids >= 1000).sum()) and np.array_equal(r.counts, want[0][0][:1000])
    with pytest.raises(tiktoken.TokenDaggerError):
        tk.ids_to_counts(ids, offs, groups=groups, n_groups=5)
    # the trained-token histogram from a label stream
    lab = np.where(np.arange(len(ids)) % 3 == 0, ids, -100).astype(np.int32)
    r = tk.ids_to_counts(lab)
    assert r.negative == int((lab < 0).sum()) and np.array_equal(r.counts, ct.counts_numpy(lab, nv)[0][0])
    e = tk.encode_batch_to_counts(golden["text"], golden["offsets"], groups=groups, n_bins=n_bins)
    assert e.n_tokens == len(ids) and np.array_equal(e.counts, seven[0]) and e.counted == len(ids)
    e = tk.encode_batch_to_counts(golden["text"], golden["offsets"])
    assert e.counts.shape == (nv,) and np.array_equal(e.counts, want[0][0])
