"""MinHash signatures on the GPU (td_minhash, td_minhash_device, td_encode_batch_minhash, the Python methods) against the truth of
tests/minhash_truth.py.  Signatures, band keys and counts must be EQUAL to it.  No case here makes the device fault: every error is
one the library reports by a status code."""
import functools

import numpy as np
import pytest

import helpers as H
import minhash_truth as mt

pytestmark = pytest.mark.gpu

FILL = 0x77
KS = (1, 2, 5, 13, 64)
# num_perm -> (bands, rows): bands * rows == num_perm and < num_perm, and no keys
PERMS = {1: (1, 1), 63: (9, 7), 64: (0, 0), 65: (13, 5), 128: (32, 3), 1024: (20, 50)}


@pytest.fixture(scope="module")
def tok():
    from tokendagger_amd import capi
    pat, mr, special = H.llama4()
    return capi.HipTokenizer(pat, mr, special, device=0)


@pytest.fixture(scope="module")
def side():
    import torch
    return torch.cuda.Stream(device=torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def edge_truth(k):
    """Computed once per k with every permutation, shared and left unchanged: a signature of fewer permutations is its prefix."""
    ids, offs = mt.edge_case(np.random.default_rng(100 + k), k)
    sig, _, counts = mt.minhash_numpy(ids, offs, k, 1024, 1)
    return ids, offs, sig, counts


def with_keys(sig, counts, num_perm, bands, rows):
    sig = np.ascontiguousarray(sig[:, :num_perm])
    keys = np.asarray([mt.band_keys_of(row, bands, rows) for row in sig], dtype=np.uint64).reshape(len(sig), bands)
    return sig, keys, counts


def check(tok, ids, offs, k=5, num_perm=128, bands=0, rows=0, want=None, n_tokens=None):
    from tokendagger_amd import capi
    want = want if want is not None else mt.minhash_numpy(ids, offs, k, num_perm, 1, bands, rows)
    sig, keys, counts = tok.minhash(ids, offs, capi.minhash_spec(k, num_perm, 1, bands, rows), n_tokens=n_tokens)
    if bands == 0:
        assert keys is None
        keys = np.zeros((len(offs) - 1, 0), dtype=np.uint64)
    mt.same((sig, keys, counts), want, (k, num_perm, bands, rows))
    return want


@pytest.mark.parametrize("num_perm", sorted(PERMS))
@pytest.mark.parametrize("k", KS)
def test_boundaries_on_lane_runs_and_tile_edges(tok, k, num_perm):
    ids, offs, sig, counts = edge_truth(k)
    lens = np.diff(offs)
    assert {0, 1, k, k + 1, 15, 16, 17, 4095, 4096, 4097, 12300} <= set(lens.tolist()) and (offs[1:-1] % 4096 == 0).any()
    assert ((offs[1:-1] % 4096 > 4096 - k) | (k == 1)).any(), "no boundary inside the last k - 1 starts of a tile"
    bands, rows = PERMS[num_perm]
    check(tok, ids, offs, k, num_perm, bands, rows, want=with_keys(sig, counts, num_perm, bands, rows))


def test_every_shingle_a_short_one(tok):
    """4096 documents of 1 to 3 ids with k = 5: a tile holds some 2000 documents, every one makes one shingle of its own length."""
    ids, offs = mt.limit_cases(5)["all_short"]
    want = check(tok, ids, offs, 5, 128, 4, 32)
    assert want[2].tolist() == [4096, 0, 4096, 0]
    one = np.flatnonzero(np.diff(offs) == 1)
    same = one[ids[offs[one]] == ids[offs[one[0]]]]
    assert (want[0][same] == want[0][one[0]]).all()


def test_a_run_of_empty_documents_overflows_the_table(tok):
    ids, offs = mt.limit_cases(5)["empty_run"]
    want = check(tok, ids, offs, 5, 65, 13, 5)
    assert want[2].tolist() == [696 + 896, 5000, 0, 0] and (want[0][1:5001] == 0xFFFFFFFF).all()
    assert (want[1][1:5001] == want[1][1]).all() and not (want[1][[0, 5001]] == want[1][1]).any()


def test_first_and_last_documents_empty(tok):
    ids, offs = mt.limit_cases(5)["empty_ends"]
    check(tok, ids, offs, 5, 64, 2, 32)
    check(tok, ids[:0], np.zeros(4, dtype=np.int64), 5, 64, 2, 32)  # nothing but empty documents
    check(tok, ids[:0], np.zeros(1, dtype=np.int64), 5, 64, 0, 0)   # no document at all
    check(tok, ids[:3], [0, 3], 5, 4, 2, 2)                          # one short document


def test_ids_behind_the_last_offset_do_not_matter(tok):
    ids, offs = mt.limit_cases(5)["edges"]
    cut = offs[:-3]  # the last documents are no documents any more: their ids lie behind tok_offsets[n_docs]
    want = check(tok, ids, cut, 5, 128)
    other = ids.copy()
    other[int(cut[-1]):] = 7
    check(tok, other, cut, 5, 128, want=want)
    check(tok, ids[:int(cut[-1])], cut, 5, 128, want=want)


def test_label_stream(tok):
    ids, offs = mt.limit_cases(5)["labels"]
    assert (ids == -100).sum() > 2000
    check(tok, ids, offs, 5, 128, 16, 8)
    check(tok, [-100, 5], [0, 2], 1, 4)


def test_identical_documents_far_apart(tok):
    ids, offs = mt.limit_cases(5)["twins"]
    want = check(tok, ids, offs, 5, 256, 32, 8)
    assert (want[0][1] == want[0][3]).all() and (want[1][1] == want[1][3]).all() and not (want[0][1] == want[0][2]).all()


# ---- the device form ----------------------------------------------------------------------------------------------------------------

def device_call(tok, ids, offs, spec, stream, n_tokens=None, shift=0, slack=5, keys=True):
    """-> (sig, keys | None, counts) as numpy arrays after the stream's work is done, slack untouched = bool, the status and its position."""
    import torch
    dev = torch.device("cuda", 0)
    ids, offs = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(offs, dtype=np.int64)
    n_docs = len(offs) - 1
    P, B = max(min(int(spec.num_perm), 1024), 1), max(min(int(spec.bands), 1024), 0)
    with torch.cuda.stream(stream):
        raw = torch.from_numpy(np.concatenate([np.zeros(shift, np.int32), ids, np.zeros(1, np.int32)])).to(dev)
        d_offs = torch.from_numpy(offs).to(dev)
        d_sig = torch.full((n_docs * P + slack,), FILL, dtype=torch.int32, device=dev)
        d_keys = torch.full((n_docs * B + slack,), FILL, dtype=torch.int64, device=dev)
        d_counts = torch.full((4,), FILL, dtype=torch.int64, device=dev)
    s = stream.cuda_stream
    tok.minhash_device(raw.data_ptr() + 4 * shift, len(ids) if n_tokens is None else n_tokens, d_offs.data_ptr(), n_docs, spec,
                       d_sig.data_ptr(), d_keys.data_ptr() if keys else 0, d_counts.data_ptr(), s)
    rc, where = tok.device_status_pos(s)
    stream.synchronize()
    sig, kk, counts = d_sig.cpu().numpy(), d_keys.cpu().numpy(), d_counts.cpu().numpy()
    slack_ok = bool((sig[n_docs * P:] == FILL).all() and (kk[n_docs * B:] == FILL).all())
    out = (sig[:n_docs * P].view(np.uint32).reshape(n_docs, P), kk[:n_docs * B].view(np.uint64).reshape(n_docs, B) if keys else None, counts)
    return out, slack_ok, rc, where


def untouched(out):
    return all(a is None or bool((a == FILL).all()) for a in out)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_ids_off_the_16_byte_grid(tok, side, shift):
    from tokendagger_amd import capi
    ids, offs, sig, counts = edge_truth(5)
    out, slack_ok, rc, _ = device_call(tok, ids, offs, capi.minhash_spec(5, 65, 1, 13, 5), side, shift=shift)
    assert rc == capi.TD_OK and slack_ok
    mt.same(out, with_keys(sig, counts, 65, 13, 5), shift)


def test_bands_and_slack(tok, side):
    from tokendagger_amd import capi
    ids, offs, sig, counts = edge_truth(13)
    for num_perm, bands, rows in ((64, 16, 4), (64, 7, 9), (128, 1, 1), (128, 128, 1)):
        out, slack_ok, rc, _ = device_call(tok, ids, offs, capi.minhash_spec(13, num_perm, 1, bands, rows), side)
        assert rc == capi.TD_OK and slack_ok
        mt.same(out, with_keys(sig, counts, num_perm, bands, rows), (num_perm, bands, rows))
    # no keys: a null pointer, and a buffer that is given stays as it was
    out, slack_ok, rc, _ = device_call(tok, ids, offs, capi.minhash_spec(13, 64), side, keys=False)
    assert rc == capi.TD_OK and slack_ok and out[1] is None and np.array_equal(out[0], sig[:, :64]) and np.array_equal(out[2], counts)
    out, slack_ok, rc, _ = device_call(tok, ids, offs, capi.minhash_spec(13, 64), side)
    assert rc == capi.TD_OK and slack_ok and np.array_equal(out[0], sig[:, :64])


def test_bad_specs_are_refused_before_a_launch(tok, side):
    from tokendagger_amd import capi
    S = capi.MinhashSpec
    ids, offs, sig, counts = edge_truth(5)
    bad = [S(0, 8, 1, 0, 0, 0), S(65, 8, 1, 0, 0, 0), S(-5, 8, 1, 0, 0, 0), S(5, 0, 1, 0, 0, 0), S(5, 1025, 1, 0, 0, 0), S(5, -1, 1, 0, 0, 0),
           S(5, 8, 1, -1, 1, 0), S(5, 8, 1, 2, 0, 0), S(5, 8, 1, 2, -4, 0), S(5, 8, 1, 2, 5, 0), S(5, 8, 1, 9, 1, 0), S(5, 8, 1, 2**32, 2**32, 0),
           S(5, 8, 1, 0, 0, 1), S(5, 8, 1, 0, 0, -1)]
    for spec in bad:
        what = [getattr(spec, f[0]) for f in spec._fields_]
        with pytest.raises(capi.TokenDaggerHipError) as e:
            device_call(tok, ids, offs, spec, side)
        assert e.value.code == capi.TD_E_INVALID and "td_minhash_device" in str(e.value), what
        with pytest.raises(capi.TokenDaggerHipError) as e:
            tok.minhash(ids, offs, spec)
        assert e.value.code == capi.TD_E_INVALID, what
    with pytest.raises(capi.TokenDaggerHipError) as e:  # band keys asked for, nowhere to put them
        device_call(tok, ids, offs, capi.minhash_spec(5, 8, 1, 2, 4), side, keys=False)
    assert e.value.code == capi.TD_E_INVALID
    import torch
    with pytest.raises(capi.TokenDaggerHipError) as e:  # the null stream
        t = torch.zeros(64, dtype=torch.int64, device="cuda")
        tok.minhash_device(t.data_ptr(), 4, t.data_ptr(), 1, capi.minhash_spec(5, 8), t.data_ptr(), 0, t.data_ptr(), 0)
    assert e.value.code == capi.TD_E_INVALID and "null stream" in str(e.value)
    rc, _ = tok.device_status_pos(side.cuda_stream)
    assert rc == capi.TD_OK  # nothing was launched that could have raised
    out, slack_ok, rc, _ = device_call(tok, ids, offs, capi.minhash_spec(5, 8), side)  # the next good call
    assert rc == capi.TD_OK and np.array_equal(out[0], sig[:, :8])


def test_bad_offsets_raise_through_device_status(tok, side):
    from tokendagger_amd import capi
    ids, offs, sig, counts = edge_truth(5)
    spec = capi.minhash_spec(5, 64, 1, 16, 4)
    d = 7 + int(np.flatnonzero(np.diff(offs[7:]) > 0)[0])  # document d is not empty
    dec = offs.copy()
    dec[d], dec[d + 1] = offs[d + 1], offs[d]               # d - 1 and d + 1 grow, d decreases
    first = offs.copy()
    first[0] = 1
    neg = offs.copy()
    neg[0] = -1
    above = int(np.searchsorted(offs, len(ids) - 10, side="right")) - 1  # the first document that ends above n_tokens = len(ids) - 10
    assert 0 < above < len(offs) - 2
    cases = [(dec, None, d), (first, None, 0), (neg, None, 0), (offs, len(ids) - 10, above)]
    for o, n_tokens, where_want in cases:
        out, slack_ok, rc, where = device_call(tok, ids, o, spec, side, n_tokens=n_tokens)
        assert rc == capi.TD_E_INVALID and where == where_want, (rc, where, where_want)
        assert untouched(out) and slack_ok, "an output was written although the offsets are bad"
        out, slack_ok, rc, _ = device_call(tok, ids, offs, spec, side)  # (the error is cleared; the next good call)
        assert rc == capi.TD_OK
        mt.same(out, with_keys(sig, counts, 64, 16, 4))
    with pytest.raises(capi.TokenDaggerHipError) as e:  # the host form checks its offsets like every host entry point, before any launch
        tok.minhash(ids, dec, spec)
    assert e.value.code == capi.TD_E_INVALID
    with pytest.raises(capi.TokenDaggerHipError):
        tok.minhash(ids, offs, spec, n_tokens=len(ids) - 10)


def test_device_form_on_a_side_stream_and_on_poisoned_workspaces(tok, side):
    from tokendagger_amd import capi
    ids, offs, sig, counts = edge_truth(5)
    spec = capi.minhash_spec(5, 128, 1, 32, 4)
    host = capi.minhash_host(ids, offs, spec)
    mt.same(host, with_keys(sig, counts, 128, 32, 4))
    runs = []
    for fill in (-1, 0x5A, 0xFF):  # a handle of its own each: its workspace is filled from its first allocation on
        tok.set_option(capi.TD_OPT_WS_FILL, fill)
        try:
            h = tok.clone()
        finally:
            tok.set_option(capi.TD_OPT_WS_FILL, -1)
        out, slack_ok, rc, _ = device_call(h, ids, offs, spec, side)
        assert rc == capi.TD_OK and slack_ok
        out2, _, rc, _ = device_call(h, ids, offs, capi.minhash_spec(5, 128, 2, 32, 4), side)  # another family: the table is rebuilt
        assert rc == capi.TD_OK and not np.array_equal(out2[0], out[0])
        again, _, rc, _ = device_call(h, ids, offs, spec, side)
        assert rc == capi.TD_OK
        mt.same(again, out, fill)
        runs.append(out)
    for out in runs:
        for a, b, c in zip(out, runs[0], host):
            assert a.tobytes() == b.tobytes() == c.tobytes()


# ---- encode + signatures, the Tokenizer's methods ----------------------------------------------------------------------------------

def test_encode_batch_to_minhash_equals_ids_to_minhash(tok, golden):
    import tokendagger as tiktoken
    from tokendagger_amd import capi
    n_docs = 400
    text, doc_offs = golden["text"], golden["offsets"].astype(np.int64)[:n_docs + 1]
    offs = golden["enc_offsets"].astype(np.int64)[:n_docs + 1]
    ids = golden["enc"].astype(np.int32)[:int(offs[-1])]
    want = mt.minhash_numpy(ids, offs, 5, 128, 1, 16, 8)
    sig, keys, counts, total = tok.encode_batch_minhash(text[:int(doc_offs[-1])], doc_offs, capi.minhash_spec(5, 128, 1, 16, 8))
    assert total == len(ids)
    mt.same((sig, keys, counts), want)
    pat, mr, special = H.llama4()
    tk = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    a = tk.ids_to_minhash(ids, offs, bands=16)
    b, n = tk.encode_batch_to_minhash(text[:int(doc_offs[-1])], doc_offs, bands=16)
    assert n == len(ids)
    mt.same(a, want)
    mt.same(b, want)
    assert a.similarity(3, 3) == 1.0 and a.similarity(3, 4) == float(np.mean(want[0][3] == want[0][4]))
    c = tk.ids_to_minhash(ids, offs, ngram=13, num_perm=64, seed=9)
    assert c.band_keys is None
    mt.same((c.signatures, np.zeros((n_docs, 0), np.uint64), c.counts), mt.minhash_numpy(ids, offs, 13, 64, 9))
    with pytest.raises(tiktoken.TokenDaggerError):
        tk.ids_to_minhash(ids, offs, ngram=65)
    with pytest.raises(tiktoken.TokenDaggerError):
        tk.ids_to_minhash(ids, offs, num_perm=64, bands=65)
