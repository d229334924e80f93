"""MinHash signatures without a GPU: the two truths of tests/minhash_truth.py against the contract's known answers and each other,
td_minhash_params and td_minhash_host through the C ABI against them with every argument error of the contract, the CPU model of the
kernel's decomposition (tests/twin/minhash_model.cpp over tokendagger_amd/csrc/td_minhash_args.h) at tile sizes 64, 256 and 4096, and
a statistical check that the family estimates the Jaccard similarity it is meant to estimate."""
import ctypes
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import minhash_truth as mt
from tokendagger_amd import capi
from tokendagger_amd.capi import MinhashSpec, minhash_host, minhash_params, minhash_spec  # noqa: F401  (the feature under test: without it nothing here runs)

ROOT = Path(__file__).resolve().parents[1]

# (k, num_perm, bands, rows): every k and num_perm of the GPU test's lists once; bands * rows == and < num_perm, and none
SHAPES = [(1, 1, 1, 1), (2, 63, 9, 7), (5, 64, 0, 0), (13, 65, 13, 5), (64, 128, 32, 4), (5, 1024, 20, 50)]


@pytest.fixture(scope="module")
def cases():
    """Built once, shared and left unchanged: (k, num_perm, bands, rows) -> {name: (ids, offs, truth)}."""
    out = {}
    for k, num_perm, bands, rows in SHAPES:
        out[(k, num_perm, bands, rows)] = {name: (ids, offs, mt.minhash_numpy(ids, offs, k, num_perm, 1, bands, rows))
                                           for name, (ids, offs) in mt.limit_cases(k).items()}
    return out


def test_known_answers():
    a, b = mt.params(1, 4)
    assert [hex(int(v)) for v in a] == ["0x910a2dec89025cc1", "0xf893a2eefb32555f", "0x71bb54d8d101b5b9", "0xe099ec6cd7363ca5"]
    assert [hex(int(v)) for v in b] == ["0xbeeb8da1658eec67", "0x71c18690ee42c90b", "0xc34d0bff90150280", "0x85e7bb0f12278575"]
    ca, cb = minhash_params(1, 4)
    assert np.array_equal(ca, a) and np.array_equal(cb, b)
    assert mt.doc_shingles([1, 2, 3, 4, 5, 6, 7], 5) == [0xa983f85b, 0xe4ec5be0, 0x742e9c03]
    assert mt.doc_shingles([1, 2, 3], 5) == [0x46b5bcab]
    assert mt.doc_shingles([-100, 5], 1) == [0x8db32d28, 0x6f92cac1]
    for fn in (mt.minhash_brute, mt.minhash_numpy, lambda i, o, *s: minhash_host(i, o, minhash_spec(*s))):
        sig, keys, counts = fn([1, 2, 3, 4, 5, 6, 7], [0, 7], 5, 4, 1, 2, 2)
        assert sig[0].tolist() == [0x149beb58, 0x79e37166, 0x30668f6e, 0x4f6d2506]
        assert keys[0].tolist() == [0x2ce97653853fdfd9, 0xe10eaebaa27b1107] and counts.tolist() == [3, 0, 0, 0]
        sig, keys, counts = fn([1, 2, 3], [0, 3], 5, 4, 1, 0, 0)
        assert sig[0].tolist() == [0x40257347, 0x73ae3a9a, 0x94303036, 0x822593bc] and counts.tolist() == [1, 0, 1, 0]
        sig, _, counts = fn([-100, 5], [0, 2], 1, 2, 1, 0, 0)
        want = [min(((int(a[j]) * x + int(b[j])) & mt.M64) >> 32 for x in (0x8db32d28, 0x6f92cac1)) for j in range(2)]
        assert sig[0].tolist() == want and counts.tolist() == [2, 0, 0, 0]


def test_truths_agree():
    rng = np.random.default_rng(3)
    for it in range(25):
        k = int(rng.integers(1, 9))
        offs = mt.offsets_of(rng.integers(0, 2 * k + 3, size=int(rng.integers(0, 12))))
        ids = rng.integers(-3, 50, size=int(offs[-1]) + 2).astype(np.int32)  # (two ids behind the last document)
        bands = int(rng.integers(0, 4))
        mt.same(mt.minhash_numpy(ids, offs, k, 7, it, bands, 2), mt.minhash_brute(ids[:int(offs[-1])], offs, k, 7, it, bands, 2), it)


def test_params_equal_the_truth():
    for seed in (0, 1, 2**63, 2**64 - 1):
        a, b = minhash_params(seed, 1024)
        ta, tb = mt.params(seed, 1024)
        assert np.array_equal(a, ta) and np.array_equal(b, tb) and np.all(a & np.uint64(1))
    for n in (0, -1, 1025):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            minhash_params(1, n)
        assert e.value.code == capi.TD_E_INVALID


def test_host_statement_equals_the_truths(cases):
    for (k, num_perm, bands, rows), by_name in cases.items():
        for name, (ids, offs, want) in by_name.items():
            sig, keys, counts = minhash_host(ids, offs, minhash_spec(k, num_perm, 1, bands, rows))
            if bands == 0:
                assert keys is None
                keys = np.zeros((len(offs) - 1, 0), dtype=np.uint64)
            mt.same((sig, keys, counts), want, (name, k, num_perm))
    # a signature is a prefix of the one with more permutations; another seed gives another family
    ids, offs, want = cases[(5, 1024, 20, 50)]["edges"]
    assert np.array_equal(minhash_host(ids, offs, minhash_spec(5, 100))[0], want[0][:, :100])
    assert not np.array_equal(minhash_host(ids, offs, minhash_spec(5, 100, seed=2))[0], want[0][:, :100])
    # ids behind tok_offsets[n_docs] are not looked at
    more = np.concatenate([ids, [5, 5, 5, 5, 5, 5]]).astype(np.int32)
    assert np.array_equal(minhash_host(more, offs, minhash_spec(5, 100))[0], want[0][:, :100])
    # rows=None: num_perm // bands; documents without an id share their keys, and nobody else's
    _, keys, _ = minhash_host(ids, offs, minhash_spec(5, 64, bands=16))
    assert np.array_equal(keys, mt.minhash_numpy(ids, offs, 5, 64, 1, 16, 4)[1])
    empty = np.flatnonzero(np.diff(offs) == 0)
    assert len(empty) >= 2 and (keys[empty] == keys[empty[0]]).all()
    assert not (keys[np.diff(offs) > 0] == keys[empty[0]]).any()


def test_host_statement_errors():
    lib = capi.load_library()
    ids, offs = np.arange(10, dtype=np.int32), np.asarray([0, 4, 10], dtype=np.int64)

    def call(spec, o=offs, sig=True, keys=True, counts=True, n_tokens=10, have_ids=True):
        s, kk, c = np.full((2, 8), 7, dtype=np.uint32), np.full((2, 8), 7, dtype=np.uint64), np.full(4, 7, dtype=np.int64)
        rc = lib.td_minhash_host(ids.ctypes.data if have_ids else None, n_tokens, o.ctypes.data, len(o) - 1, ctypes.byref(spec) if spec else None,
                                 s.ctypes.data if sig else None, kk.ctypes.data if keys else None, c.ctypes.data if counts else None)
        return rc, bool((s == 7).all() and (kk == 7).all() and (c == 7).all())

    rc, untouched = call(minhash_spec(5, 8, 1, 2, 4))
    assert rc == capi.TD_OK and not untouched
    bad_specs = [MinhashSpec(0, 8, 1, 0, 0, 0), MinhashSpec(65, 8, 1, 0, 0, 0), MinhashSpec(-1, 8, 1, 0, 0, 0), MinhashSpec(5, 0, 1, 0, 0, 0),
                 MinhashSpec(5, 1025, 1, 0, 0, 0), MinhashSpec(5, 8, 1, -1, 1, 0), MinhashSpec(5, 8, 1, 2, 0, 0), MinhashSpec(5, 8, 1, 2, 5, 0),
                 MinhashSpec(5, 8, 1, 9, 1, 0), MinhashSpec(5, 8, 1, 2**32, 2**32, 0), MinhashSpec(5, 8, 1, 0, 0, 1), None]
    for spec in bad_specs:
        rc, untouched = call(spec)
        assert rc == capi.TD_E_INVALID and untouched, spec and [getattr(spec, f[0]) for f in spec._fields_]
    for o in ([1, 4, 10], [0, 5, 4], [0, 4, 11], [-1, 4, 10]):
        rc, untouched = call(minhash_spec(5, 8), np.asarray(o, dtype=np.int64))
        assert rc == capi.TD_E_INVALID and untouched, o
    for kw in (dict(sig=False), dict(counts=False), dict(n_tokens=-1), dict(have_ids=False)):
        rc, untouched = call(minhash_spec(5, 8, 1, 2, 4), **kw)
        assert rc == capi.TD_E_INVALID and untouched, kw
    rc, untouched = call(minhash_spec(5, 8, 1, 2, 4), keys=False)  # band keys asked for, nowhere to put them
    assert rc == capi.TD_E_INVALID and untouched
    assert call(minhash_spec(5, 8), keys=False)[0] == capi.TD_OK  # bands = 0 with a null keys pointer
    with pytest.raises(capi.TokenDaggerHipError) as e:
        minhash_host(ids, offs, minhash_spec(5, 8, bands=9))
    assert e.value.code == capi.TD_E_INVALID


def test_exports():
    names = ["td_minhash_params", "td_minhash_host", "td_minhash_device", "td_minhash", "td_encode_batch_minhash"]
    lib = capi.load_library()
    for n in names:
        assert n in capi.EXPORTS and hasattr(lib, n)
    for n in ("minhash", "minhash_device", "encode_batch_minhash"):
        assert callable(getattr(capi.HipTokenizer, n))


# ---- the model ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    src = ROOT / "tests" / "twin" / "minhash_model.cpp"
    out = ROOT / "tests" / "twin" / "_build" / "libminhashmodel.so"
    out.parent.mkdir(parents=True, exist_ok=True)
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))  # (td_minhash_args.h takes __host__ __device__ from HIP's host header)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__",
                           f"-I{rocm / 'include'}", str(src), "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.minhash_model.restype = i32
    lib.minhash_model.argtypes = [vp, vp, i64, i32, i32, i32, ctypes.c_uint64, i32, i32, vp, vp, vp, vp]
    return lib


def run_model(lib, ids, offs, k, num_perm, bands, rows, tile=4096, seed=1):
    """-> ((sig, keys, counts), stats = tiles, windows hashed, merges, most documents of a tile, (document, wavefront) runs, short shingles)."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    n_docs = len(offs) - 1
    sig = np.zeros((max(n_docs, 1), num_perm), dtype=np.uint32)
    keys = np.zeros((max(n_docs, 1), max(bands, 1)), dtype=np.uint64)
    counts, stats = np.zeros(4, dtype=np.int64), np.zeros(6, dtype=np.int64)
    rc = lib.minhash_model(ids.ctypes.data if len(ids) else None, offs.ctypes.data, n_docs, tile, k, num_perm, seed, bands, rows,
                           sig.ctypes.data, keys.ctypes.data, counts.ctypes.data, stats.ctypes.data)
    assert rc == 0, ("a rolled hash differs from the recomputed one" if rc == 2 else "bad arguments", rc)
    return (sig[:n_docs], keys[:n_docs, :bands], counts), stats


@pytest.mark.parametrize("tile", [64, 256, 4096])
def test_model_equals_the_truths(model, cases, tile):
    for (k, num_perm, bands, rows), by_name in cases.items():
        if tile < 4096 and num_perm == 1024:
            continue  # (the chunks are walked at 128 and 65 already; the small tiles multiply the merges)
        for name, (ids, offs, want) in by_name.items():
            got, stats = run_model(model, ids, offs, k, num_perm, bands, rows, tile=tile)
            mt.same(got, want, (name, k, num_perm, tile))
            total = int(offs[-1])
            assert stats[0] == -(-total // tile) and stats[2] == stats[4] * -(-num_perm // 64)
            assert stats[5] == want[2][2], "a short document makes one shingle, in one tile, in one wavefront"
            if name == "all_short" and tile == 4096:
                assert stats[3] > 1024, "more documents in a tile than a wavefront has starts to spare"
            if name == "empty_run" and tile == 4096:
                assert stats[3] > 4352, "the run of empty documents does not overflow the kernel's table"


def test_model_merges_once_per_document_wavefront_and_chunk(model):
    """A document over many tiles gets one merge per wavefront quarter and chunk, not one per lane or per shingle."""
    ids = np.random.default_rng(5).integers(0, 200000, size=12300).astype(np.int32)
    got, stats = run_model(model, ids, [0, 12300], 5, 128, 0, 0)
    mt.same(got, mt.minhash_numpy(ids, [0, 12300], 5, 128, 1, 0, 0))
    assert stats[0] == 4 and stats[4] == 13 and stats[2] == 26 and got[2][0] == 12296


# ---- the family is useful, not only self-consistent -------------------------------------------------------------------------------

def shingle_set(doc, k):
    return {w.tobytes() for w in np.lib.stride_tricks.sliding_window_view(np.asarray(doc, dtype=np.int32), k)}


def test_signature_agreement_estimates_jaccard():
    """72 pairs of 2000-id documents that share all but one redrawn block: the fraction of equal signature entries is a binomial
    estimate of the Jaccard similarity J of the two shingle sets, mean J and variance J (1 - J) / num_perm; it must lie within four
    standard deviations (derived, not measured: the prototype's largest deviation over these pairs was 2.7)."""
    rng = np.random.default_rng(2024)
    k, num_perm = 5, 256
    worst = 0.0
    for frac in (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9):
        for _ in range(8):
            d1 = rng.integers(0, 200000, 2000)
            n = int((1 - frac) * 2000)
            at = int(rng.integers(0, 2000 - n + 1))
            d2 = d1.copy()
            d2[at:at + n] = rng.integers(0, 200000, n)
            s1, s2 = shingle_set(d1, k), shingle_set(d2, k)
            J = len(s1 & s2) / len(s1 | s2)
            sig, _, _ = minhash_host(np.concatenate([d1, d2]), [0, 2000, 4000], minhash_spec(k, num_perm, 1))
            est = float(np.mean(sig[0] == sig[1]))
            sigma = np.sqrt(J * (1 - J) / num_perm)
            worst = max(worst, abs(est - J) / sigma)
            assert abs(est - J) <= 4 * sigma, (frac, J, est, sigma)
    print(f"largest deviation: {worst:.2f} sigma")
    d1 = rng.integers(0, 200000, 2000)
    d3 = rng.integers(0, 200000, 2000)
    sig, _, _ = minhash_host(np.concatenate([d1, d1, d3]), [0, 2000, 4000, 6000], minhash_spec(k, num_perm, 1))
    assert not (shingle_set(d1, k) & shingle_set(d3, k))
    assert (sig[0] == sig[1]).all() and not (sig[0] == sig[2]).any()
