"""N-gram matches without a GPU: the two truths of tests/ngram_truth.py against each other, td_ngram_matches_host through the C ABI
against both with every argument error of the contract, and the CPU model of the kernel's decomposition (tests/twin/ngram_model.cpp
over tokendagger_amd/csrc/td_ngram_args.h) against the truths at tile sizes 64, 256 and 4096 and at 1 to 4 tag bits, where it
must meet tag matches whose ids differ: the path the GPU test walks with TD_OPT_NGRAM_TAG_BITS."""
import ctypes
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ngram_truth as nt
from tokendagger_amd import capi
from tokendagger_amd.capi import NgramSpec, ngram_matches_host, ngram_spec  # noqa: F401  (the feature under test: without it nothing here runs)

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def cases():
    """Built once, shared and left unchanged: name -> (case, truth with labels = the ids)."""
    out = {}
    for name, c in nt.limit_cases().items():
        out[name] = (c, nt.matches_numpy(c["seqs"], c["ids"], c["offs"], labels=c["ids"]))
    return out


def test_truths_agree(cases):
    for name, (c, want) in cases.items():
        nt.same(nt.matches_brute(c["seqs"], c["ids"], c["offs"], labels=c["ids"]), want, name)
    c, want = cases["nested"]
    # [7,7] in 7,7,7,7: three occurrences; with [7,7,7] and [7]: 3 + 2 + 4 in the first run of four
    one = nt.matches_brute([[7, 7]], [7, 7, 7, 7], [0, 4])
    assert one[4].tolist() == [3, 4, 1, 0] and one[3].tolist() == [3]
    assert nt.matches_brute(c["seqs"], [7, 7, 7, 7], [0, 4])[3].tolist() == [3, 2, 4]
    # across a document border: nothing
    assert nt.matches_numpy([[1, 2, 3]], [1, 2, 3, 1, 2, 3], [0, 2, 4, 6])[4].tolist() == [0, 0, 0, 0]
    rng = np.random.default_rng(3)
    for it in range(30):
        d = nt.dense(rng, total=int(rng.integers(1, 400)), n_docs=int(rng.integers(1, 12)), n_pats=int(rng.integers(1, 30)))
        pc = rng.integers(0, 9, size=len(d["seqs"])).astype(np.int64)
        nt.same(nt.matches_brute(d["seqs"], d["ids"], d["offs"], labels=d["ids"], ignore=-5, pattern_counts=pc),
                nt.matches_numpy(d["seqs"], d["ids"], d["offs"], labels=d["ids"], ignore=-5, pattern_counts=pc), it)


def test_host_statement_equals_the_truths(cases):
    for name, (c, want) in cases.items():
        nt.same(ngram_matches_host(c["seqs"], c["ids"], c["offs"], labels=c["ids"]), want, name)
    c, want = cases["dense"]
    # outputs are optional; accumulate adds to the pattern counts that are there
    got = ngram_matches_host(c["seqs"], c["ids"], c["offs"], cover=False, doc_stats=False, pattern_counts=False)
    assert got[0] is None and got[2] is None and got[3] is None and np.array_equal(got[4], want[4])
    acc = want[3].copy()
    got = ngram_matches_host(c["seqs"], c["ids"], c["offs"], ngram_spec(accumulate=True), pattern_counts=acc)
    assert got[3] is acc and np.array_equal(acc, 2 * want[3])
    # ids behind tok_offsets[n_docs] are not looked at, slots there not written
    lab = np.concatenate([c["ids"], [5, 5, 5]]).astype(np.int32)
    got = ngram_matches_host([[5]], np.concatenate([c["ids"], [5, 5, 5]]), c["offs"], labels=lab)
    assert got[4].tolist() == [0, 0, 0, 0] and got[1][-3:].tolist() == [5, 5, 5]


def test_host_statement_errors():
    ids, offs = np.arange(10, dtype=np.int32), np.asarray([0, 4, 10], dtype=np.int64)
    ok = ngram_matches_host([[1, 2]], ids, offs)
    assert ok[4].tolist() == [1, 2, 1, 0]
    bad_lists = ([[]], [list(range(65))], [[1] * k for k in range(1, 10)], [[1, -2]], [])
    for seqs in bad_lists:
        with pytest.raises(capi.TokenDaggerHipError) as e:
            ngram_matches_host(seqs, ids, offs)
        assert e.value.code == capi.TD_E_INVALID, seqs
    for spec in (NgramSpec(-100, 2), NgramSpec(2**31, 0), NgramSpec(-2**31 - 1, 0)):
        with pytest.raises(capi.TokenDaggerHipError):
            ngram_matches_host([[1, 2]], ids, offs, spec)
    for o in ([1, 4, 10], [0, 5, 4], [0, 4, 11], [-1, 4, 10]):
        with pytest.raises(capi.TokenDaggerHipError):
            ngram_matches_host([[1, 2]], ids, np.asarray(o, dtype=np.int64))
    assert ngram_matches_host([list(range(64))], ids, offs)[4].tolist() == [0, 0, 0, 0]  # the longest length is fine


# ---- the model ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    src = ROOT / "tests" / "twin" / "ngram_model.cpp"
    out = ROOT / "tests" / "twin" / "_build" / "libngrammodel.so"
    out.parent.mkdir(parents=True, exist_ok=True)
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))  # (td_ngram_args.h takes __host__ __device__ from HIP's host header)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__",
                           f"-I{rocm / 'include'}", str(src), "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.ngram_model.restype = i32
    lib.ngram_model.argtypes = [vp, vp, i64, vp, vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    return lib


def run_model(lib, c, tile=4096, tag_bits=0, ignore=-100):
    """-> (the five outputs with labels = the ids, stats = failed id compares, longest probe, slots, adds to doc_stats, tiles, windows)."""
    pi, po = capi.ngram_patterns(c["seqs"])
    ids = np.ascontiguousarray(c["ids"], dtype=np.int32)
    offs = np.ascontiguousarray(c["offs"], dtype=np.int64)
    n_docs, total = len(offs) - 1, int(offs[-1])
    cover, labels = np.zeros(max(total, 1), dtype=np.uint8), ids.copy()
    stats_d, pc = np.zeros((max(n_docs, 1), 2), dtype=np.int64), np.zeros(len(po) - 1, dtype=np.int64)
    counts, stats = np.zeros(4, dtype=np.int64), np.zeros(6, dtype=np.int64)
    rc = lib.ngram_model(pi.ctypes.data, po.ctypes.data, len(po) - 1, ids.ctypes.data if len(ids) else None, offs.ctypes.data, n_docs, tile,
                         tag_bits, ignore, cover.ctypes.data, labels.ctypes.data if len(labels) else None, stats_d.ctypes.data, pc.ctypes.data,
                         counts.ctypes.data, stats.ctypes.data)
    assert rc == 0, ("a rolled hash differs from the recomputed one" if rc == 2 else "bad list", rc)
    return (cover[:total], labels, stats_d[:n_docs], pc, counts), stats


@pytest.mark.parametrize("tile", [64, 256, 4096])
def test_model_equals_the_truths(model, cases, tile):
    for name, (c, want) in cases.items():
        got, stats = run_model(model, c, tile=tile)
        nt.same(got, want, (name, tile))
        total = int(c["offs"][-1])
        assert stats[4] == -(-total // tile) and stats[2] >= 16 and stats[2] & (stats[2] - 1) == 0
        if name == "no_tokens":
            assert stats[5] == 0
    # a document over many tiles gets one add a tile, not one a lane or an id
    c, want = cases["nested"]
    got, stats = run_model(model, c, tile=64)
    assert 0 < stats[3] <= stats[4] + len(c["offs"])


@pytest.mark.parametrize("tag_bits", [1, 2, 3, 4])
def test_forced_collisions_walk_the_id_compare(model, tag_bits):
    c = nt.forced_collisions(np.random.default_rng(31))
    want = nt.matches_numpy(c["seqs"], c["ids"], c["offs"], labels=c["ids"])
    got, stats = run_model(model, c, tag_bits=tag_bits)
    nt.same(got, want, tag_bits)
    assert stats[0] > 0, "no tag match failed its id compare: the inputs do not force the path"
    full, stats_full = run_model(model, c, tag_bits=0)
    nt.same(full, want, "all 32 bits")
    assert stats_full[0] <= stats[0]


def test_model_probes_past_the_first_slot(model):
    """Enough patterns that some sit behind their first slot: found all the same, within the recorded distance."""
    rng = np.random.default_rng(41)
    seqs = [nt.pattern(rng, 4) for _ in range(3000)]
    total = nt.TILE + 99
    places = [(int(p), int(q)) for p, q in zip(rng.integers(0, 3000, size=150), rng.integers(0, total - 4, size=150))]
    c = nt.planted(rng, total, nt.random_offsets(rng, total, 5), seqs, places)
    got, stats = run_model(model, c)
    nt.same(got, nt.matches_numpy(c["seqs"], c["ids"], c["offs"], labels=c["ids"]))
    assert stats[1] >= 1 and got[4][0] >= 100
