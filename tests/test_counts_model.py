"""Token counts without a GPU: the two truths of tests/counts_truth.py against each other, the CPU model of the kernel's
decomposition (tests/twin/counts_model.cpp over tokendagger_amd/csrc/td_counts_args.h) against both truths at several seat
counts and flush intervals, and td_token_counts_host through the C ABI with every argument error of the contract."""
import ctypes
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import counts_truth as ct
from tokendagger_amd.capi import CountsSpec, counts_spec, token_counts_host  # noqa: F401  (the feature under test: without it nothing here runs)

ROOT = Path(__file__).resolve().parents[1]


def _same(a, b, what=""):
    assert a[0].dtype == b[0].dtype == np.int64 and a[0].shape == b[0].shape, what
    assert np.array_equal(a[0], b[0]), what
    assert np.array_equal(np.asarray(a[1], dtype=np.int64), np.asarray(b[1], dtype=np.int64)), (what, a[1], b[1])


def _truth_args(c):
    """A random case as the truths take it: one group visits every position and ignores documents and groups."""
    if c["n_groups"] == 1:
        return dict(ids=c["ids"], n_bins=c["n_bins"])
    return dict(ids=c["ids"], n_bins=c["n_bins"], tok_offsets=c["tok_offsets"], groups=c["groups"], n_groups=c["n_groups"])


def test_truths_agree_on_random_cases():
    rng = np.random.default_rng(11)
    seen = dict(empty_doc=0, negative=0, too_large=0, bad_group=0, lead=0, tail=0, grouped=0, one_group=0)
    for it in range(400):
        c = ct.random_case(rng, max_docs=12 if it % 8 else 60)
        a = ct.counts_brute(**_truth_args(c))
        _same(a, ct.counts_numpy(**_truth_args(c)), it)
        visited = len(c["ids"]) if c["n_groups"] == 1 else int(c["tok_offsets"][-1] - c["tok_offsets"][0])
        assert int(a[1].sum()) == visited and int(a[0].sum()) == int(a[1][0])
        seen["empty_doc"] += int((np.diff(c["tok_offsets"]) == 0).sum())
        seen["negative"] += int(a[1][1] > 0)
        seen["too_large"] += int(a[1][2] > 0)
        seen["bad_group"] += int(a[1][3] > 0)
        seen["lead"] += int(c["tok_offsets"][0] > 0)
        seen["tail"] += int(c["tok_offsets"][-1] < c["n_tokens"])
        seen["grouped"] += int(c["n_groups"] > 1)
        seen["one_group"] += int(c["n_groups"] == 1)
    assert all(v >= 50 for v in seen.values()), seen


# ---- the model ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    src = ROOT / "tests" / "twin" / "counts_model.cpp"
    out = ROOT / "tests" / "twin" / "_build" / "libcountsmodel.so"
    out.parent.mkdir(parents=True, exist_ok=True)
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))  # (td_counts_args.h takes __host__ __device__ from HIP's host header)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__",
                           f"-I{rocm / 'include'}", str(src), "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.counts_model.restype = i32
    lib.counts_model.argtypes = [vp, i64, vp, i64, vp, i64, i64, i32, i32, i32, i64, vp, vp, vp, vp]
    lib.counts_model_const.restype = i64
    lib.counts_model_const.argtypes = [i32, i64]
    return lib


def run_model(lib, ids, n_bins, tok_offsets=None, groups=None, n_groups=1, seats=0, flush=0, grid=0, table=0, counts=None):
    """-> (counts, info, stats = adds to the counts from conflicts, from flushes, adds to seats, tiles, (err, err_pos))."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    o = None if groups is None else np.ascontiguousarray(tok_offsets, dtype=np.int64)
    g = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
    counts = np.zeros((n_groups, n_bins), dtype=np.int64) if counts is None else counts
    info, stats, pos = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64), np.zeros(1, dtype=np.int64)
    err = lib.counts_model(ids.ctypes.data, len(ids), None if o is None else o.ctypes.data, 0 if o is None else len(o) - 1,
                           None if g is None else g.ctypes.data, n_bins, n_groups, int(seats).bit_length() - 1 if seats else 0, flush, grid,
                           table, counts.ctypes.data, info.ctypes.data, stats.ctypes.data, pos.ctypes.data)
    return counts, info, stats, (err, int(pos[0]))


def _check(lib, ids, n_bins, tok_offsets=None, groups=None, n_groups=1, what="", **kw):
    want = ct.counts_numpy(ids, n_bins, tok_offsets, groups, n_groups)
    got = run_model(lib, ids, n_bins, tok_offsets, groups, n_groups, **kw)
    _same(got[:2], want, (what, kw))
    bad = int(want[1][3])
    assert (got[3][0] != 0) == (bad > 0), (what, got[3])
    if bad:
        d = got[3][1]
        assert not 0 <= groups[d] < n_groups and tok_offsets[d + 1] > tok_offsets[d], (what, d)
    return got


SEATS = [2, 64, 0]  # (0: the production count)


def test_model_constants_match_the_kernel(model):
    common = (ROOT / "tokendagger_amd" / "csrc" / "td_rows_common.h").read_text()
    val = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", common).group(1))  # noqa: E731
    assert val("RC_LDS_DOCS") == 4352 and "4352" in (ROOT / "tests" / "twin" / "counts_model.cpp").read_text()
    assert model.counts_model_const(2, 0) == val("RC_TILE") == 4096
    assert model.counts_model_const(4, 0) <= val("RC_MAX_GRID")
    seats, flush = model.counts_model_const(0, 0), model.counts_model_const(1, 0)
    assert seats & (seats - 1) == 0 and flush * 4096 < 2**31  # a seat's 32-bit counter between two flushes
    assert model.counts_model_const(3, 0) == 1 and model.counts_model_const(3, 4096 * 8 + 1) == 2  # a small call flushes few tables
    assert model.counts_model_const(3, 1 << 40) == model.counts_model_const(4, 0)


@pytest.mark.parametrize("seats", SEATS)
def test_model_matches_truth_on_random_cases(model, seats):
    rng = np.random.default_rng(3)
    for it in range(150):
        c = ct.random_case(rng, max_docs=12 if it % 8 else 60)
        _check(model, what=it, seats=seats, **_truth_args(c))


@pytest.mark.parametrize("seats", SEATS)
def test_model_on_the_golden_ids(model, golden, seats):
    ids, offs = golden["enc"].astype(np.int32), golden["enc_offsets"].astype(np.int64)
    n_bins = int(ids.max()) + 1
    _check(model, ids, n_bins, seats=seats)
    groups = (np.arange(len(offs) - 1) % 7).astype(np.int32)
    _check(model, ids, n_bins, offs, groups, 7, seats=seats)


@pytest.mark.parametrize("seats", SEATS)
@pytest.mark.parametrize("flush", [0, 1])
def test_model_on_the_shaped_streams(model, seats, flush):
    n_bins, n = 50000, 5 * 4096 + 123
    kw = dict(seats=seats, flush=flush, grid=2)
    c, info, stats, _ = _check(model, np.full(n, 77, dtype=np.int32), n_bins, what="all equal", **kw)
    assert c[0, 77] == n
    _check(model, np.random.default_rng(1).permutation(n_bins).astype(np.int32), n_bins, what="every id distinct", **kw)
    cold_hot = np.concatenate([np.arange(1000, 1000 + 4096), np.full(6 * 4096, 5)]).astype(np.int32)
    _check(model, cold_hot, n_bins, what="cold tile first, then the hot id", grid=1, seats=seats, flush=flush)


@pytest.mark.parametrize("seats", SEATS)
def test_model_documents_at_tile_borders(model, seats):
    ids, offs, groups, n_bins, n_groups = ct.border_documents()
    _check(model, ids, n_bins, offs, groups, n_groups, seats=seats)
    _check(model, ids, n_bins, offs, groups, n_groups, seats=seats, flush=1, grid=3)
    ids, offs, groups, n_bins, n_groups = ct.empty_documents_tile()
    _check(model, ids, n_bins, offs, groups, n_groups, seats=seats)
    _check(model, ids, n_bins, offs, groups, n_groups, seats=seats, table=256)


def test_model_accumulates_and_starts_above_zero(model):
    ids = np.random.default_rng(2).integers(-3, 40, size=10000).astype(np.int32)
    offs = np.asarray([4090, 4097, 4097, 9000], dtype=np.int64)
    groups = np.asarray([1, 0, 1], dtype=np.int32)
    c, info, _, _ = _check(model, ids, 32, offs, groups, 2)
    c2, _, _, _ = run_model(model, ids, 32, offs, groups, 2, counts=c.copy())
    assert np.array_equal(c2, 2 * c) and int(info.sum()) == 9000 - 4090


def test_model_raises_offsets_that_decrease_or_leave_the_buffer(model):
    ids, offs, groups, n_bins, n_groups = ct.border_documents()
    down = offs.copy()
    down[4] = down[3] - 50
    c, info, _, (err, pos) = run_model(model, ids, n_bins, down, groups, n_groups)
    assert err == 1 and pos == 3 and int(info.sum()) == len(ids) and int(c.sum()) == int(info[0])
    c, info, _, (err, pos) = run_model(model, ids[:-5000], n_bins, offs, groups, n_groups)
    assert err == 1 and pos == len(groups) and int(info.sum()) == len(ids) - 5000


def test_model_global_add_share_of_the_golden_ids(model, golden):
    """The figure DESIGN 4.16 records (nothing asserts its size): adds that reach global memory per id."""
    ids = golden["enc"].astype(np.int32)
    _, info, stats, _ = run_model(model, ids, int(ids.max()) + 1)
    print(f"golden ids: {len(ids)} ids, conflict adds {stats[0]}, flush adds {stats[1]}, seat adds {stats[2]}, tiles {stats[3]}; "
          f"global adds per id {(stats[0] + stats[1]) / len(ids):.4f}")
    assert int(info[0]) == len(ids)


# ---- td_token_counts_host through the C ABI --------------------------------------------------------------------------------------

def test_host_statement_matches_the_truths():
    from tokendagger_amd import capi
    rng = np.random.default_rng(21)
    errors = 0
    for it in range(300):
        c = ct.random_case(rng)
        spec = capi.counts_spec(c["n_bins"], c["n_groups"])
        grouped = c["n_groups"] > 1
        want = ct.counts_brute(**_truth_args(c))
        if want[1][3] or (grouped and np.any((c["groups"] < 0) | (c["groups"] >= c["n_groups"]))):
            errors += 1
            with pytest.raises(capi.TokenDaggerHipError) as e:
                capi.token_counts_host(c["ids"], c["tok_offsets"], c["groups"], spec)
            bad = np.flatnonzero((c["groups"] < 0) | (c["groups"] >= c["n_groups"]))
            assert e.value.code == capi.TD_E_INVALID and int(e.value.info[0]) == int(bad[0])
            continue
        got = capi.token_counts_host(c["ids"], c["tok_offsets"] if grouped else None, c["groups"] if grouped else None, spec)
        _same(got, want, it)
        _same(got, ct.counts_numpy(**_truth_args(c)), it)
        acc = got[0].copy().reshape(-1)
        again = capi.token_counts_host(c["ids"], c["tok_offsets"] if grouped else None, c["groups"] if grouped else None,
                                       capi.counts_spec(c["n_bins"], c["n_groups"], accumulate=True), counts=acc)
        assert np.array_equal(again[0], 2 * got[0]) and np.array_equal(again[1], got[1])
    assert errors >= 20


def test_host_statement_argument_errors():
    from tokendagger_amd import capi
    lib = capi.load_library()
    ids = np.asarray([1, 2, 3, 4], dtype=np.int32)
    offs = np.asarray([0, 2, 4], dtype=np.int64)
    grp = np.asarray([0, 1], dtype=np.int32)
    counts = np.full(16, -7, dtype=np.int64)
    info = np.zeros(4, dtype=np.int64)

    def call(spec, ids_p=ids.ctypes.data, n=4, offs_p=offs.ctypes.data, n_docs=2, grp_p=grp.ctypes.data, counts_p=counts.ctypes.data,
             info_p=info.ctypes.data):
        info[:] = 99
        return lib.td_token_counts_host(ids_p, n, offs_p, n_docs, grp_p, ctypes.byref(spec) if spec is not None else None, counts_p, info_p)

    S = capi.CountsSpec
    bad_specs = [S(0, 1, 0), S(-1, 1, 0), S(8, 0, 0), S(8, -2, 0), S(1 << 27, 4, 0), S(1 << 40, 1 << 40, 0), S(8, 2, 2), S(8, 2, -1), None]
    for spec in bad_specs:
        assert call(spec) == capi.TD_E_INVALID and info[0] == -1, spec
    assert call(S(8, 2, 0), offs_p=None) == capi.TD_E_INVALID and info[0] == -1        # groups without offsets
    assert call(S(8, 2, 0), grp_p=None) == capi.TD_E_INVALID and info[0] == -1         # ... without doc_group
    assert call(S(8, 2, 0), n=-1) == capi.TD_E_INVALID and info[0] == -1
    assert call(S(8, 2, 0), n_docs=-1) == capi.TD_E_INVALID and info[0] == -1
    assert call(S(8, 2, 0), n=3) == capi.TD_E_INVALID and info[0] == -1                # offsets end above n_tokens
    assert call(S(8, 2, 0), ids_p=None) == capi.TD_E_INVALID and info[0] == -1         # positions to visit, no ids
    assert call(S(8, 2, 0), counts_p=None) == capi.TD_E_INVALID and info[0] == -1
    assert call(S(8, 2, 0), info_p=None) == capi.TD_E_INVALID
    down = np.asarray([0, 3, 2], dtype=np.int64)
    assert call(S(8, 2, 0), offs_p=down.ctypes.data) == capi.TD_E_INVALID and info[0] == -1
    neg = np.asarray([-1, 2, 4], dtype=np.int64)
    assert call(S(8, 2, 0), offs_p=neg.ctypes.data) == capi.TD_E_INVALID and info[0] == -1
    for g, d in (([0, 2], 1), ([-1, 5], 0), ([1, -1], 1)):
        gg = np.asarray(g, dtype=np.int32)
        assert call(S(8, 2, 0), grp_p=gg.ctypes.data) == capi.TD_E_INVALID and info[0] == d
    assert np.all(counts == -7)  # no error touched the counts
    # the limits that are allowed: exactly 2^28 keys is a valid spec (not run: 2 GiB of counts); one group ignores documents and groups
    assert call(S(8, 1, 0), offs_p=None, n_docs=0, grp_p=None) == capi.TD_OK and info.tolist() == [4, 0, 0, 0]
    assert counts[:8].tolist() == [0, 1, 1, 1, 1, 0, 0, 0] and np.all(counts[8:] == -7)
    assert call(S(3, 2, 0)) == capi.TD_OK and info.tolist() == [2, 0, 2, 0] and counts[:6].tolist() == [0, 1, 1, 0, 0, 0]
    assert call(S(8, 1, 0), ids_p=None, n=0, offs_p=None, n_docs=0, grp_p=None) == capi.TD_OK and info.tolist() == [0, 0, 0, 0]
