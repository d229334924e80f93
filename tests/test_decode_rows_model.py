"""Decode rows without a GPU: the two truths of tests/decode_rows_truth.py against each other, the aggregate's operator, the CPU
model of the kernels' decomposition (tests/twin/decode_rows_model.cpp over tokendagger_amd/csrc/td_decode_rows_args.h) against both
truths at three tile sizes, and td_decode_rows_check through the C ABI with every argument error of the contract."""
import ctypes
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import decode_rows_truth as dt
import helpers as H
from tokendagger_amd import capi
from tokendagger_amd.capi import DecodeSpec, decode_rows_check, decode_spec  # noqa: F401  (the feature under test: without it nothing here runs)

ROOT = Path(__file__).resolve().parents[1]


def _same(a, b, what=""):
    assert a[0] == b[0], what
    for x, y in zip(a[1:], b[1:]):
        assert x.dtype == y.dtype == np.int64 and np.array_equal(x, y), (what, x, y)


def _both(c):
    """Both truths on a random case -> the result, or the DecodeError both raised."""
    try:
        a = dt.decode_brute(c["ids"], c["tok"], **c["kw"])
    except dt.DecodeError as e:
        with pytest.raises(dt.DecodeError) as e2:
            dt.decode_numpy(c["ids"], dt.Vocab(c["tok"]), **c["kw"])
        assert (e.code, e.pos) == (e2.value.code, e2.value.pos)
        return e
    _same(a, dt.decode_numpy(c["ids"], dt.Vocab(c["tok"]), **c["kw"]))
    return a


def test_codes_are_the_headers():
    assert (dt.E_INVALID, dt.E_BAD_TOKEN) == (capi.TD_E_INVALID, capi.TD_E_BAD_TOKEN)
    assert (capi.TD_DECODE_KEEP_STOP, capi.TD_DECODE_SKIP_NEGATIVE, capi.TD_DECODE_SKIP_SPECIAL) == (1, 2, 4)


def test_truths_agree_on_random_cases():
    rng = np.random.default_rng(17)
    seen = dict(empty_segment=0, stop_present=0, stop_first=0, junk_behind_stop=0, negative_skipped=0, listed_above_max_id=0,
                row_len_zero=0, row_len_stride=0, skipped_and_stop=0, lead=0, tail=0, error=0)
    for it in range(400):
        c = dt.random_case(rng)
        kw, ids, tok = c["kw"], c["ids"], c["tok"]
        r = _both(c)
        if isinstance(r, dt.DecodeError):
            seen["error"] += 1
            continue
        out, offs, seg_ids, info = r
        assert info[0] == len(out) == offs[-1] and info[1] + info[2] == seg_ids.sum() and offs[0] == 0
        rows = kw.get("row_stride", 0) > 0
        n = len(seg_ids)
        lens = (np.diff(kw["tok_offsets"]) if not rows else
                (np.full(n, kw["row_stride"]) if kw["lengths"] is None else np.asarray(kw["lengths"])))
        first = kw["tok_offsets"][:-1] if not rows else np.arange(n) * kw["row_stride"]
        seen["empty_segment"] += int((lens == 0).any())
        seen["stop_present"] += int(info[3] > 0)
        stopped = [d for d in range(n) if seg_ids[d] and int(ids[first[d] + seg_ids[d] - 1]) in kw["stop"]]
        seen["stop_first"] += int(any(seg_ids[d] == 1 for d in stopped))
        behind = [int(x) for d in stopped for x in ids[first[d] + seg_ids[d]:first[d] + lens[d]]]
        seen["junk_behind_stop"] += int(any(x not in tok for x in behind))
        consumed = [int(x) for d in range(n) for x in ids[first[d]:first[d] + seg_ids[d]]]
        seen["negative_skipped"] += int(any(x < 0 for x in consumed))
        seen["listed_above_max_id"] += int(any(x > max(tok) for x in consumed))
        seen["row_len_zero"] += int(rows and (lens == 0).any())
        seen["row_len_stride"] += int(rows and n > 0 and (lens == kw["row_stride"]).any())
        seen["skipped_and_stop"] += int(any(x in kw["stop"] and x in kw["skip"] for x in consumed))
        seen["lead"] += int(not rows and kw["tok_offsets"][0] > 0)
        seen["tail"] += int(not rows and kw["tok_offsets"][-1] < len(ids))
    assert all(v >= 50 for k, v in seen.items() if k != "error") and seen["error"] >= 10, seen


def _llama4_tok():
    pat, mr, special = H.llama4()
    tok = {r: b for b, r in mr.items()}
    tok.update({i: s.encode("utf-8") for s, i in special.items()})
    return tok, sorted(special.values())


def test_round_trip_on_the_golden_fixture(golden):
    tok, _ = _llama4_tok()
    ids, offs = golden["enc"].astype(np.int32), golden["enc_offsets"].astype(np.int64)
    out, o, seg_ids, info = dt.decode_numpy(ids, dt.Vocab(tok), tok_offsets=offs)
    assert out == golden["text"].tobytes() and np.array_equal(o, golden["offsets"].astype(np.int64))
    assert np.array_equal(seg_ids, np.diff(offs)) and info.tolist() == [len(out), len(ids), 0, 0]
    part = slice(0, int(offs[40]))
    _same(dt.decode_brute(ids[part], tok, tok_offsets=offs[:41]), dt.decode_numpy(ids[part], dt.Vocab(tok), tok_offsets=offs[:41]))


def test_the_compiled_references_decode_cases(golden):
    tok, _ = _llama4_tok()
    vocab = dt.Vocab(tok)
    assert len(golden["decode_ids"]) == 5
    for ids, exp in zip(golden["decode_ids"], golden["decode_bytes"]):
        ids = np.asarray(ids, dtype=np.int32)
        o = np.asarray([0, len(ids)], dtype=np.int64)
        assert dt.decode_brute(ids, tok, tok_offsets=o)[0] == exp == dt.decode_numpy(ids, vocab, tok_offsets=o)[0]


# ---- the model ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    src = ROOT / "tests" / "twin" / "decode_rows_model.cpp"
    out = ROOT / "tests" / "twin" / "_build" / "libdecoderowsmodel.so"
    out.parent.mkdir(parents=True, exist_ok=True)
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))  # (the shared header takes __host__ __device__ from HIP's host header)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__",
                           f"-I{rocm / 'include'}", str(src), "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.decode_rows_model.restype = i32
    lib.decode_rows_model.argtypes = [vp, i64, vp, vp, i64, i64, vp, i32, vp, vp, i64, i32, vp, vp, i64, vp, i64, vp, vp, vp, vp]
    lib.decode_rows_model_op.restype = None
    lib.decode_rows_model_op.argtypes = [i64, vp, vp, vp]
    lib.decode_rows_model_const.restype = i64
    lib.decode_rows_model_const.argtypes = [i32]
    return lib


def run_model(lib, ids, tok, tile, tok_offsets=None, row_stride=0, lengths=None, n_segs=None, skip=(), stop=(), keep_stop=False,
              skip_negative=False, skip_special=False, special_ids=(), capacity=None):
    """-> (bytes, out_offsets, seg_ids, info, (err, err_pos)).  The listed ids are merged as the host library merges them."""
    vocab = dt.Vocab(tok)
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    o = None if row_stride else np.ascontiguousarray(tok_offsets, dtype=np.int64)
    ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
    n = len(o) - 1 if o is not None else (len(ln) if ln is not None else n_segs)
    bits = {}
    for x in skip:
        bits[int(x)] = bits.get(int(x), 0) | 1
    for x in stop:
        bits[int(x)] = bits.get(int(x), 0) | (2 if keep_stop else 3)
    if skip_special:
        for x in special_ids:
            bits[int(x)] = bits.get(int(x), 0) | 1
    listed = np.asarray(sorted(bits), dtype=np.int32)
    lbits = np.asarray([bits[int(x)] for x in listed], dtype=np.uint8)
    lens = np.ascontiguousarray(vocab.lens, dtype=np.uint32)
    src_off = np.ascontiguousarray(vocab.begin, dtype=np.uint32)
    blob = np.ascontiguousarray(vocab.blob) if len(vocab.blob) else np.zeros(1, dtype=np.uint8)
    cap = int(8 * len(ids) + 64) if capacity is None else capacity
    out = np.full(cap + 32, 0xEE, dtype=np.uint8)
    offs, seg, info, pos = np.full(n + 1, -1, dtype=np.int64), np.full(max(n, 1), -1, dtype=np.int64), np.zeros(4, dtype=np.int64), np.zeros(1, dtype=np.int64)
    err = lib.decode_rows_model(ids.ctypes.data, len(ids), None if o is None else o.ctypes.data, None if ln is None else ln.ctypes.data, n,
                                row_stride, lens.ctypes.data, vocab.max_id, listed.ctypes.data, lbits.ctypes.data, len(listed),
                                int(skip_negative), src_off.ctypes.data, blob.ctypes.data, tile, out.ctypes.data, cap, offs.ctypes.data,
                                seg.ctypes.data, info.ctypes.data, pos.ctypes.data)
    assert (out[cap:] == 0xEE).all()
    return out[:max(int(info[0]), 0)].tobytes() if not err else b"", offs, seg[:n], info, (err, int(pos[0]))


def test_operator_is_associative(model):
    rng = np.random.default_rng(5)
    n = 10000

    def aggs():
        f = rng.integers(0, 2, size=n)
        return np.ascontiguousarray(np.stack([rng.integers(0, 1000, size=n), f * rng.integers(0, 1000, size=n), f, rng.integers(0, 2, size=n)], axis=1).astype(np.int64))

    def op(x, y):
        r = np.zeros_like(x)
        model.decode_rows_model_op(n, x.ctypes.data, y.ctypes.data, r.ctypes.data)
        return r

    x, y, z = aggs(), aggs(), aggs()
    assert np.array_equal(op(op(x, y), z), op(x, op(y, z)))
    e = np.zeros_like(x)
    assert np.array_equal(op(e, x), x) and np.array_equal(op(x, e), x)
    assert not np.array_equal(op(x, y), op(y, x))  # (the order matters: a scan, not a sum)


def test_model_constants_match_the_kernels(model):
    common = (ROOT / "tokendagger_amd" / "csrc" / "td_rows_common.h").read_text()
    assert "constexpr int RC_TILE = 4096;" in common and model.decode_rows_model_const(0) == 4096
    assert "constexpr int RC_THREADS = 256;" in common and model.decode_rows_model_const(1) == 256
    assert model.decode_rows_model_const(2) >= 4 * (4096 + 1)  # the byte prefixes of a tile share the window's LDS


@pytest.mark.parametrize("tile", [4, 16, 4096])
def test_model_matches_truth_on_random_cases(model, tile):
    rng = np.random.default_rng(29)
    errors = 0
    for it in range(200):
        c = dt.random_case(rng)
        want = _both(c)
        got = run_model(model, c["ids"], c["tok"], tile, **c["kw"])
        if isinstance(want, dt.DecodeError):
            errors += 1
            assert got[4] == (want.code, want.pos), (it, got[4], want)
            continue
        assert got[4][0] == 0, (it, got[4])
        _same(got[:4], want, it)
    assert errors >= 5


@pytest.mark.parametrize("tile", [4, 16])
def test_model_capacity_and_stop_across_tiles(model, tile):
    tok = {i: bytes([97 + i]) * (i + 1) for i in range(8)}
    ids = np.asarray([1, 2, 3, 7, 100, -5, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 100, 2, 2], dtype=np.int32)
    kw = dict(tok_offsets=np.asarray([0, 19, 19, 21], dtype=np.int64), stop=[7])
    want = dt.decode_brute(ids, tok, **kw)
    assert want[2].tolist() == [4, 0, 2] and want[3].tolist() == [len(want[0]), 5, 1, 1]
    _same(run_model(model, ids, tok, tile, **kw)[:4], want)
    short = run_model(model, ids, tok, tile, capacity=len(want[0]) - 1, **kw)
    assert short[4] == (capi.TD_E_CAPACITY, len(want[0])) and all(np.array_equal(x, y) for x, y in zip(short[1:4], want[1:]))


# ---- td_decode_rows_check through the C ABI -----------------------------------------------------------------------------------

def test_check_accepts_what_the_contract_allows():
    decode_rows_check(decode_spec(), 10, tok_offsets=[2, 2, 5, 9])
    decode_rows_check(decode_spec(), 0, tok_offsets=[0])
    decode_rows_check(decode_spec(3), 9, lengths=[0, 3, 2])
    decode_rows_check(decode_spec(3, skip=[5, 5, 10**9], stop=[5], keep_stop=True, skip_negative=True, skip_special=True), 9, n_segs=3)
    decode_rows_check(decode_spec(7), 0, n_segs=0)


def test_check_argument_errors_and_positions():
    def bad(pos, spec, n_tokens, **kw):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            decode_rows_check(spec, n_tokens, **kw)
        assert e.value.code == capi.TD_E_INVALID and e.value.pos == pos, (e.value.pos, pos, kw)

    bad(-1, None, 4, tok_offsets=[0, 4])
    bad(-1, decode_spec(flags=8), 4, tok_offsets=[0, 4])
    bad(-1, decode_spec(), -1, tok_offsets=[0, 0])
    bad(-1, decode_spec(), 4, n_segs=-1, tok_offsets=[0, 4])
    bad(-1, decode_spec(-2), 4, n_segs=1)
    bad(-1, decode_spec(), 4, n_segs=1)                      # the offsets form without offsets
    bad(0, decode_spec(), 4, tok_offsets=[-1, 4])
    bad(1, decode_spec(), 9, tok_offsets=[0, 5, 4, 9])       # decreasing at segment 1
    bad(3, decode_spec(), 8, tok_offsets=[0, 5, 5, 9])       # the end above n_tokens
    bad(-1, decode_spec(5), 14, n_segs=3)                    # 3 rows of 5 in 14 ids
    bad(-1, decode_spec(2**40), 2**62, n_segs=2**40)         # (no overflow in the product)
    bad(2, decode_spec(5), 15, lengths=[0, 5, 6])
    bad(0, decode_spec(5), 15, lengths=[-1, 5, 6])
    bad(1, decode_spec(skip=[3, -4]), 4, tok_offsets=[0, 4])
    bad(2, decode_spec(skip=[3, 4], stop=[-1]), 4, tok_offsets=[0, 4])
    lib = capi.load_library()
    spec = DecodeSpec(0, None, 2, None, 0, 0)                # a list with entries and no ids
    o = np.asarray([0, 4], dtype=np.int64)
    assert lib.td_decode_rows_check(ctypes.byref(spec), 4, o.ctypes.data, None, 1, None) == capi.TD_E_INVALID
    spec = DecodeSpec(0, None, 0, None, -1, 0)
    assert lib.td_decode_rows_check(ctypes.byref(spec), 4, o.ctypes.data, None, 1, None) == capi.TD_E_INVALID
    assert lib.td_decode_rows_check(ctypes.byref(decode_spec()), 4, o.ctypes.data, None, 1, None) == capi.TD_OK
