"""Best-fit-decreasing rows on the CPU: the hand-worked example of the contract (include/tokendagger_hip.h, TD_ROWS_BESTFIT), the
run-form truth against the item-by-item one, td_pack_plan (host only) against both, the capacity bound, and the C ABI's argument
checks (no device needed for those)."""
import ctypes

import numpy as np
import pytest

import pack_truth as pt

BOS, EOS, PAD = 100, 101, -7


def _docs(lengths, first=1):
    ids, offs, v = [], [0], first
    for n in lengths:
        ids += list(range(v, v + n))
        v += n
        offs.append(len(ids))
    return np.array(ids, np.int32), np.array(offs, np.int64)


def _lib():
    from tokendagger_amd import capi
    return capi, capi.load_library()


# S = 8, no BOS / EOS, split: document lengths [3, 6, 2, 10, 5, 0, 2] (ids 1 .. 28 in document order)
HAND_L = [3, 6, 2, 10, 5, 0, 2]


def test_hand_worked_example():
    ids, offs = _docs(HAND_L)
    d = {k: list(range(int(offs[k]) + 1, int(offs[k + 1]) + 1)) for k in range(len(HAND_L))}
    rows = [d[3][:8], d[1] + d[2], d[4] + d[0], d[3][8:] + d[6] + [PAD] * 4]
    for f in (pt.pack_brute, pt.pack_runs):
        r_ids, r_pos, cu, lens, docs, counts = f(ids, offs, 8, pad=PAD)
        assert r_ids.tolist() == rows, f.__name__
        assert cu.tolist() == [0, 8, 14, 16, 21, 24, 26, 28, 32]
        assert docs.tolist() == [3, 1, 2, 4, 0, 3, 6, -1]
        assert lens.tolist() == [8, 8, 8, 4]
        assert counts.tolist() == [4, 28, 8, 1]
        assert r_pos.tolist() == [list(range(8)), list(range(6)) + [0, 1], list(range(5)) + [0, 1, 2], [0, 1, 0, 1, 0, 0, 0, 0]]
    capi, _ = _lib()
    c, row, slot = capi.pack_plan(offs, capi.pack_spec(8), placement=True)
    assert c.tolist() == [4, 28, 8, 1]
    assert row.tolist() == [2, 1, 1, 3, 2, -1, 3] and slot.tolist() == [5, 0, 6, 0, 0, -1, 2]


def test_hand_worked_truncate_and_frames():
    capi, _ = _lib()
    ids, offs = _docs(HAND_L)
    d = {k: list(range(int(offs[k]) + 1, int(offs[k + 1]) + 1)) for k in range(len(HAND_L))}
    # truncate, no BOS / EOS: d3 keeps 8 ids and is a full row; nothing else changes but d3's remainder is gone
    r = pt.pack_brute(ids, offs, 8, pad=PAD, truncate=True)
    assert r[0].tolist() == [d[3][:8], d[1] + d[2], d[4] + d[0], d[6] + [PAD] * 6]
    assert r[2].tolist() == [0, 8, 14, 16, 21, 24, 26, 32] and r[4].tolist() == [3, 1, 2, 4, 0, 6, -1]
    assert r[5].tolist() == [4, 26, 7, 1]
    # BOS + EOS, split: n = [5, 8, 4, 12, 7, 2, 4] -> items 8 (d1), 8 (d3 chunk 0), 7 (d4), 5 (d0), 4 (d2), 4 (d3 rest), 4 (d6), 2 (d5)
    r = pt.pack_brute(ids, offs, 8, BOS, EOS, PAD)
    B, E = [BOS], [EOS]
    # (worked by hand: rows 0 and 1 are the full chunks; d4 (7), d0 (5) and d2 (4) open rows 2, 3 and 4; d3's rest (4) fills row 4;
    #  d6 (4) opens row 5; d5 (2) goes to row 3, whose free 3 is the smallest >= 2)
    want = [B + d[1] + E, B + d[3][:7], B + d[4] + E + [PAD], B + d[0] + E + [BOS, EOS, PAD], B + d[2] + E + d[3][7:] + E, B + d[6] + E + [PAD] * 4]
    assert r[0].tolist() == want
    assert r[5].tolist() == [6, 42, 11, 1]
    assert r[1][4].tolist() == [0, 1, 2, 3, 0, 1, 2, 3]  # (d3's second chunk restarts at 0)
    for trunc in (False, True):
        for bos, eos in ((-1, -1), (BOS, -1), (-1, EOS), (BOS, EOS)):
            a = pt.pack_brute(ids, offs, 8, bos, eos, PAD, trunc, placement=True)
            b = pt.pack_runs(ids, offs, 8, bos, eos, PAD, trunc, placement=True)
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
            for x, y in zip(capi.pack_plan(offs, capi.pack_spec(8, bos, eos, PAD, trunc), placement=True), a[5:]):
                assert np.array_equal(x, y)


def _random_case(rng):
    S = int(rng.choice([1, 2, 3, 5, 8, 16, 31, 64, 100]))
    n = int(rng.integers(0, 40))
    special = [0, 1, max(S - 1, 0), S, S + 1, 2 * S, 3 * S]
    pool = rng.integers(0, 3 * S + 2, 4)  # few distinct lengths: many equal ones
    L = np.where(rng.random(n) < 0.4, rng.choice(special, n), rng.choice(pool, n)).astype(np.int64)
    bos, eos = [(-1, -1), (BOS, -1), (-1, EOS), (BOS, EOS)][int(rng.integers(0, 4))]
    trunc = bool(rng.integers(0, 2))
    if trunc and S < (bos >= 0) + (eos >= 0):
        trunc = False
    return L, S, bos, eos, trunc


def test_runs_equal_brute_on_random_cases():
    capi, _ = _lib()
    rng = np.random.default_rng(11)
    for _ in range(3000):
        L, S, bos, eos, trunc = _random_case(rng)
        ids, offs = _docs(L.tolist())
        a = pt.pack_brute(ids, offs, S, bos, eos, PAD, trunc, placement=True)
        b = pt.pack_runs(ids, offs, S, bos, eos, PAD, trunc, placement=True)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), (L.tolist(), S, bos, eos, trunc)
        assert np.array_equal(capi.pack_plan(offs, capi.pack_spec(S, bos, eos, PAD, trunc)), a[5])


def _check_invariants(ids, offs, S, bos, eos, trunc, res):
    r_ids, r_pos, cu, lens, docs, counts = res[:6]
    b, e = int(bos >= 0), int(eos >= 0)
    L = np.diff(offs)
    rows = int(counts[0])
    assert rows <= pt.rows_bound(len(ids), len(L), S, bos, eos)
    assert cu[0] == 0 and cu[-1] == rows * S and np.all(np.diff(cu) > 0)
    assert int(lens.sum()) == counts[1] and len(docs) == counts[2] == len(cu) - 1
    flat = r_ids.reshape(-1)
    # every document's slots appear exactly once and in order: its segments, in order, concatenate to [BOS] body [EOS]
    for d in range(len(L)):
        body = ids[offs[d]:offs[d + 1]].tolist()
        if trunc:
            body = body[:S - b - e]
        want = ([bos] if b else []) + body + ([eos] if e else [])
        got = [flat[cu[k]:cu[k + 1]].tolist() for k in np.nonzero(docs == d)[0]]
        full = [g for g in got if len(g) == S]
        rest = [g for g in got if len(g) < S]
        assert sum(full + rest, []) == want, d  # (full chunks first in row order, then the remainder)


def test_invariants_and_bound():
    capi, _ = _lib()
    rng = np.random.default_rng(12)
    for _ in range(400):
        L, S, bos, eos, trunc = _random_case(rng)
        ids, offs = _docs(L.tolist())
        _check_invariants(ids, offs, S, bos, eos, trunc, pt.pack_runs(ids, offs, S, bos, eos, PAD, trunc))
        sp = capi.pack_spec(S, bos, eos, PAD, trunc)
        assert capi.pack_plan(offs, sp)[0] <= capi.pack_rows_capacity_of(sp, len(ids), len(L))


def test_pack_plan_equals_truth_on_random_cases():
    capi, _ = _lib()
    rng = np.random.default_rng(13)
    for _ in range(2000):
        L, S, bos, eos, trunc = _random_case(rng)
        ids, offs = _docs(L.tolist())
        t = pt.pack_runs(ids, offs, S, bos, eos, PAD, trunc, placement=True)
        c, row, slot = capi.pack_plan(offs, capi.pack_spec(S, bos, eos, PAD, trunc), placement=True)
        assert np.array_equal(c, t[5]) and np.array_equal(row, t[6]) and np.array_equal(slot, t[7]), (L.tolist(), S, bos, eos, trunc)
        assert np.array_equal(capi.pack_plan(offs, capi.pack_spec(S, bos, eos, PAD, trunc)), t[5])


@pytest.mark.parametrize("S", [7, 512, 2048, 8192])
def test_pack_plan_on_golden_offsets(golden, S):
    capi, _ = _lib()
    offs = np.asarray(golden["enc_offsets"], np.int64)
    ids = np.asarray(golden["enc"], np.int32)
    for bos, eos in ((-1, -1), (BOS, EOS)):
        for trunc in (False, True):
            t = pt.pack_runs(ids, offs, S, bos, eos, PAD, trunc, placement=True)
            c, row, slot = capi.pack_plan(offs, capi.pack_spec(S, bos, eos, PAD, trunc), placement=True)
            assert np.array_equal(c, t[5]) and np.array_equal(row, t[6]) and np.array_equal(slot, t[7])
            assert c[0] <= pt.rows_bound(len(ids), len(offs) - 1, S, bos, eos)
            assert c[0] <= capi.pack_rows_capacity_of(capi.pack_spec(S, bos, eos), len(ids), len(offs) - 1)
            if S == 2048 and bos >= 0 and not trunc:
                _check_invariants(ids, offs, S, bos, eos, trunc, t)
                assert c[1] / (c[0] * S) > 0.99  # (the issue's 99.94 % fill)
    if S == 512:  # the item-by-item truth on the golden fixture too (its linear scan over the rows is slow at small S)
        a = pt.pack_brute(ids, offs, S, BOS, EOS, PAD)
        b = pt.pack_runs(ids, offs, S, BOS, EOS, PAD)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_empty_inputs():
    capi, _ = _lib()
    z = np.zeros(0, np.int32)
    for f in (pt.pack_brute, pt.pack_runs):
        r = f(z, np.zeros(1, np.int64), 8, BOS, EOS)
        assert r[0].shape == (0, 8) and r[2].tolist() == [0] and r[5].tolist() == [0, 0, 0, 0]
        r = f(z, np.zeros(4, np.int64), 4)  # three empty documents, no BOS / EOS: no slots, no rows
        assert r[0].shape == (0, 4) and r[2].tolist() == [0] and r[4].tolist() == [] and r[5].tolist() == [0, 0, 0, 0]
    assert capi.pack_plan(np.zeros(1, np.int64), capi.pack_spec(8)).tolist() == [0, 0, 0, 0]
    c, row, slot = capi.pack_plan(np.zeros(4, np.int64), capi.pack_spec(4, BOS, EOS), placement=True)
    assert c.tolist() == [2, 6, 4, 0] and row.tolist() == [0, 0, 1] and slot.tolist() == [0, 2, 0]


def test_pack_plan_rejects_bad_specs_and_offsets():
    capi, lib = _lib()
    offs = np.array([0, 3, 8], np.int64)
    for sp in (capi.pack_spec(0), capi.rows_spec(8), capi.rows_spec(8, capi.TD_ROWS_PAD), capi.RowsSpec(2, 8, -1, -1, 0, 1),
               capi.RowsSpec(2, 8, -1, -1, 0, 4), capi.pack_spec(1, BOS, EOS, truncate=True), capi.pack_spec(8, pad=1 << 40)):
        with pytest.raises(capi.TokenDaggerHipError):
            capi.pack_plan(offs, sp)
    for bad in ([1, 3, 8], [0, 5, 3]):
        with pytest.raises(capi.TokenDaggerHipError):
            capi.pack_plan(np.array(bad, np.int64), capi.pack_spec(8))
    counts = np.zeros(4, np.int64)
    assert lib.td_pack_plan(None, 0, ctypes.byref(capi.pack_spec(8)), counts.ctypes.data, None, None) == capi.TD_E_INVALID
    # split allows S < b + e: S = 1 gives one full row per slot
    assert capi.pack_plan(offs, capi.pack_spec(1, BOS, EOS)).tolist() == [12, 12, 12, 2]


def test_pack_abi_rejects_null_handle_and_bad_specs():
    capi, lib = _lib()
    ids = np.arange(8, dtype=np.int32)
    offs = np.array([0, 3, 8], np.int64)
    out = np.zeros(64, np.int32)
    counts = np.zeros(4, np.int64)
    outs = capi.PackOutputs(out.ctypes.data, None, None, None, None)
    bad = [capi.pack_spec(0), capi.pack_spec(-3), capi.rows_spec(4), capi.rows_spec(4, capi.TD_ROWS_PAD), capi.RowsSpec(2, 4, -1, -1, 0, 1),
           capi.pack_spec(1, 5, 6, truncate=True), capi.pack_spec(4, pad=1 << 40)]
    for sp in [capi.pack_spec(4)] + bad:
        assert lib.td_pack_rows(None, ids.ctypes.data, 8, offs.ctypes.data, 2, ctypes.byref(sp), ctypes.byref(outs), 16,
                                counts.ctypes.data) == capi.TD_E_INVALID
        assert lib.td_pack_rows_device(None, ids.ctypes.data, 8, offs.ctypes.data, 2, ctypes.byref(sp), ctypes.byref(outs), 16,
                                       counts.ctypes.data, None) == capi.TD_E_INVALID
        assert lib.td_encode_batch_pack_rows(None, b"abc", offs.ctypes.data, 1, 0, ctypes.byref(sp), ctypes.byref(outs), 16,
                                             counts.ctypes.data) == capi.TD_E_INVALID
    assert lib.td_pack_rows(None, None, 0, None, 0, None, None, 0, None) == capi.TD_E_INVALID
    assert counts.tolist() == [0, 0, 0, 0] and not out.any()


def test_existing_rows_entry_points_still_reject_bestfit():
    capi, lib = _lib()
    ids = np.arange(8, dtype=np.int32)
    offs = np.array([0, 3, 8], np.int64)
    out = np.zeros(64, np.int32)
    counts = np.zeros(4, np.int64)
    for sp in (capi.pack_spec(4), capi.RowsSpec(0, 4, -1, -1, 0, capi.TD_ROWS_TRUNCATE)):
        assert lib.td_make_rows(None, ids.ctypes.data, 8, offs.ctypes.data, 2, ctypes.byref(sp), out.ctypes.data, 16, None, None,
                                counts.ctypes.data) == capi.TD_E_INVALID


def test_pack_entry_points_in_header_and_exports():
    capi, lib = _lib()
    for name in ("td_pack_plan", "td_pack_rows", "td_pack_rows_device", "td_encode_batch_pack_rows"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert capi.pack_rows_capacity_of(capi.pack_spec(4, bos=1, eos=2), 8, 3) == 2 * 14 // 4 + 1
    assert capi.TD_ROWS_BESTFIT == 2 and capi.TD_ROWS_TRUNCATE == 2
