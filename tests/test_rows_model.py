"""Training rows on the CPU: hand-worked cases of the contract, the vectorised truth and the kernels' closed forms (base_d, c_d)
against the brute-force truth, and the C ABI's argument checks (no device needed for those)."""
import ctypes

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

import rows_truth as rt

BOS, EOS, PAD = 100, 101, -7


def _docs(lengths, first=1):
    ids, offs, v = [], [0], first
    for n in lengths:
        ids += list(range(v, v + n))
        v += n
        offs.append(len(ids))
    return np.array(ids, np.int32), np.array(offs, np.int64)


# L = [3, 0, 5], S = 4: ids 1 2 3 | (empty) | 4 5 6 7 8
IDS, OFFS = _docs([3, 0, 5])
HAND = {
    # (bos, eos, drop_last): (rows, positions, cu_seqlens).  Without BOS / EOS the second document starts at slot 3 and the row
    # start 4 cuts it again: positions restart at both.
    (-1, -1, False): ([[1, 2, 3, 4], [5, 6, 7, 8]], [[0, 1, 2, 0], [0, 1, 2, 3]], [0, 3, 4, 8]),
    (BOS, -1, False): ([[BOS, 1, 2, 3], [BOS, BOS, 4, 5], [6, 7, 8, PAD]], [[0, 1, 2, 3], [0, 0, 1, 2], [0, 1, 2, 0]],
                       [0, 4, 5, 8, 11]),
    (-1, EOS, False): ([[1, 2, 3, EOS], [EOS, 4, 5, 6], [7, 8, EOS, PAD]], [[0, 1, 2, 3], [0, 0, 1, 2], [0, 1, 2, 0]],
                       [0, 4, 5, 8, 11]),
    (BOS, EOS, False): ([[BOS, 1, 2, 3], [EOS, BOS, EOS, BOS], [4, 5, 6, 7], [8, EOS, PAD, PAD]],
                        [[0, 1, 2, 3], [0, 0, 1, 0], [0, 1, 2, 3], [0, 1, 0, 0]], [0, 4, 5, 7, 8, 12, 14]),
    (BOS, EOS, True): ([[BOS, 1, 2, 3], [EOS, BOS, EOS, BOS], [4, 5, 6, 7]],
                       [[0, 1, 2, 3], [0, 0, 1, 0], [0, 1, 2, 3]], [0, 4, 5, 7, 8, 12]),
    (-1, -1, True): ([[1, 2, 3, 4], [5, 6, 7, 8]], [[0, 1, 2, 0], [0, 1, 2, 3]], [0, 3, 4, 8]),
}


@pytest.mark.parametrize("key", sorted(HAND, key=str))
def test_concat_hand_worked(key):
    bos, eos, drop = key
    rows, pos, cu = HAND[key]
    for f in (rt.rows_brute, rt.rows_numpy):
        r_ids, r_pos, r_cu, counts = f(IDS, OFFS, 4, rt.CONCAT, bos, eos, PAD, drop)
        assert r_ids.tolist() == rows, f.__name__
        assert r_pos.tolist() == pos, f.__name__
        assert r_cu.tolist() == cu, f.__name__
        assert counts[0] == len(rows) and counts[2] == len(cu) - 1 and counts[1] == cu[-1]
        assert not np.any(np.diff(r_cu) == 0), "a zero-length segment"


def test_pad_hand_worked():
    r_ids, r_pos, lens, counts = rt.rows_brute(IDS, OFFS, 4, rt.PAD, BOS, EOS, PAD)
    assert r_ids.tolist() == [[BOS, 1, 2, EOS], [BOS, EOS, PAD, PAD], [BOS, 4, 5, EOS]]
    assert r_pos.tolist() == [[0, 1, 2, 3], [0, 1, 0, 0], [0, 1, 2, 3]]
    assert lens.tolist() == [4, 2, 4]
    assert counts.tolist() == [3, 10, 3, 2]
    r_ids, _, lens, counts = rt.rows_brute(IDS, OFFS, 4, rt.PAD, -1, -1, PAD)
    assert r_ids.tolist() == [[1, 2, 3, PAD], [PAD] * 4, [4, 5, 6, 7]]
    assert lens.tolist() == [3, 0, 4] and counts.tolist() == [3, 7, 2, 1]


def test_empty_documents_add_no_segment():
    ids, offs = _docs([2, 0, 0, 2, 0])
    _, pos, cu, counts = rt.rows_brute(ids, offs, 3, rt.CONCAT)
    assert cu.tolist() == [0, 2, 3, 4]  # (document 3 starts at 2; the row start 3 cuts it)
    assert pos.tolist() == [[0, 1, 0], [0, 0, 0]]
    assert counts.tolist() == [2, 4, 3, 0]
    # a document that starts exactly at a row start gives one boundary
    ids, offs = _docs([3, 3])
    _, _, cu, _ = rt.rows_brute(ids, offs, 3, rt.CONCAT)
    assert cu.tolist() == [0, 3, 6]


def test_no_documents_and_short_stream():
    z = np.zeros(0, np.int32)
    for f in (rt.rows_brute, rt.rows_numpy):
        r = f(z, np.zeros(1, np.int64), 8, rt.CONCAT, BOS, EOS)
        assert r[0].shape == (0, 8) and r[2].tolist() == [0] and r[3].tolist() == [0, 0, 0, 0]
        ids, offs = _docs([3])
        r = f(ids, offs, 8, rt.CONCAT, BOS, EOS, PAD, True)  # T = 5 < S with drop_last: no rows
        assert r[0].shape == (0, 8) and r[2].tolist() == [0] and r[3].tolist() == [0, 0, 0, 0]


specs = st.tuples(st.lists(st.integers(0, 12), min_size=0, max_size=12), st.integers(1, 9), st.sampled_from([-1, BOS]),
                  st.sampled_from([-1, EOS]), st.booleans())


@settings(max_examples=300, deadline=None)
@given(specs)
def test_numpy_truth_matches_brute_force(case):
    lengths, S, bos, eos, drop = case
    ids, offs = _docs(lengths)
    for layout in (rt.CONCAT, rt.PAD):
        if layout == rt.PAD and (drop or S < (bos >= 0) + (eos >= 0)):
            continue
        want = rt.rows_brute(ids, offs, S, layout, bos, eos, PAD, drop)
        got = rt.rows_numpy(ids, offs, S, layout, bos, eos, PAD, drop)
        for w, g in zip(want, got):
            assert np.array_equal(w, g), (layout, case)


@settings(max_examples=300, deadline=None)
@given(specs)
def test_closed_forms_match_brute_force(case):
    """base_d places every document without a scan; the exclusive scan of c_d indexes cu_seqlens, and its total is n_seg."""
    lengths, S, bos, eos, drop = case
    ids, offs = _docs(lengths)
    b, e = bos >= 0, eos >= 0
    stream_starts, pos = [], 0
    for n in lengths:
        stream_starts.append(pos)
        pos += b + n + e
    base = rt.doc_base(offs, b, e)
    assert base[:-1].tolist() == stream_starts and base[-1] == pos
    _, _, cu, counts = rt.rows_brute(ids, offs, S, rt.CONCAT, bos, eos, PAD, drop)
    R = int(counts[1])
    c = rt.doc_cuts(offs, S, b, e, R)
    assert int(c.sum()) == len(cu) - 1
    excl = np.concatenate([[0], np.cumsum(c)])[:-1]
    entries = []
    for d in range(len(lengths)):
        for m in range(int(c[d])):
            entries.append(int(base[d]) if m == 0 else (int(base[d]) // S + m) * S)
    assert entries + [R] == cu.tolist()
    for d in range(len(lengths)):
        if c[d]:
            assert cu[excl[d]] == base[d]


# ---- the C ABI's argument checks: no device, no handle ------------------------------------------------------------------
def _lib():
    from tokendagger_amd import capi
    return capi, capi.load_library()


def test_rows_abi_rejects_null_handle_and_bad_specs():
    capi, lib = _lib()
    ids = np.arange(8, dtype=np.int32)
    offs = np.array([0, 3, 8], np.int64)
    out = np.zeros(64, np.int32)
    counts = np.zeros(4, np.int64)
    bad = [capi.rows_spec(0), capi.rows_spec(-3), capi.RowsSpec(2, 4, -1, -1, 0, 0), capi.RowsSpec(0, 4, -1, -1, 0, 2),
           capi.rows_spec(1, capi.TD_ROWS_PAD, 5, 6), capi.rows_spec(8, capi.TD_ROWS_PAD, drop_last=True), capi.rows_spec(4, pad=1 << 40)]
    for sp in [capi.rows_spec(4)] + bad:
        assert lib.td_make_rows(None, ids.ctypes.data, 8, offs.ctypes.data, 2, ctypes.byref(sp), out.ctypes.data, 16, None, None,
                                counts.ctypes.data) == capi.TD_E_INVALID
        assert lib.td_make_rows_device(None, ids.ctypes.data, 8, offs.ctypes.data, 2, ctypes.byref(sp), out.ctypes.data, 16, None, None,
                                       counts.ctypes.data, None) == capi.TD_E_INVALID
        assert lib.td_encode_batch_rows(None, b"abc", offs.ctypes.data, 1, 0, ctypes.byref(sp), out.ctypes.data, 16, None, None,
                                        counts.ctypes.data) == capi.TD_E_INVALID
    assert lib.td_make_rows(None, None, 0, None, 0, None, None, 0, None, None, None) == capi.TD_E_INVALID
    assert counts.tolist() == [0, 0, 0, 0] and not out.any()


def test_rows_entry_points_in_header_and_exports():
    capi, lib = _lib()
    for name in ("td_make_rows", "td_make_rows_device", "td_encode_batch_rows"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert capi.rows_capacity_of(capi.rows_spec(4, bos=1, eos=2), 8, 3) == 4
    assert capi.rows_capacity_of(capi.rows_spec(4, bos=1, eos=2, drop_last=True), 8, 3) == 3
    assert capi.rows_capacity_of(capi.rows_spec(4, capi.TD_ROWS_PAD), 8, 3) == 3
