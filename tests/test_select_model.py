"""Document selection on the CPU: a hand-worked example of the contract (include/tokendagger_hip.h, td_select_spec), the loop truth
against the vectorised one, td_select_plan (host only) against both, the properties of a selection, and the C ABI's argument
checks (no device needed for those)."""
import ctypes

import numpy as np
import pytest

import select_truth as st


def _capi():
    from tokendagger_amd import capi
    capi.load_library()
    return capi


def _cases(n=300, seed=11):
    rng = np.random.default_rng(seed)
    return [st.random_case(rng) for _ in range(n)]


def _same(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and np.array_equal(x, y)


def test_hand_worked_example():
    # Lengths [3, 0, 5, 1, 0, 4]; ids 1 .. 13 in document order, labels = -ids.
    #   document 0: 1 2 3    1: -    2: 4 5 6 7 8    3: 9    4: -    5: 10 11 12 13
    offs = np.array([0, 3, 3, 8, 9, 9, 13], np.int64)
    ids = np.arange(1, 14, dtype=np.int32)
    sel = [5, 1, 1, 2, 0, 4, 2]  # their lengths: 4 0 0 5 3 0 5
    capi = _capi()
    for f in (st.select_brute, st.select_numpy):
        o_ids, o_lab, o_offs, o_docs, counts = f(ids, offs, sel, 0, -1, labels=-ids)
        assert o_ids.tolist() == [10, 11, 12, 13, 4, 5, 6, 7, 8, 1, 2, 3, 4, 5, 6, 7, 8], f.__name__
        assert o_lab.tolist() == [-x for x in o_ids.tolist()]
        assert o_offs.tolist() == [0, 4, 4, 4, 9, 12, 12, 17]  # (the empty documents keep their places)
        assert o_docs.tolist() == sel
        assert counts.tolist() == [7, 17, 0, 0]
        # min_len = 1 drops the three empty entries (1, 1, 4), max_len = 4 the two of document 2 (5 ids): 5 and 0 stay.
        # K + short + long = 2 + 3 + 2 = 7 = n_sel, T = 4 + 3.
        o_ids, _, o_offs, o_docs, counts = f(ids, offs, sel, 1, 4)
        assert o_ids.tolist() == [10, 11, 12, 13, 1, 2, 3]
        assert o_offs.tolist() == [0, 4, 7] and o_docs.tolist() == [5, 0]
        assert counts.tolist() == [2, 7, 3, 2]
    counts, p_offs, p_docs = capi.select_plan(offs, sel, capi.select_spec(0))
    assert counts.tolist() == [7, 17, 0, 0] and p_offs.tolist() == [0, 4, 4, 4, 9, 12, 12, 17] and p_docs.tolist() == sel
    counts, p_offs, p_docs = capi.select_plan(offs, sel, capi.select_spec(1, 4))
    assert counts.tolist() == [2, 7, 3, 2] and p_offs.tolist() == [0, 4, 7] and p_docs.tolist() == [5, 0]


def test_brute_equals_numpy():
    seen = set()
    for ids, labels, offs, sel, mn, mx in _cases():
        b = st.select_brute(ids, offs, sel, mn, mx, labels=labels)
        _same(b, st.select_numpy(ids, offs, sel, mn, mx, labels=labels))
        _same(st.select_brute(ids, offs, sel, mn, mx), st.select_numpy(ids, offs, sel, mn, mx))
        n_sel = len(offs) - 1 if sel is None else len(sel)
        assert b[4][0] + b[4][2] + b[4][3] == n_sel
        seen |= {("identity", sel is None), ("no limit", mx == -1), ("equal", mx == mn), ("short", b[4][2] > 0), ("long", b[4][3] > 0),
                 ("repeats", sel is not None and len(set(sel.tolist())) < len(sel)), ("more", n_sel > len(offs) - 1)}
    for what in ("identity", "no limit", "equal", "short", "long", "repeats", "more"):
        assert (what, True) in seen, what


def test_plan_equals_truths():
    capi = _capi()
    for ids, labels, offs, sel, mn, mx in _cases():
        _, _, t_offs, t_docs, t_counts = st.select_numpy(ids, offs, sel, mn, mx)
        counts, p_offs, p_docs = capi.select_plan(offs, sel, capi.select_spec(mn, mx))
        assert np.array_equal(counts, t_counts) and np.array_equal(p_offs, t_offs) and np.array_equal(p_docs, t_docs)
        assert np.array_equal(capi.select_plan(offs, sel, capi.select_spec(mn, mx), outputs=False), t_counts)
        assert np.array_equal(st.select_brute(ids, offs, sel, mn, mx)[4], counts)


def test_properties():
    rng = np.random.default_rng(3)
    for ids, labels, offs, _, _, _ in _cases(60, seed=4):
        n_docs = len(offs) - 1
        # the identity with no limits returns the input
        o_ids, o_lab, o_offs, o_docs, counts = st.select_numpy(ids, offs, None, 0, -1, labels=labels)
        assert np.array_equal(o_ids, ids) and np.array_equal(o_lab, labels) and np.array_equal(o_offs, offs)
        assert np.array_equal(o_docs, np.arange(n_docs)) and counts.tolist() == [n_docs, len(ids), 0, 0]
        # p, then the inverse of p
        p = rng.permutation(n_docs).astype(np.int64)
        inv = np.empty_like(p)
        inv[p] = np.arange(n_docs)
        a = st.select_numpy(ids, offs, p)
        b = st.select_numpy(a[0], a[2], inv)
        assert np.array_equal(b[0], ids) and np.array_equal(b[2], offs)
        assert np.array_equal(p[b[3]], np.arange(n_docs))


def _plan_rc(capi, offs, sel, n_sel, spec, counts=True, n_docs=None):
    lib = capi.load_library()
    o = np.ascontiguousarray(offs, np.int64)
    s = None if sel is None else np.ascontiguousarray(sel, np.int64)
    c = np.full(4, 55, np.int64)
    out_o, out_d = np.full(n_sel + 2, 77, np.int64), np.full(n_sel + 2, 77, np.int64)
    rc = lib.td_select_plan(o.ctypes.data, len(o) - 1 if n_docs is None else n_docs, s.ctypes.data if s is not None else None, n_sel,
                            ctypes.byref(spec) if spec is not None else None, c.ctypes.data if counts else None, out_o.ctypes.data,
                            out_d.ctypes.data)
    assert rc == capi.TD_OK or ((out_o == 77).all() and (out_d == 77).all())  # an error writes no output
    return rc, c


def test_argument_checks_without_a_device():
    capi = _capi()
    offs = np.array([0, 3, 3, 8, 9, 9, 13], np.int64)
    sel = np.array([5, 1, 1, 2, 0, 4, 2], np.int64)
    assert _plan_rc(capi, offs, sel, 7, capi.select_spec(0))[0] == capi.TD_OK
    for bad in (capi.select_spec(-1), capi.select_spec(0, -2), capi.select_spec(3, 2), capi.select_spec(0, flags=1), None):
        rc, c = _plan_rc(capi, offs, sel, 7, bad)
        assert rc == capi.TD_E_INVALID and c[0] == -1
    assert _plan_rc(capi, offs, sel, 7, capi.select_spec(2, 2))[0] == capi.TD_OK       # min_len == max_len
    assert _plan_rc(capi, offs, sel, 7, capi.select_spec(5, None))[0] == capi.TD_OK    # -1: no limit, whatever min_len
    # the identity needs n_sel == n_docs
    assert _plan_rc(capi, offs, None, 6, capi.select_spec())[0] == capi.TD_OK
    for n in (5, 7, 0):
        rc, c = _plan_rc(capi, offs, None, n, capi.select_spec())
        assert rc == capi.TD_E_INVALID and c[0] == -1
    assert _plan_rc(capi, offs, sel, 7, capi.select_spec(), counts=False)[0] == capi.TD_E_INVALID
    assert _plan_rc(capi, offs, sel, -1, capi.select_spec())[0] == capi.TD_E_INVALID
    assert _plan_rc(capi, offs, sel, 7, capi.select_spec(), n_docs=-1)[0] == capi.TD_E_INVALID
    # an entry out of range, with its position
    for pos, v in ((0, 6), (3, -1), (6, 6), (2, 1 << 40)):
        s = sel.copy()
        s[pos] = v
        rc, c = _plan_rc(capi, offs, s, 7, capi.select_spec())
        assert rc == capi.TD_E_INVALID and c[0] == pos
        with pytest.raises(capi.TokenDaggerHipError) as ei:
            capi.select_plan(offs, s)
        assert ei.value.code == capi.TD_E_INVALID and ei.value.counts[0] == pos
    # decreasing offsets count where the document is listed, and only there
    dec = offs.copy()
    dec[3], dec[4] = offs[4], offs[3]  # documents 2 (fine: 3 .. 9), 3 (9 .. 8: decreasing) and 4 (8 .. 9)
    rc, c = _plan_rc(capi, dec, np.array([0, 2, 3, 1], np.int64), 4, capi.select_spec())
    assert rc == capi.TD_E_INVALID and c[0] == 2
    rc, c = _plan_rc(capi, dec, np.array([0, 2, 4, 1], np.int64), 4, capi.select_spec())
    assert rc == capi.TD_OK and c.tolist() == [4, 3 + 6 + 1 + 0, 0, 0]
    # nothing selected from nothing
    rc, c = _plan_rc(capi, np.zeros(1, np.int64), None, 0, capi.select_spec())
    assert rc == capi.TD_OK and c.tolist() == [0, 0, 0, 0]
    rc, c = _plan_rc(capi, np.zeros(1, np.int64), np.zeros(1, np.int64), 1, capi.select_spec())
    assert rc == capi.TD_E_INVALID and c[0] == 0
