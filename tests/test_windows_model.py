"""Overlapping window rows on the CPU: a hand-worked example of the contract (include/tokendagger_hip.h, TD_ROWS_WINDOWS), the
loop truth against the closed-form one, the coverage property, td_window_plan (host only) against both, and the C ABI's argument
checks (no device needed for those)."""
import ctypes

import numpy as np
import pytest

import windows_truth as wt

BOS, EOS, PAD = 100, 101, -7
FRAMES = [(-1, -1), (BOS, -1), (-1, EOS), (BOS, EOS)]


def _capi():
    from tokendagger_amd import capi
    capi.load_library()
    return capi


def _random_case(rng, max_len=40, max_docs=30, force_max_overlap=False):
    lengths = rng.integers(0, max_len + 1, rng.integers(0, max_docs))
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ids = rng.integers(0, 200000, int(offs[-1])).astype(np.int32)
    bos, eos = FRAMES[int(rng.integers(0, 4))]
    k = (bos >= 0) + (eos >= 0)
    S = int(rng.integers(1 + k, 21))
    C = S - k
    overlap = C - 1 if force_max_overlap else int(rng.integers(0, C))
    return ids, offs, S, overlap, bos, eos


def test_hand_worked_example():
    # S = 6 with BOS and EOS: C = 4, overlap 1, step 3.  Lengths [3, 9, 0, 4, 5]; ids 1 .. 21 in document order.
    offs = np.array([0, 3, 12, 12, 16, 21], np.int64)
    ids = np.arange(1, 22, dtype=np.int32)
    rows = [[BOS, 1, 2, 3, EOS, PAD],
            [BOS, 4, 5, 6, 7, EOS], [BOS, 7, 8, 9, 10, EOS], [BOS, 10, 11, 12, EOS, PAD],  # 9 ids: [0, 4) [3, 7) [6, 9)
            [BOS, EOS, PAD, PAD, PAD, PAD],
            [BOS, 13, 14, 15, 16, EOS],                                                    # L = C: one window
            [BOS, 17, 18, 19, 20, EOS], [BOS, 20, 21, EOS, PAD, PAD]]                      # L = C + 1: two
    for f in (wt.windows_brute, wt.windows_numpy):
        r_ids, r_pos, lens, docs, starts, counts = f(ids, offs, 6, 1, BOS, EOS, PAD)
        assert r_ids.tolist() == rows, f.__name__
        assert lens.tolist() == [5, 6, 6, 5, 2, 6, 6, 4]
        assert docs.tolist() == [0, 1, 1, 1, 2, 3, 4, 4]
        assert starts.tolist() == [0, 0, 3, 6, 0, 0, 0, 3]
        assert counts.tolist() == [8, 40, 2, 3]
        assert r_pos.tolist() == [list(range(n)) + [0] * (6 - n) for n in lens.tolist()]
    capi = _capi()
    c, first = capi.window_plan(offs, capi.windows_spec(6, BOS, EOS, PAD), 1, first_row=True)
    assert c.tolist() == [8, 40, 2, 3] and first.tolist() == [0, 1, 4, 5, 6, 8]


def test_brute_against_numpy():
    rng = np.random.default_rng(11)
    for it in range(300):
        ids, offs, S, overlap, bos, eos = _random_case(rng, force_max_overlap=it % 5 == 4)
        a = wt.windows_brute(ids, offs, S, overlap, bos, eos, PAD)
        b = wt.windows_numpy(ids, offs, S, overlap, bos, eos, PAD)
        for x, y in zip(a, b):
            assert x.shape == y.shape and np.array_equal(x, y), (S, overlap, bos, eos)


def test_coverage_property():
    """The union of a document's windows is the document; every later window repeats exactly `overlap` ids of the one before
    and brings at least one new id."""
    rng = np.random.default_rng(12)
    for it in range(300):
        ids, offs, S, overlap, bos, eos = _random_case(rng, force_max_overlap=it % 5 == 4)
        r_ids, _, lens, docs, starts, counts = wt.windows_numpy(ids, offs, S, overlap, bos, eos, PAD)
        b, e = int(bos >= 0), int(eos >= 0)
        assert len(np.unique(docs)) == len(offs) - 1 and np.all(np.diff(docs) >= 0)  # every document has a row, in order
        for d in range(len(offs) - 1):
            mine = np.flatnonzero(docs == d)
            doc = ids[offs[d]:offs[d + 1]]
            covered = 0
            for n, r in enumerate(mine):
                body = r_ids[r, b:lens[r] - e]
                lo = int(starts[r])
                assert np.array_equal(body, doc[lo:lo + len(body)])
                if n == 0:
                    assert lo == 0
                else:
                    assert covered - lo == overlap and lo + len(body) > covered
                covered = lo + len(body)
            assert covered == len(doc)


def test_window_plan_against_truth(golden):
    capi = _capi()
    rng = np.random.default_rng(13)
    cases = []
    for it in range(200):
        _, offs, S, overlap, bos, eos = _random_case(rng, max_len=200, max_docs=100, force_max_overlap=it % 5 == 4)
        cases.append((offs, S, overlap, bos, eos))
    g = golden["enc_offsets"]
    for S, overlap in ((1, 0), (7, 2), (128, 0), (128, 32), (512, 64), (2048, 128), (8192, 0)):
        for bos, eos in FRAMES:
            C = S - (bos >= 0) - (eos >= 0)
            if C >= 1 and overlap < C:
                cases.append((g, S, overlap, bos, eos))
    cases.append((np.zeros(1, np.int64), 8, 3, BOS, EOS))       # n_docs = 0
    cases.append((np.zeros(1001, np.int64), 8, 3, BOS, EOS))    # all documents empty
    cases.append((np.array([0, 5, 5, 6], np.int64), 1, 0, -1, -1))  # S = 1 without BOS / EOS
    cases.append((np.array([0, 50, 51, 300], np.int64), 9, 6, BOS, EOS))  # overlap = C - 1
    for offs, S, overlap, bos, eos in cases:
        w, first = wt.window_counts(offs, S, overlap, bos, eos)
        L = np.diff(np.asarray(offs, np.int64))
        k = int(bos >= 0) + int(eos >= 0)
        want = [int(first[-1]), int((w * k + L + (w - 1) * overlap).sum()), int((w > 1).sum()), int(w.max()) if len(w) else 0]
        c, fr = capi.window_plan(offs, capi.windows_spec(S, bos, eos, PAD), overlap, first_row=True)
        assert c.tolist() == want, (S, overlap, bos, eos)
        assert np.array_equal(fr, first)
        assert capi.window_plan(offs, capi.windows_spec(S, bos, eos, PAD), overlap).tolist() == want
    # the counts of the closed form are the counts of the walk
    for offs, S, overlap, bos, eos in cases[:200]:
        ids = np.zeros(int(offs[-1]), np.int32)
        t = wt.windows_brute(ids, offs, S, overlap, bos, eos, PAD)
        assert capi.window_plan(offs, capi.windows_spec(S, bos, eos, PAD), overlap).tolist() == t[5].tolist()


def test_golden_figures(golden):
    """The figures the GPU cases rest on: every (S, overlap) of the GPU test has split documents."""
    capi = _capi()
    g = golden["enc_offsets"]
    assert len(g) - 1 == 3335 and int(g[-1]) == 828407 and int(np.diff(g).max()) == 263300 and int((np.diff(g) == 0).sum()) == 1
    c = capi.window_plan(g, capi.windows_spec(1, -1, -1, PAD), 0)
    assert c.tolist() == [828408, 828407, int((np.diff(g) > 1).sum()), 263300]
    for S, overlap in ((7, 2), (128, 0), (128, 32), (512, 64), (2048, 128), (8192, 0)):
        c = capi.window_plan(g, capi.windows_spec(S, BOS, EOS, PAD), overlap)
        assert c[0] > 3335 and c[2] >= 7 and c[3] >= 2


def test_invalid_arguments():
    capi = _capi()
    lib = capi.load_library()
    offs = np.array([0, 3, 10], np.int64)
    counts = np.zeros(4, np.int64)

    def plan(spec, overlap, o=offs, n_docs=None, c=counts):
        return lib.td_window_plan(o.ctypes.data if o is not None else None, len(offs) - 1 if n_docs is None else n_docs,
                                  ctypes.byref(spec) if spec is not None else None, overlap, c.ctypes.data if c is not None else None, None)

    ok = capi.windows_spec(8, BOS, EOS, PAD)
    assert plan(ok, 0) == capi.TD_OK and plan(ok, 5) == capi.TD_OK
    assert plan(ok, 6) == capi.TD_E_INVALID            # overlap >= C
    assert plan(ok, -1) == capi.TD_E_INVALID           # overlap < 0
    assert plan(capi.windows_spec(2, BOS, EOS, PAD), 0) == capi.TD_E_INVALID   # C < 1
    assert plan(capi.windows_spec(1, BOS, -1, PAD), 0) == capi.TD_E_INVALID
    assert plan(capi.windows_spec(0, -1, -1, PAD), 0) == capi.TD_E_INVALID
    assert plan(capi.windows_spec(1 << 31, -1, -1, PAD), 0) == capi.TD_E_INVALID
    assert plan(capi.windows_spec(8, BOS, EOS, 1 << 40), 0) == capi.TD_E_INVALID  # pad is an int32
    for flags in (capi.TD_ROWS_DROP_LAST, capi.TD_ROWS_TRUNCATE, 4):
        sp = capi.windows_spec(8, BOS, EOS, PAD)
        sp.flags = flags
        assert plan(sp, 0) == capi.TD_E_INVALID
    for layout in (capi.TD_ROWS_CONCAT, capi.TD_ROWS_PAD, capi.TD_ROWS_BESTFIT, 4):
        sp = capi.windows_spec(8, BOS, EOS, PAD)
        sp.layout = layout
        assert plan(sp, 0) == capi.TD_E_INVALID
    assert plan(None, 0) == capi.TD_E_INVALID and plan(ok, 0, o=None) == capi.TD_E_INVALID and plan(ok, 0, c=None) == capi.TD_E_INVALID
    assert plan(ok, 0, n_docs=-1) == capi.TD_E_INVALID
    assert plan(ok, 0, o=np.array([1, 3, 10], np.int64)) == capi.TD_E_INVALID   # does not start at 0
    assert plan(ok, 0, o=np.array([0, 11, 10], np.int64)) == capi.TD_E_INVALID  # decreases
    with pytest.raises(capi.TokenDaggerHipError) as ei:
        capi.window_plan(offs, ok, 6)
    assert ei.value.code == capi.TD_E_INVALID
    # the other layouts' planner rejects the new layout
    with pytest.raises(capi.TokenDaggerHipError):
        capi.pack_plan(offs, ok)
