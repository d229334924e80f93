"""Field joins on the CPU: a hand-worked example of the contract (include/tokendagger_hip.h, td_join_spec), the loop truth against
the vectorised one, td_join_plan (host only; it runs the truncation rule the kernels run) against both, TD_JOIN_SHRINK_LONGEST on
lengths no loop can walk, and the C ABI's argument checks (no device needed for those)."""
import ctypes

import numpy as np
import pytest

import join_truth as jt

BOS, EOS = 900, 901


def _capi():
    from tokendagger_amd import capi
    capi.load_library()
    return capi


def _cases(n=400, seed=11):
    rng = np.random.default_rng(seed)
    return [jt.random_case(rng, K=(1 if i % 10 == 0 else 8 if i % 10 == 1 else None)) for i in range(n)]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)


def _sft(max_total):
    # [BOS] prompt completion [EOS]: the prompt keeps its END when cut and is cut first, the completion and EOS are trained
    return jt.make_join([jt.field([BOS], rank=1, keep_tail=True, type=0), jt.field(rank=2, train=True, type=1)], tail=[EOS], tail_type=1,
                        train_tail=True, max_total=max_total)


def test_hand_worked_example():
    # K = 2, fixed = 2 (BOS, EOS), max_total = 8.  Documents (prompt, completion) of five examples, ids 1 .. 31 in document order:
    #   0: 1 2 3 | 4 5              need 2 + 5 = 7: fits
    #   1: 6 7 8 9 10 11 | 12 13    need 10, over 2: the prompt (rank 1) loses 2 and keeps its end, 8 9 10 11
    #   2: 14 15 16 | 17 .. 23      need 12, over 4: the prompt loses all 3, the completion (rank 2) the last 1 of its 7
    #   3: - | -                    need 2: an empty example, kept as BOS EOS
    #   4: 24 .. 31 | -             need 10, over 2: the prompt keeps 26 .. 31
    lengths = [3, 2, 6, 2, 3, 7, 0, 0, 8, 0]
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ids = np.arange(1, 32, dtype=np.int32)
    want_ids = [BOS, 1, 2, 3, 4, 5, EOS, BOS, 8, 9, 10, 11, 12, 13, EOS, BOS, 17, 18, 19, 20, 21, 22, EOS, BOS, EOS,
                BOS, 26, 27, 28, 29, 30, 31, EOS]
    I = -100
    want_lab = [I, I, I, I, 4, 5, EOS, I, I, I, I, I, 12, 13, EOS, I, 17, 18, 19, 20, 21, 22, EOS, I, EOS, I, I, I, I, I, I, I, EOS]
    want_typ = [0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1]
    capi = _capi()
    join = _sft(8)
    for f in (jt.join_brute, jt.join_numpy):
        o_ids, o_lab, o_typ, o_offs, o_ex, o_len, counts = f(ids, offs, join)
        assert o_ids.tolist() == want_ids, f.__name__
        assert o_lab.tolist() == want_lab and o_typ.tolist() == want_typ
        assert o_offs.tolist() == [0, 7, 15, 23, 25, 33] and o_ex.tolist() == [0, 1, 2, 3, 4]
        assert o_len.tolist() == [[3, 2], [4, 2], [0, 6], [0, 0], [6, 0]]
        assert counts.tolist() == [5, 33, 0, 3]
        # max_total = 1 is below the two literals: fixed > max_total, and no cut of a body can help: every example is dropped,
        # the empty one too.  (Within one call fixed and max_total are the same for every example, so this case is a call of its own.)
        o_ids, _, _, o_offs, o_ex, o_len, counts = f(ids, offs, _sft(1))
        assert len(o_ids) == 0 and o_offs.tolist() == [0] and len(o_ex) == 0 and counts.tolist() == [0, 0, 5, 0]
    counts, p_offs, p_ex, p_len = capi.join_plan(offs, jt.capi_spec(join))
    assert counts.tolist() == [5, 33, 0, 3] and p_offs.tolist() == [0, 7, 15, 23, 25, 33] and p_ex.tolist() == [0, 1, 2, 3, 4]
    assert p_len.tolist() == [[3, 2], [4, 2], [0, 6], [0, 0], [6, 0]]
    counts, p_offs, p_ex, p_len = capi.join_plan(offs, jt.capi_spec(_sft(1)))
    assert counts.tolist() == [0, 0, 5, 0] and p_offs.tolist() == [0] and len(p_ex) == 0
    # longest_first on example 2 (3 | 7, over 4): 7 -> 6 -> 5 -> 4 -> 3, the prompt untouched
    join["shrink"] = "longest"
    assert jt.kept_lengths(join, [3, 7]) == ([3, 3], False)
    assert jt.kept_lengths(join, [6, 6]) == ([3, 3], False)  # over 6: a tie is taken from the HIGHEST index first, 6 5 | 5 5 | 5 4 ...
    assert jt.kept_lengths(join, [5, 6]) == ([3, 3], False) and jt.kept_lengths(join, [4, 5]) == ([3, 3], False)
    join["max_total"] = 9
    assert jt.kept_lengths(join, [6, 6]) == ([4, 3], False)  # an odd rest: the lower index keeps the extra id


def test_brute_equals_numpy():
    seen = set()
    for ids, offs, join in _cases():
        b = jt.join_brute(ids, offs, join)
        _same(b, jt.join_numpy(ids, offs, join))
        fs = join["fields"]
        K = len(fs)
        n_ex = (len(offs) - 1) // K
        assert b[6][0] + b[6][2] == n_ex and b[6][1] == b[3][-1] == len(b[0])
        L = np.diff(offs)
        for x in range(n_ex):
            Lx = [int(L[jt.doc_of(join, n_ex, x, f)]) for f in range(K)]
            c, dropped = jt.kept_lengths(join, Lx)
            capped = [min(Lx[f], fs[f]["max_len"]) if fs[f]["max_len"] >= 0 else Lx[f] for f in range(K)]
            cut = c != capped
            seen.add(("cap binds", capped != Lx))
            seen.add(("dropped", dropped))
            seen.add(("empty example kept", not dropped and sum(c) == 0 and not any(f["before"] for f in fs) and not join["tail"]))
            seen.add((join["shrink"], cut and not dropped))
            seen.add(("keep_tail cut", any(fs[f]["keep_tail"] and 0 < c[f] < Lx[f] for f in range(K)) and not dropped))
            sh = [capped[f] for f in range(K) if fs[f]["rank"] > 0]
            seen.add(("tie in longest", join["shrink"] == "longest" and cut and not dropped and len(sh) > 1 and sorted(sh)[-1] == sorted(sh)[-2]))
        seen |= {("K", K), ("field_major", join["field_major"] and n_ex > 1 and K > 1)}
    for what in ("cap binds", "dropped", "empty example kept", "order", "longest", "keep_tail cut", "tie in longest", "field_major"):
        assert (what, True) in seen, what
    assert ("K", 1) in seen and ("K", 8) in seen


def test_plan_equals_truths():
    capi = _capi()
    for ids, offs, join in _cases():
        t = jt.join_numpy(ids, offs, join)
        sp = jt.capi_spec(join)
        counts, p_offs, p_ex, p_len = capi.join_plan(offs, sp)
        assert np.array_equal(counts, t[6]) and np.array_equal(p_offs, t[3]) and np.array_equal(p_ex, t[4])
        assert p_len.dtype == np.int32 and np.array_equal(p_len, t[5])
        assert np.array_equal(capi.join_plan(offs, sp, outputs=False), t[6])
        assert np.array_equal(jt.join_brute(ids, offs, join)[6], counts)


def test_longest_closed_form_equals_the_loop():
    rng = np.random.default_rng(2)
    n = 0
    for _ in range(4000):
        K = int(rng.integers(1, 9))
        c = [int(v) for v in rng.integers(0, 9, K)]
        shrinkable = [bool(v) for v in rng.integers(0, 3, K)]
        over = int(rng.integers(0, sum(c) + 3))
        fs = [jt.field(rank=1 if shrinkable[f] else 0) for f in range(K)]
        join = jt.make_join(fs, max_total=max(sum(c) - over, 0), shrink="longest")
        if sum(c) - over < 0:
            continue
        want = jt.kept_lengths(join, c)
        got = jt.longest_closed(c, shrinkable, over)
        assert got[1] == want[1] and (want[1] or got[0] == want[0]), (c, shrinkable, over)  # (a dropped example's lengths mean nothing)
        n += 1
    assert n > 3000


def test_longest_on_lengths_near_2_to_31():
    """One id at a time these would take 2^31 steps an example: td_join_plan finishes because the rule is in closed form.  Against
    longest_closed (checked against the loop above)."""
    capi = _capi()
    big = (1 << 31) - 5
    rng = np.random.default_rng(5)
    rows = [[big, big, 7], [big, big - 1, big - 2], [big, 3, big], [big, big, big], [1, big, 0], [big - 3, big - 3, big - 4]]
    rows += [[int(v) for v in big - rng.integers(0, 50, 3)] for _ in range(30)]
    for shrinkable in ([True, True, True], [True, False, True], [False, True, True]):
        for max_total in (10, 11, big, big + 1, 2 * big - 1, 2 * big + 6, 3 * big - 1):
            fs = [jt.field(rank=1 if s else 0) for s in shrinkable]
            join = jt.make_join(fs, max_total=max_total, shrink="longest")
            L = np.array(rows, np.int64)
            offs = np.concatenate([[0], np.cumsum(L.reshape(-1))]).astype(np.int64)
            counts, p_offs, p_ex, p_len = capi.join_plan(offs, jt.capi_spec(join))
            want_len, want_ex = [], []
            for x, r in enumerate(rows):
                c, dropped = jt.longest_closed(r, shrinkable, sum(r) - max_total)
                if not dropped:
                    want_len.append(c)
                    want_ex.append(x)
                    assert sum(c) == min(sum(r), max_total)
            assert p_ex.tolist() == want_ex and p_len.tolist() == want_len, (shrinkable, max_total)
            assert counts[0] + counts[2] == len(rows) and counts[1] == sum(map(sum, want_len)) == p_offs[-1]
            c2, d2 = jt.lengths_numpy(join, L)
            assert c2[~d2].tolist() == want_len


def test_field_major_is_the_interleaved_result_on_permuted_offsets():
    capi = _capi()
    for ids, offs, join in _cases(150, seed=12):
        K = len(join["fields"])
        n_ex = (len(offs) - 1) // K
        # the same fields, laid out the other way: documents permuted, ids moved with them
        other = dict(join, field_major=not join["field_major"])
        L = np.diff(offs)
        perm = np.array([jt.doc_of(join, n_ex, x, f) for x in range(n_ex) for f in range(K)], np.int64)  # interleaved order of `join`'s documents
        if other["field_major"]:
            perm = perm.reshape(n_ex, K).T.reshape(-1)
        o2 = np.concatenate([[0], np.cumsum(L[perm])]).astype(np.int64)
        ids2 = np.concatenate([ids[offs[d]:offs[d + 1]] for d in perm] + [np.zeros(0, np.int32)]).astype(np.int32)
        _same(jt.join_brute(ids, offs, join), jt.join_brute(ids2, o2, other))
        a, b = capi.join_plan(offs, jt.capi_spec(join)), capi.join_plan(o2, jt.capi_spec(other))
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def _plan_rc(capi, offs, spec, counts=True, n_docs=None, n_ex_room=16):
    lib = capi.load_library()
    o = np.ascontiguousarray(offs, np.int64)
    c = np.full(4, 55, np.int64)
    out_o, out_e, out_l = np.full(n_ex_room, 77, np.int64), np.full(n_ex_room, 77, np.int64), np.full(8 * n_ex_room, 77, np.int32)
    rc = lib.td_join_plan(o.ctypes.data, len(o) - 1 if n_docs is None else n_docs, ctypes.byref(spec) if spec is not None else None,
                          c.ctypes.data if counts else None, out_o.ctypes.data, out_e.ctypes.data, out_l.ctypes.data)
    assert rc == capi.TD_OK or ((out_o == 77).all() and (out_e == 77).all() and (out_l == 77).all())  # an error writes no output
    return rc, c


def test_argument_checks_without_a_device():
    capi = _capi()
    offs = np.array([0, 3, 5, 11, 13, 13, 13], np.int64)
    F = capi.join_field
    good = lambda **kw: capi.join_spec([F([1], shrink_rank=1), F()], tail=[2], **kw)
    assert _plan_rc(capi, offs, good())[0] == capi.TD_OK
    big = 1 << 31
    bad_specs = [
        capi.join_spec([]),                                            # K = 0
        capi.join_spec([F()] * 2, n_fields=9),                         # K = 9
        capi.join_spec([F(), dict(F(), n_before=17)]),                 # literal counts out of range
        capi.join_spec([F(), dict(F(), n_before=-1)]),
        capi.join_spec([F(max_len=-2), F()]),
        good(max_total=-2),
        capi.join_spec([F(shrink_rank=-1), F()]),
        good(shrink=2), good(shrink=-1),                               # unknown shrink
        good(flags=4), good(flags=-1),                                 # unknown spec flags
        capi.join_spec([F(flags=8), F()]),                             # unknown field flags
        good(ignore_index=big), good(ignore_index=-big - 1),           # outside int32
        good(tail_type=big),
        capi.join_spec([F(type_value=-big - 1), F()]),
        None,
    ]
    for bad in bad_specs:
        rc, c = _plan_rc(capi, offs, bad)
        assert rc == capi.TD_E_INVALID and c[0] == -1
    sp = good()
    sp.n_tail = 17
    rc, c = _plan_rc(capi, offs, sp)
    assert rc == capi.TD_E_INVALID and c[0] == -1
    # the limits themselves are fine
    assert _plan_rc(capi, offs, good(ignore_index=big - 1, tail_type=-big, max_total=0, shrink=1, flags=3))[0] == capi.TD_OK
    assert _plan_rc(capi, offs, capi.join_spec([F(list(range(16)), max_len=0)] * 6, tail=list(range(16))))[0] == capi.TD_OK
    with pytest.raises(ValueError):
        capi.join_spec([F()] * 9)
    with pytest.raises(ValueError):
        capi.join_spec([F(list(range(17)))])
    # n_docs % K != 0
    rc, c = _plan_rc(capi, offs[:-1], good())
    assert rc == capi.TD_E_INVALID and c[0] == -1
    rc, c = _plan_rc(capi, offs, capi.join_spec([F()] * 4))
    assert rc == capi.TD_E_INVALID and c[0] == -1
    assert _plan_rc(capi, offs, good(), counts=False)[0] == capi.TD_E_INVALID
    assert _plan_rc(capi, offs, good(), n_docs=-2)[0] == capi.TD_E_INVALID
    # offsets that decrease or are negative: the position is the example, in both layouts
    dec = offs.copy()
    dec[3], dec[4] = offs[4], offs[3]  # document 3 (13 .. 11) decreases: example 1 interleaved, example 0 field-major (documents 0 and 3)
    rc, c = _plan_rc(capi, dec, good())
    assert rc == capi.TD_E_INVALID and c[0] == 1
    rc, c = _plan_rc(capi, dec, good(field_major=True))
    assert rc == capi.TD_E_INVALID and c[0] == 0
    with pytest.raises(capi.TokenDaggerHipError) as ei:
        capi.join_plan(dec, good())
    assert ei.value.code == capi.TD_E_INVALID and ei.value.counts[0] == 1
    neg = offs - 1
    rc, c = _plan_rc(capi, neg, good())
    assert rc == capi.TD_E_INVALID and c[0] == 0
    # nothing joined from nothing
    rc, c = _plan_rc(capi, np.zeros(1, np.int64), good())
    assert rc == capi.TD_OK and c.tolist() == [0, 0, 0, 0]
