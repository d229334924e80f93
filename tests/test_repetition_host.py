"""td_repetition_host, the contract's executable statement (no device), against the truth (tests/repetition_truth.py)."""
import numpy as np
import pytest

import repetition_truth as rt


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, got[0].tolist(), want[0].tolist())
    assert np.array_equal(got[1], want[1]), (what, got[1].tolist(), want[1].tolist())


def test_the_cases_and_random_texts():
    from tokendagger_amd import capi
    named = list(rt.cases().items()) + [(f"seed {s}", rt.random_case(s)) for s in range(300)]
    for name, (text, offs) in named:
        for groups in (rt.LINES, rt.PARAS, rt.LINES | rt.PARAS):
            same(capi.repetition_host(text, offs, groups), rt.truth(text, offs, groups), (name, groups))
    s = rt.truth(*rt.cases()["the rule's examples"])[0]
    assert s[0, 0] == 2 and s[2, 0] == 0 and s[3, 6] == 2 and s[4, 6] == 1 and s[9, 3] == 1
    tm = rt.truth(*rt.cases()["Thue-Morse, its complement and a copy"])[0]
    assert tm[0, 3] == 1 and rt.truth(*rt.cases()["Thue-Morse and its complement"])[0][0, 3] == 0


def test_argument_errors_write_nothing():
    from tokendagger_amd import capi
    for groups, offs in ((0, [0, 2]), (4, [0, 2]), (3, [1, 2]), (3, [0, 2, 1])):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            capi.repetition_host(b"ab", np.asarray(offs, dtype=np.int64), groups)
        assert e.value.code == capi.TD_E_INVALID
