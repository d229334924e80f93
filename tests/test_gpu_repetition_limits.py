"""td_repetition_device at the limits its design text names: td_rp_prefix with more than one tile a lane (257 and 513 tiles, a line that
crosses a lane's whole chunk), a tile whose table of documents does not fit LDS (runs of empty documents, a sweep around RC_LDS_DOCS
with the run inside a line), nothing but empty documents, one table slot under contention, the capacity check at that scale and repeats
on a poisoned workspace.  tests/test_limit_cases_model.py proves on the CPU which path each case of repetition_truth.limit_cases() and
big_cases() reaches; here every result is compared with the truth, exactly.  run() and same() are test_gpu_repetition.py's: the guard
bytes around the text, the 0xFF-filled outputs with slack and the pointer shift are theirs.
No case here makes the device fault: every error is one the library reports by a status code."""
import pytest

import repetition_truth as rt
from helpers import every_case
from test_gpu_repetition import ALL, FF, run, same, tok  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def limits():
    """Built once, shared and left unchanged: name -> (text, offsets, (stats, totals))."""
    return {name: (text, offs, rt.truth(text, offs)) for name, (text, offs) in rt.limit_cases().items()}


@pytest.fixture(scope="module")
def bigs():
    """name -> (text, offsets, {groups: (stats, totals)})"""
    return {name: (text, offs, {g: rt.truth(text, offs, g) for g in (rt.LINES, rt.PARAS, ALL)}) for name, (text, offs) in rt.big_cases().items()}


@pytest.mark.parametrize("shift", rt.SHIFTS)
def test_limit_cases_equal_truth(tok, limits, shift):
    def one(name, text, offs, want):
        got, st, rest = run(tok, text, offs, ALL, shift)
        assert st[0] == 0 and rest, (name, st)
        same(got, want, (name, shift))
    every_case(limits, one)


@pytest.mark.parametrize("groups", (rt.LINES, rt.PARAS, ALL))
@pytest.mark.parametrize("shift", rt.SHIFTS)
def test_big_cases_equal_truth(tok, bigs, shift, groups):
    def one(name, text, offs, want):
        got, st, rest = run(tok, text, offs, groups, shift)
        assert st[0] == 0 and rest, (name, st)
        same(got, want[groups], (name, shift, groups))
    every_case(bigs, one)


@pytest.mark.parametrize("shift", (0, 1))
def test_capacity_at_scale(tok, bigs, shift):
    """256 tiles, and 257: td_rp_prefix's capacity branch behind two tiles a lane"""
    from tokendagger_amd import capi
    text, offs, want = bigs["big A, cut"]
    need = int(want[ALL][1][0] + want[ALL][1][6])
    assert need > 100000
    got, st, rest = run(tok, text, offs, ALL, shift, max_units=need - 1)
    assert st == (capi.TD_E_CAPACITY, need) and rest and (got[0] == FF).all() and (got[1] == FF).all()
    got, st, rest = run(tok, text, offs, ALL, shift, max_units=need)
    assert st[0] == 0 and rest
    same(got, want[ALL], "the exact need")


def test_repeats_on_a_poisoned_workspace(tok, bigs):
    from tokendagger_amd import capi
    tok.set_option(capi.TD_OPT_WS_FILL, 0xA5)
    try:
        clone = tok.clone()
    finally:
        tok.set_option(capi.TD_OPT_WS_FILL, -1)
    try:
        for name in ("big A, one document", "big A, cut"):
            text, offs, want = bigs[name]
            for k in range(3):
                got, st, rest = run(clone, text, offs, ALL, 1)
                assert st[0] == 0 and rest
                same(got, want[ALL], ("poisoned", name, k))
    finally:
        clone.close()
