"""td_word_ngrams_host, the contract's executable statement (no device), against the truth (tests/wordgrams_truth.py)."""
import numpy as np
import pytest

import wordgrams_truth as wt


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, got[0].tolist(), want[0].tolist())
    assert np.array_equal(got[1], want[1]), (what, got[1].tolist(), want[1].tolist())


def test_the_cases_and_random_texts():
    from tokendagger_amd import capi
    named = list(wt.cases().items()) + [(f"seed {s}", wt.random_case(s)) for s in range(300)]
    for name, (text, offs) in named:
        for groups in (wt.TOP, wt.DUP, wt.TOP | wt.DUP):
            same(capi.word_ngrams_host(text, offs, groups), wt.truth(text, offs, groups), (name, groups))
    s = wt.truth(*wt.cases()["the rule's examples"])[0]
    assert s[0].tolist()[:5] == [6, 6, 12, 3, 2] and s[2, 0] == 0 and s[3, 3] == 2 and s[5, 0] == 2 and s[7, 3:5].tolist() == [2, 4]
    assert wt.truth(*wt.cases()["equal counts, different chars"])[0][:, 3:5].tolist() == [[2, 5], [2, 5]]
    assert wt.truth(*wt.cases()["a 5-gram twice"])[0][:, 9].tolist() == [10, 10, 7, 15]
    assert wt.truth(*wt.cases()["a 10-gram in two documents and in one"])[0][:, 14].tolist() == [0, 0, 42]
    assert wt.truth(*wt.cases()["Thue-Morse and its complement"])[0][0, 3] == 1
    assert wt.truth(*wt.cases()["Thue-Morse, its complement and a copy"])[0][0, 3] == 2


def test_the_greedy_walk_never_exceeds_dup_chars():
    for seed in range(300):
        text, offs = wt.random_case(seed)
        stats = wt.truth(text, offs, wt.DUP)[0]
        for d in range(len(offs) - 1):
            words = bytes(text)[offs[d]:offs[d + 1]].split()
            for n in range(5, 11):
                assert wt.greedy_dup_chars(words, n) <= stats[d, 9 + n - 5], (seed, d, n)


def test_argument_errors_write_nothing():
    from tokendagger_amd import capi
    for groups, offs in ((0, [0, 2]), (4, [0, 2]), (3, [1, 2]), (3, [0, 2, 1])):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            capi.word_ngrams_host(b"ab", np.asarray(offs, dtype=np.int64), groups)
        assert e.value.code == capi.TD_E_INVALID
