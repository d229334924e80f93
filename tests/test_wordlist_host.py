"""td_word_matches_host, the rule's executable statement, against the rule in plain Python (tests/wordlist_truth.py) on the seam cases
the GPU test uses, and every argument error of the SET paragraph with its position, which writes nothing."""
import numpy as np
import pytest

import wordlist_truth as wt


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build_hip()
    from tokendagger_amd import capi
    return capi


@pytest.mark.parametrize("name", list(wt.seam_cases()))
def test_seam_cases(capi, name):
    text, offs, entries, groups, flags = wt.seam_cases()[name]
    wt.same(capi.word_matches_host(entries, groups, flags, text, offs), wt.matches(text, offs, entries, groups, flags), name)


BAD_LISTS = {  # name -> (entries, groups, flags, the position reported)
    "an empty entry": ([b"a", b"", b"c"], None, 1, 1),
    "65 bytes": ([b"a", b"b", b"x" * 65], None, 1, 2),
    "64 bytes are fine, group 64 is not": ([b"x" * 64, b"b"], [63, 64], 1, 1),
    "a negative group": ([b"a"], [-1], 0, 0),
    "upper case under the fold": ([b"a", b"bC"], None, 1, 1),
    "a duplicate: the second one": ([b"a", b"b", b"c", b"b", b"a"], None, 0, 3),
    "the lowest of two faults": ([b"a", b"a", b""], None, 0, 1),
    "unknown flag bits": ([b"a"], None, 4, -1),
    "no entry": ([], None, 1, -1),
    "65536 entries": ([b"%d" % i for i in range(65536)], None, 1, -1),
}


@pytest.mark.parametrize("name", list(BAD_LISTS))
def test_list_errors_name_the_entry_and_write_nothing(capi, name):
    entries, groups, flags, pos = BAD_LISTS[name]
    eb, eo, eg = capi.word_list(entries, groups)
    text, offs = np.frombuffer(b"a b c", dtype=np.uint8), np.array([0, 5], dtype=np.int64)
    stats, totals, hits, got = np.full(4, 0x77, np.int64), np.full(4, 0x77, np.int64), np.full(max(len(entries), 1), 0x77, np.int64), capi.ctypes.c_int64(7)
    rc = capi.load_library().td_word_matches_host(eb.ctypes.data if len(eb) else None, eo.ctypes.data, eg.ctypes.data if eg is not None else None,
                                                 len(entries), flags, text.ctypes.data, offs.ctypes.data, 1, stats.ctypes.data, totals.ctypes.data,
                                                 hits.ctypes.data, capi.ctypes.byref(got))
    assert (rc, got.value) == (capi.TD_E_INVALID, pos)
    assert all((x == 0x77).all() for x in (stats, totals, hits))


def test_upper_case_is_an_entry_without_the_fold(capi):
    wt.same(capi.word_matches_host([b"The"], None, 0, b"the The", [0, 7]), wt.matches(b"the The", [0, 7], [b"The"], None, 0), "no fold")


@pytest.mark.parametrize("offs", [[1, 5], [0, 4, 3]])
def test_bad_offsets(capi, offs):
    with pytest.raises(capi.TokenDaggerHipError) as e:
        capi.word_matches_host([b"a"], None, 1, b"a b c", offs)
    assert e.value.code == capi.TD_E_INVALID and e.value.pos == -1
