"""What the limit cases of tests/repetition_truth.py and tests/wordgrams_truth.py reach, proven from their inputs on the CPU: the
library has no counter for the path a kernel took, so every property a case exists for is asserted here from a model of the kernel's
own arithmetic (rp_tiles and td_rp_prefix's chunks in td_repetition_scan.h, rw_table and rw_doc_of in td_rewrite_common.h, the grids
and thresholds of td_wordgrams.hip).  The device tests (test_gpu_repetition_limits.py, test_gpu_wordgrams_limits.py) then only compare.
The contracts' host statements (td_repetition_host, td_word_ngrams_host) are held against the truth on the same cases."""
import numpy as np
import pytest

import repetition_truth as rt
import wordgrams_truth as wt

TILE, SHIFTS = rt.TILE, rt.SHIFTS
WG_ALL = wt.TOP | wt.DUP
SEPS = {"rp": b"\n", "wg": b" \t\n\r\x0b\x0c"}


@pytest.fixture(scope="module")
def rp():
    """name -> (text, offsets, (stats, totals)), limit and big cases together; built once and left unchanged"""
    return {k: (x, o, rt.truth(x, o)) for k, (x, o) in {**rt.limit_cases(), **rt.big_cases()}.items()}


@pytest.fixture(scope="module")
def wg():
    return {k: (x, o, wt.truths(x, o)[WG_ALL]) for k, (x, o) in {**wt.limit_cases(), **wt.big_cases()}.items()}


def test_the_merged_truth_is_the_truth_of_both_groups():
    for name, (text, offs) in wt.cases().items():
        t, want = wt.truths(text, offs), wt.truth(text, offs, WG_ALL)
        assert np.array_equal(t[WG_ALL][0], want[0]) and np.array_equal(t[WG_ALL][1], want[1]), name


def test_the_builders_repeat_themselves():
    for m in (rt, wt):
        for build in (m.limit_cases, m.big_cases):
            a, b = build(), build()
            assert list(a) == list(b)
            for k in a:
                assert a[k][0] == b[k][0] and np.array_equal(a[k][1], b[k][1]) and a[k][1].dtype == np.int64 and a[k][1][0] == 0, k
                assert (np.diff(a[k][1]) >= 0).all() and a[k][1][-1] <= len(a[k][0]), k


# ---- td_rp_prefix: the tiles and a lane's chunk ------------------------------------------------------------------------------------------
def prefix_chunks(ntiles):
    """[t0, t1) of every lane of td_rp_prefix"""
    per = (ntiles + rt.PREFIX_LANES - 1) // rt.PREFIX_LANES
    return per, [(min(lane * per, ntiles), min(min(lane * per, ntiles) + per, ntiles)) for lane in range(rt.PREFIX_LANES)]


def test_the_big_texts_tiles_and_chunks():
    assert [rt.tiles(rt.BIG_A, s) for s in SHIFTS] == [256, 257, 257] and [rt.tiles(rt.BIG_B, s) for s in SHIFTS] == [513] * 3
    per, ch = prefix_chunks(256)
    assert per == 1 and all(t1 - t0 == 1 for t0, t1 in ch)
    per, ch = prefix_chunks(257)
    assert per == 2 and ch[127] == (254, 256) and ch[128] == (256, 257) and all(t0 == t1 == 257 for t0, t1 in ch[129:])
    per, ch = prefix_chunks(513)
    assert per == 3 and ch[170] == (510, 513) and all(t0 == t1 == 513 for t0, t1 in ch[171:])


@pytest.mark.parametrize("which", ["rp", "wg"])
def test_the_long_unit_of_the_big_texts(which, rp, wg):
    m, cases, sep = (rt, rp, SEPS["rp"]) if which == "rp" else (wt, wg, SEPS["wg"])
    for total, seed, names in ((rt.BIG_A, 21 if which == "rp" else 31, ("big A, one document", "big A, cut")),
                               (rt.BIG_B, 23 if which == "rp" else 33, ("big B, cut",))):
        text, (begin, end) = m.big_text(total, seed)
        n = 6 * TILE + 123
        long = text[begin:begin + n]
        assert len(text) == total and text[begin - 1] in sep and text[begin + n] in sep and not any(x in sep for x in long)
        second = text.index(long, begin + n)
        third = text.index(long[:-1], second + n)
        assert second + n < third and third + n - 1 < end and text[third + n - 1] in sep and text[second - 1] in sep and text[third - 1] in sep
        assert TILE // 4 < begin < TILE - 64  # mid-tile at every shift
        if which == "wg":  # a word is a duplicate only with its neighbours: the same words behind all three copies
            behind = [text[at:at + 200].split()[:12] for at in (begin + n, second + n, third + n - 1)]
            assert behind[0] == behind[1] == behind[2] and len(behind[0]) == 12
            # the copy without its last byte is no duplicate: with the whole word in its place the truth is another
            lo, hi = begin - 100, third + n + 200
            whole = text[lo:third] + long + text[third + n - 1:hi]
            for x, y in ((text[lo:hi], whole),) + (((text, text[:third] + long + text[third + n - 1:]),) if total == rt.BIG_A else ()):
                t, u = wt.truth(*wt.docs(x)), wt.truth(*wt.docs(y))
                assert u[0][0, 3] >= 3 and (t[0][0, 9:] < u[0][0, 9:]).all() and u[0][0, 9] - t[0][0, 9] >= n - 1, (t[0].tolist(), u[0].tolist())
        for s in SHIFTS:
            first_whole, end_whole = (begin + s + TILE - 1) // TILE, (begin + n + s) // TILE  # tiles [first_whole, end_whole) lie inside it
            assert end_whole - first_whole >= 5
            per, ch = prefix_chunks(rt.tiles(total, s))
            assert per == 1 or any(first_whole <= t0 and t0 + per == t1 <= end_whole for t0, t1 in ch), "no lane's whole chunk inside the unit"
        for name in names:  # all three copies lie in one document
            x, offs, (stats, totals) = cases[name]
            assert x == text and (np.searchsorted(offs, begin, "right") == np.searchsorted(offs, end - 1, "right"))
            assert (totals != 0).all(), (name, totals.tolist())
            assert (len(offs) == 2) == name.endswith("one document") and (name.endswith("one document") or (50 < len(offs) < 75 and (np.diff(offs) == 0).sum() >= 3))


# ---- rw_table: the empty runs ------------------------------------------------------------------------------------------------------------
def _doc_of_all(offs, table):
    """the model of rw_doc_of on every byte of the tile against a plain search"""
    n_docs = len(offs) - 1
    for x in range(table[0], table[1]):
        assert rt.doc_of_model(offs, table, x) == int(np.searchsorted(offs[:n_docs], x, "right")) - 1, (table, x)


@pytest.mark.parametrize("which", ["rp", "wg"])
def test_the_sweep_of_empty_runs_asks_for_both_tables(which, rp, wg):
    cases, sep, unit = (rp, SEPS["rp"], "line") if which == "rp" else (wg, SEPS["wg"], "word")
    kinds = set()
    for E in rt.EMPTY_RUNS:
        text, offs, _ = cases[f"{E} empty documents inside a {unit}"]
        at = int(offs[1])
        assert len(offs) == E + 3 and (offs[1:-1] == at).all() and text[at - 1] not in sep and text[at] not in sep
        for s in SHIFTS:
            (table,) = rt.tile_tables(offs, s)
            assert table[:4] == (0, len(text), 0, E + 2) and table[4] == (E <= 4349)
            kinds.add(table[4])
            _doc_of_all(offs, table)
    assert kinds == {True, False}
    assert min(rt.EMPTY_RUNS) <= 4349 < 4350 <= max(rt.EMPTY_RUNS) and set(range(4344, 4357)) <= set(rt.EMPTY_RUNS)


@pytest.mark.parametrize("which", ["rp", "wg"])
def test_the_runs_of_10000_empty_documents(which, rp, wg):
    cases, sep = (rp, SEPS["rp"]) if which == "rp" else (wg, SEPS["wg"])
    lds = lambda name, s: [t[4] for t in rt.tile_tables(cases[name][1], s)]  # noqa: E731
    text = cases["10 000 empty documents at byte 0"][0]
    assert 2 * TILE + 15 < len(text) < 2 * TILE + 1024
    assert not any(x in sep for x in text[TILE - 16:TILE + 2])  # one unit across the edge of every shift
    for s in SHIFTS:
        assert lds("10 000 empty documents at byte 0", s) == [False, True, True]
        name = "10 000 empty documents mid-tile inside a unit"
        at = int(cases[name][1][1])
        assert lds(name, s) == [False, True, True] and text[at - 1] not in sep and text[at] not in sep
        name = f"10 000 empty documents on the tile edge of shift {s}"
        offs = cases[name][1]
        tables = rt.tile_tables(offs, s)
        # the run begins where tile 1 begins: kb is the document in front of it, the run's entries are tile 1's
        assert tables[1][0] == offs[1] == TILE - s and tables[1][2] == 0 and tables[1][3] == 10002 and [t[4] for t in tables] == [True, False, True]
        for other in SHIFTS:
            assert lds(name, other).count(False) == 1
        assert lds("10 000 empty documents at the text's end", s) == [True, True, True]  # no tile sees the run
        for name in cases:
            if name.startswith("10 000"):
                offs = cases[name][1]
                assert len(offs) == 10003 and (np.diff(offs) == 0).sum() >= 10000
                for table in rt.tile_tables(offs, s):
                    for x in (table[0], (table[0] + table[1]) // 2, table[1] - 1, min(max(int(offs[1]), table[0]), table[1] - 1)):
                        assert rt.doc_of_model(offs, table, x) == int(np.searchsorted(offs[:-1], x, "right")) - 1
    for name, n_bytes in (("nothing but empty documents, no bytes", 0), ("nothing but empty documents, some bytes", 100)):
        x, offs, (stats, totals) = cases[name]
        assert len(x) == n_bytes and len(offs) == 5001 and not offs.any() and rt.tile_tables(offs, 1) == [] and not stats.any() and not totals.any()


# ---- word n-grams ----------------------------------------------------------------------------------------------------------------------------
def test_the_global_stride_case(wg):
    text, offs, (stats, totals) = wg["global stride"]
    assert stats[:, 0].tolist() == [540000, 2000] and stats[0, 0] > wt.GRID_WORDS and stats[1, 0] > wt.LDS_WORDS
    assert text[:200000] == b"a " * 100000
    # max_words as the device test passes it: the grid is WG_MAX_GRID workgroups, a lane of which takes a second word
    assert -(-(len(text) // 2 + 3) // 256) >= 2048
    assert rt.tiles(len(text), 0) > 256 and 1_300_000 < len(text) < 1_500_000
    assert (totals != 0).all() and stats[0, 3] >= 99999 and stats[0, 14] > 0


def test_the_long_list_case(wg):
    text, offs, (stats, totals) = wg["long list"]
    words = stats[:, 0]
    assert len(words) == 600 > 256
    long = np.flatnonzero(words > wt.LDS_WORDS)
    assert long.tolist() == [d for d in range(600) if d % 7 == 0] + [599] and (words[long] >= 1025).all() and (words[long] <= 1100).all()
    per = (600 + 255) // 256
    assert per == 3 and len(set((long // per).tolist())) > 80  # td_wg_long: the long documents lie in more than 80 lanes' chunks
    rest = np.delete(words, long)
    assert (rest <= 40).all() and (rest == 0).sum() > 50 and (rest == 1).sum() > 50 and (rest >= 2).sum() > 200
    first = np.concatenate([[0], np.cumsum(words[long])])  # the long words in front of each long document (long_first)
    k = int(np.flatnonzero(words[long] == 1088)[0])
    assert words[long[k:k + 3]].tolist() == [1088, 1088, 1089] and first[k] % 64 == 0 and first[k + 1] % 64 == 0 and first[k + 2] % 64 == 0
    assert first[k + 3] % 64 == 1  # the wavefront behind the 1089 words straddles two documents
    assert (totals != 0).all()


def test_the_small_word_cases(wg):
    text, offs, (stats, totals) = wg["LDS table steps"]
    assert tuple(stats[:, 0].tolist()) == wt.STEP_WORDS
    for n in (2, 10):  # n = 2: both sides of every step of the table's size; n = 10: of the steps to 128 and to 256 slots
        sizes = [max(64, 1 << (2 * (W - n + 1) - 1).bit_length()) for W in wt.STEP_WORDS]
        assert sorted(set(sizes)) == [64, 128, 256, 512, 1024, 2048][:len(set(sizes))] and len(set(sizes)) >= 5
    for d, W in enumerate(wt.STEP_WORDS):
        w = text[offs[d]:offs[d + 1]].split()
        assert len(w) == W and len(set(w)) == W - 12 and w[:12] == w[-12:]
        assert stats[d, 3:9].tolist()[::2] == [2, 2, 2] and (stats[d, 9:] == stats[d, 9]).all() and stats[d, 9] == 2 * sum(map(wt.chars, w[:12]))
    for n_docs in (31, 32, 33, 65):
        s = wg[f"{n_docs} documents of 2 to 6 words"][2][0]
        assert len(s) == n_docs and (s[:, 0] >= 2).all() and (s[:, 0] <= 6).all()
    s = wg["64 documents, words in the last alone"][2][0]
    assert len(s) == 2 * wt.DOC_BLOCK and (s[:63, 0] <= 1).all() and s[63, 0] == 7 and s[63, 3] == 3
    text, offs, (stats, totals) = wg["tie-break across lanes"]
    w = text.split()
    assert len(w) == 600 and len(offs) == 2
    where = lambda a, b: [i for i in range(599) if w[i] == a and w[i + 1] == b]  # noqa: E731
    assert len(where(b"aa", b"bb")) == 3 and max(where(b"aa", b"bb")) < 256 and len(where(b"cccc", b"dddd")) == 3 and min(where(b"cccc", b"dddd")) > 256
    assert stats[0, 3:5].tolist() == [3, 8]


# ---- repetition ------------------------------------------------------------------------------------------------------------------------------
def test_the_repetition_cases(rp):
    stats, totals = rp["2000 documents of the same five lines"][2]
    assert len(stats) == 2000 and (stats[:, [0, 6]] == [5, 2]).all() and not stats[:, 3:6].any() and not stats[:, 9:].any()
    stats, totals = rp["the same five lines 2000 times in one document"][2]
    assert rp["the same five lines 2000 times in one document"][0] == rp["2000 documents of the same five lines"][0]
    assert stats[0, 0] == 10000 and stats[0, 3] == 9995 and stats[0, 6] == 2001 and stats[0, 9] == 1998
    text, offs, (stats, totals) = rp["100 000 copies of one line"]
    assert text == b"ab\n" * 100000 and stats[0, :4].tolist() == [100000, 200000, 200000, 99999]
    for name in rp:
        if name.startswith("big"):
            assert (rp[name][2][1] != 0).all(), name


# ---- the host statements -----------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what


def test_the_host_statements_equal_the_truth(rp, wg):
    from tokendagger_amd import capi
    for name, (text, offs, want) in rp.items():
        if name != "big B, cut":
            _same(capi.repetition_host(text, offs), want, name)
    for name, (text, offs, want) in wg.items():
        if name != "big B, cut":
            _same(capi.word_ngrams_host(text, offs), want, name)
