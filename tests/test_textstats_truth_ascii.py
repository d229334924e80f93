"""The truth of the text statistics (tests/textstats_truth.py) pinned by a second, independent statement for ASCII-only documents, in
plain Python on `bytes`: split(), isalpha(), max(map(len, ...)).  ASCII whitespace is what bytes.split() splits on but for 0x1C - 0x1F,
which the class tables call spaces and Python does not: the documents here hold none.  td_text_stats_host must give the same."""
import numpy as np
import pytest

import textstats_truth as tt
from tokendagger_amd import capi
from tokendagger_amd.capi import text_stats_host  # noqa: F401  (the feature under test: without it nothing here runs)

ASCII = [b" ", b" ", b"\n", b"\r", b"\t", b".", b".", b"#", b"{", b"}", b"-", b"*", b"!", b"?", b'"', b"a", b"b", b"Z", b"7", b"_", b"'", b"/", b"\x0b", b"\x0c"]


def plain(doc: bytes) -> dict:
    words = doc.split()
    lines = doc.split(b"\n")
    if lines[-1] == b"":
        lines = lines[:-1]
    runs, k = 0, 0
    while k < len(doc):
        j = k
        while j < len(doc) and doc[j] == 0x2E:
            j += 1
        runs += j - k >= 3
        k = max(j, k + 1)
    return {
        tt.BYTES: len(doc), tt.CHARS: len(doc), tt.UPPER: sum(chr(c).isupper() for c in doc), tt.LOWER: sum(chr(c).islower() for c in doc),
        tt.LETTER_OTHER: 0, tt.MARK: 0, tt.NUMBER: sum(chr(c).isdigit() for c in doc), tt.SPACE: sum(chr(c).isspace() for c in doc),
        tt.NON_ASCII: 0, tt.WORDS: len(words), tt.WORDS_ALPHA: sum(any(chr(c).isalpha() for c in w) for w in words),
        tt.WORD_MAX: max(map(len, words), default=0), tt.LINES: len(lines), tt.LINES_BLANK: sum(not ln.strip() for ln in lines),
        tt.LINE_MAX: max(map(len, lines), default=0),
        tt.END_TERMINAL: sum(ln.rstrip()[-1:] in (b".", b"!", b"?", b'"') for ln in lines),
        tt.END_ELLIPSIS: sum(ln.rstrip().endswith(b"...") for ln in lines),
        tt.START_BULLET: sum(ln.lstrip()[:1] in (b"-", b"*") for ln in lines),
        tt.HASHES: doc.count(b"#"), tt.ELLIPSES: runs, tt.CURLY: doc.count(b"{") + doc.count(b"}"),
    }


@pytest.fixture(scope="module")
def docs():
    rng = np.random.default_rng(11)
    out = [b"", b"a\n\nb\n", b"\n", b"a", b"...", b"....", b".. ...\n", b"- x\n  * y\n\n", b"A b.\nC d!  \n e?\"\n", b"x " * 300]
    for _ in range(1500):
        out.append(b"".join(ASCII[i] for i in rng.integers(0, len(ASCII), size=int(rng.integers(0, 80)))))
    return out


def test_the_truth_is_the_plain_statement_on_ascii(docs):
    text = b"".join(docs)
    offs = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    stats, totals = tt.truth(text, offs)
    for d, doc in enumerate(docs):
        want = plain(doc)
        assert {c: int(stats[d, c]) for c in range(tt.COLS)} == want, doc
    assert (b"a\n\nb\n", 3) == (docs[1], int(stats[1, tt.LINES])) and stats[0, tt.LINES] == 0
    got, gtot = text_stats_host(text, offs)
    assert np.array_equal(got, stats) and np.array_equal(gtot, totals)


def test_groups_and_argument_errors_of_the_host_statement(docs):
    text = b"".join(docs[:200])
    offs = np.concatenate([[0], np.cumsum([len(d) for d in docs[:200]])]).astype(np.int64)
    for g in (tt.LOCAL, tt.RUNS, tt.LOCAL | tt.RUNS):
        want, wtot = tt.truth(text, offs, g)
        got, gtot = text_stats_host(text, offs, g)
        assert np.array_equal(got, want) and np.array_equal(gtot, wtot), g
        if g != tt.LOCAL | tt.RUNS:
            assert not got[:, tt.RUNS_COLS if g == tt.LOCAL else tt.LOCAL_COLS].any()
    lib = capi.load_library()
    buf = np.frombuffer(text, dtype=np.uint8)
    for groups, o in ((0, offs), (4, offs), (7, offs), (-1, offs), (3, offs[::-1].copy()), (3, offs + 1)):
        stats = np.full((len(o) - 1, tt.COLS), -7, dtype=np.int64)
        totals = np.full(tt.COLS, -7, dtype=np.int64)
        rc = lib.td_text_stats_host(buf.ctypes.data, o.ctypes.data, len(o) - 1, groups, stats.ctypes.data, totals.ctypes.data)
        assert rc == capi.TD_E_INVALID and (stats == -7).all() and (totals == -7).all(), groups
    assert capi.TD_TS_COLS == tt.COLS and len(capi.TS_COLUMNS) == tt.COLS and (capi.TD_TS_LOCAL, capi.TD_TS_RUNS) == (tt.LOCAL, tt.RUNS)
    for n in ("td_text_stats_host", "td_text_stats_device", "td_text_stats", "td_encode_batch_text_stats"):
        assert n in capi.EXPORTS and hasattr(lib, n)
