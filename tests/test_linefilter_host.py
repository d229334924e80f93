"""td_line_filter_host, the rule's executable statement, against the rule in plain Python (tests/linefilter_truth.py): the seam cases
the GPU test uses, a few hundred random texts over an alphabet that makes events dense, and every argument error, which writes nothing."""
import random

import numpy as np
import pytest

import linefilter_truth as lt


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build_hip()
    from tokendagger_amd import capi
    return capi


def test_seam_cases(capi):
    for name, (text, offs, kw) in lt.seam_cases().items():
        lt.same(capi.line_filter_host(text, offs, lt.make_rules(kw)), lt.filter_lines(text, offs, **kw), name)


def test_random_texts(capi):
    rnd = random.Random(7)
    alphabet = [b"a", b"A", b" ", b"\n", b".", b"\r", "”".encode()]
    for i in range(400):
        text = b"".join(rnd.choice(alphabet) for _ in range(rnd.randrange(0, 60)))
        offs = sorted([0, len(text)] + [rnd.randrange(0, len(text) + 1) for _ in range(rnd.randrange(0, 4))])
        kw = dict(min_words=rnd.randrange(0, 3), max_word_bytes=rnd.randrange(0, 4), need_terminal=rnd.random() < 0.5,
                  drop=rnd.choice([(), (b"aa",), (b"a.", b". a")]), count=rnd.choice([(), (b"a",), (b"aa", b"a a")]))
        lt.same(capi.line_filter_host(text, offs, lt.make_rules(kw)), lt.filter_lines(text, offs, **kw), (i, text, offs, kw))


BAD_RULES = {
    "a phrase with an LF": dict(drop=(b"a\nb",)),
    "a phrase in upper case": dict(count=(b"aB",)),
    "an empty phrase": dict(drop=(b"",)),
    "a phrase of 33 bytes": dict(drop=(b"x" * 33,)),
    "17 phrases": dict(drop=(b"x",) * 17),
    "negative min_words": dict(min_words=-1),
    "negative max_word_bytes": dict(max_word_bytes=-1),
}


@pytest.mark.parametrize("name", list(BAD_RULES) + ["unknown flag bits", "an unknown kind", "offsets that decrease", "offsets not from 0"])
def test_argument_errors_write_nothing(capi, name):
    text, offs = np.frombuffer(b"Some words.\nmore\n", dtype=np.uint8), np.array([0, 12, 17], dtype=np.int64)
    rules = lt.make_rules(BAD_RULES.get(name, {}))
    if name == "unknown flag bits":
        rules.flags = 2
    if name == "an unknown kind":
        rules = capi.LineRules.make(phrases=[(2, b"x")])
    if name == "offsets that decrease":
        offs = np.array([0, 13, 12], dtype=np.int64)
    if name == "offsets not from 0":
        offs = np.array([1, 12, 17], dtype=np.int64)
    out, ooff, stats, totals = np.full(32, 0x77, np.uint8), np.full(3, 0x77, np.int64), np.full((2, 8), 0x77, np.int64), np.full(8, 0x77, np.int64)
    rc = capi.load_library().td_line_filter_host(text.ctypes.data, offs.ctypes.data, 2, capi.ctypes.byref(rules), out.ctypes.data, 32,
                                                 ooff.ctypes.data, stats.ctypes.data, totals.ctypes.data)
    assert rc == capi.TD_E_INVALID
    assert all((x == 0x77).all() for x in (out, ooff, stats, totals))


def test_capacity_one_byte_short(capi):
    text, offs, kw = lt.seam_cases()["one document of 4097"]
    want = lt.filter_lines(text, offs, **kw)
    with pytest.raises(capi.TokenDaggerHipError) as e:
        capi.line_filter_host(text, offs, lt.make_rules(kw), capacity=len(want[0]) - 1)
    assert e.value.code == capi.TD_E_CAPACITY
    lt.same(capi.line_filter_host(text, offs, lt.make_rules(kw), capacity=len(want[0])), want, "exactly enough")
