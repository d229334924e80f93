"""td_mask_addresses_host, the rule's executable statement, against the rule in plain Python (tests/mask_truth.py): the seam cases the
GPU test uses, a few hundred random texts over an alphabet that makes anchors dense, and every argument error, which writes nothing."""
import random

import numpy as np
import pytest

import mask_truth as mt


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build_hip()
    from tokendagger_amd import capi
    return capi


def test_seam_cases(capi):
    for name, (text, offs, kw) in mt.seam_cases().items():
        mt.same(capi.mask_addresses_host(text, offs, mt.make_rules(kw)), mt.mask(text, offs, **kw), name)


def test_random_texts(capi):
    rnd = random.Random(11)
    alphabet = [b"a", b"Z", b"1", b"0", b"2", b"5", b".", b".", b"@", b"-", b"_", b" ", b"\n", b"a.aa", b"1.2.5.0", b"a@Z.aa"]  # (and runs of it that match)
    for i in range(600):
        text = b"".join(rnd.choice(alphabet) for _ in range(rnd.randrange(0, 40)))
        offs = sorted([0, len(text)] + [rnd.randrange(0, len(text) + 1) for _ in range(rnd.randrange(0, 4))])
        kw = dict(emails=rnd.choice([(), (b"<m>",), (b"", b"MAIL", b"m" * 32)]), ips=rnd.choice([(), (b"<i>",), (b"I", b"", b"ii")]), keep=rnd.random() < 0.5)
        mt.same(capi.mask_addresses_host(text, offs, mt.make_rules(kw)), mt.mask(text, offs, **kw), (i, text, offs, kw))


BAD_RULES = {
    "nine literals": lambda r: setattr(r, "n_ips", 9),
    "a negative count": lambda r: setattr(r, "n_emails", -1),
    "a literal of 33 bytes": lambda r: setattr(r.emails[0], "len", 33),
    "unknown flag bits": lambda r: setattr(r, "flags", 8 | 1),
    "e-mails on with no literal": lambda r: setattr(r, "n_emails", 0),
    "IPv4 on with no literal": lambda r: setattr(r, "n_ips", 0),
}


@pytest.mark.parametrize("name", list(BAD_RULES) + ["offsets that decrease", "offsets not from 0"])
def test_argument_errors_write_nothing(capi, name):
    text, offs = np.frombuffer(b"to bob@x.com\n1.2.3.4\n", dtype=np.uint8), np.array([0, 13, 21], dtype=np.int64)
    rules = mt.make_rules(mt.BOTH)
    BAD_RULES.get(name, lambda r: None)(rules)
    if name == "offsets that decrease":
        offs = np.array([0, 14, 13], dtype=np.int64)
    if name == "offsets not from 0":
        offs = np.array([1, 13, 21], dtype=np.int64)
    out, ooff, stats, totals = np.full(64, 0x77, np.uint8), np.full(3, 0x77, np.int64), np.full((2, 6), 0x77, np.int64), np.full(6, 0x77, np.int64)
    rc = capi.load_library().td_mask_addresses_host(text.ctypes.data, offs.ctypes.data, 2, capi.ctypes.byref(rules), out.ctypes.data, 64,
                                                    ooff.ctypes.data, stats.ctypes.data, totals.ctypes.data)
    assert rc == capi.TD_E_INVALID
    assert all((x == 0x77).all() for x in (out, ooff, stats, totals))


def test_capacity_one_byte_short(capi):
    text, offs, kw = mt.seam_cases()["literals of 32 bytes"]
    want = mt.mask(text, offs, **kw)
    assert len(want[0]) > len(text)
    with pytest.raises(capi.TokenDaggerHipError) as e:
        capi.mask_addresses_host(text, offs, mt.make_rules(kw), capacity=len(want[0]) - 1)
    assert e.value.code == capi.TD_E_CAPACITY
    mt.same(capi.mask_addresses_host(text, offs, mt.make_rules(kw), capacity=len(want[0])), want, "exactly enough")
