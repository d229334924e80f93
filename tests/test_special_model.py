"""Allowed special tokens without a GPU: the two truths of tests/special_truth.py against each other, and the CPU model of
td_special.hip's decomposition (tests/twin/special_model.cpp over tokendagger_amd/csrc/td_special_dev.h and td_special_table.h:
candidates per 32-byte word, a match per candidate, heads and cluster walks, the document bits of td_special_mark) against the truths:
on every call of special_truth.calls() (the sets and placements tests/test_gpu_special_sets.py sends to the kernels), with the
aligned and the bytewise load of the scan, and on a seeded fuzz the GPU cannot afford: 3000 cases (literal sets of 1 to 8 strings of
1 to 6 letters over {a,b,c,d}, every third case with most of them stretched to 48 bytes; texts that are soups of literals, their
prefixes and other bytes; documents cut anywhere).  A second build of the model with a candidate list of n / 32 + 8 entries walks
the overflow exit: the model reports where the kernel raises TD_E_SCRATCH."""
import ctypes
import os
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

import special_truth as stt

ROOT = Path(__file__).resolve().parents[1]
OK, BAD_INPUT, SCRATCH, LOADS_DIFFER = 0, 1, 2, 3
S_CANDIDATES, S_CAP, S_FIRST_LOST, S_HITS, S_HEADS, S_REMATCHES, S_CLIMBS, S_MAXLEN = range(8)
FUZZ_CASES = 3000


def _build(extra: int | None):
    src = ROOT / "tests" / "twin" / "special_model.cpp"
    out = ROOT / "tests" / "twin" / "_build" / (f"libspecialmodel{'' if extra is None else extra}.so")
    out.parent.mkdir(parents=True, exist_ok=True)
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))  # (td_special_dev.h takes __host__ __device__ from HIP's host header)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__",
                           *([] if extra is None else [f"-DSP_MODEL_CAND_EXTRA={extra}"]), f"-I{rocm / 'include'}", str(src), "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.special_model.restype = ctypes.c_int
    lib.special_model.argtypes = [vp, i64, vp, i64, vp, vp, vp, i64, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    return lib


@pytest.fixture(scope="module")
def model():
    return _build(None)


@pytest.fixture(scope="module")
def small_model():
    return _build(8)


def run_model(lib, text: bytes, offs, lits: dict, aligned: int = 1):
    """-> (rc, [(position, length, id)], hitbits, accbits, docbits, stats)"""
    x = np.frombuffer(text, dtype=np.uint8).copy() if text else np.zeros(1, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    n = len(text)
    items = list(lits.items())
    lb = np.frombuffer(b"".join(s for s, _ in items) or b"\0", dtype=np.uint8).copy()
    lo = np.concatenate([[0], np.cumsum([len(s) for s, _ in items])]).astype(np.int64)
    li = np.asarray([i for _, i in items] or [0], dtype=np.int32)
    nw = (n + 31) // 32
    pos, ln, idd = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int32), np.zeros(n + 1, dtype=np.int32)
    hit, acc, doc = np.zeros(nw + 1, dtype=np.uint32), np.zeros(nw + 1, dtype=np.uint32), np.zeros(nw + 1, dtype=np.uint32)
    n_out, stats = ctypes.c_int64(0), np.zeros(8, dtype=np.int64)
    rc = lib.special_model(x.ctypes.data, n, offs.ctypes.data, len(offs) - 1, lb.ctypes.data, lo.ctypes.data, li.ctypes.data, len(items), aligned,
                           pos.ctypes.data, ln.ctypes.data, idd.ctypes.data, ctypes.byref(n_out), hit.ctypes.data, acc.ctypes.data, doc.ctypes.data,
                           stats.ctypes.data)
    k = n_out.value
    return rc, list(zip(pos[:k].tolist(), ln[:k].tolist(), idd[:k].tolist())), hit[:nw], acc[:nw], doc, stats


def _bits(positions, nw):
    out = np.zeros(nw, dtype=np.uint32)
    for p in positions:
        out[p >> 5] |= np.uint32(1 << (p & 31))
    return out


def check(lib, text, offs, lits, what, aligned=1):
    want = stt.cuts(text, offs, lits)
    rc, got, hit, acc, doc, stats = run_model(lib, text, offs, lits, aligned)
    assert rc == OK, (what, rc)
    assert got == want, (what, "the model's cuts differ from the truths'", got[:5], want[:5])
    n, nw = len(text), (len(text) + 31) // 32
    assert np.array_equal(acc, _bits([p for p, _, _ in want], nw)), (what, "accept bitmap")
    assert np.array_equal(acc & ~hit, np.zeros(nw, dtype=np.uint32)), (what, "accepted without a hit")
    # a hit is a position at which some literal fits inside its document, whether it is cut out or lies inside a cut
    ends = [p + l for p, l, _ in want if p + l < n] + [int(o) for o in offs[:-1] if o < n] + [p for p, _, _ in want]
    assert np.array_equal(doc, _bits(ends, nw + 1)), (what, "document bits behind td_special_mark")
    return stats


def test_truths_agree_and_state_the_rule():
    L = {b"<|a|>": 1, b"<|a|><|b|>": 2, b"<|b|>": 3, b"<|": 4, b"a": 5}
    t = b"x<|a|><|b|>y<|a|<|b|>a"
    assert stt.cuts(t, [0, len(t)], L) == [(1, 10, 2), (12, 2, 4), (14, 1, 5), (16, 5, 3), (21, 1, 5)]
    # a document's end cuts a literal short: the shorter one that fits is taken, the rest is the next document's
    assert stt.cuts(t, [0, 8, len(t)], L) == [(1, 5, 1), (6, 2, 4), (12, 2, 4), (14, 1, 5), (16, 5, 3), (21, 1, 5)]
    for c in stt.calls():
        stt.cuts(c.text, c.offs, stt.literals(c.set_name))
    ids, toffs = stt.expected_ids(b"ab<|b|>", [0, 1, 7], L, lambda seg: np.asarray([1000 + len(seg)]))
    assert ids.tolist() == [5, 1001, 3] and toffs.tolist() == [0, 1, 3]


def test_sets_are_what_their_reasons_say():
    v = stt.vocabulary()
    assert min(v.values()) == 200000 and v["<|alias1|>"] == v["<|alias2|>"] and len(set(v.values())) == len(v) - 1
    for name, (strings, why) in stt.SETS.items():
        assert why and strings and all(1 <= len(s.encode()) <= (49 if name == "too_long" else 48) for s in strings), name
    assert sorted(len(s) for s in stt.LENS) == list(range(1, 49)) and not any(a != b and b.startswith(a) for a in stt.LENS for b in stt.LENS)
    assert max(len(s) for s in stt.SETS["one_byte"][0]) == 1
    for a, b in (("graph_a", "graph_b"),):
        assert len(stt.SETS[a][0]) == len(stt.SETS[b][0]) and max(map(len, stt.SETS[a][0])) == max(map(len, stt.SETS[b][0])) == 48


def test_model_equals_the_truths_on_every_call(model):
    climbs = {}
    for c in stt.calls():
        for aligned in (1, 0):
            stats = check(model, c.text, c.offs, stt.literals(c.set_name), (c.name, aligned), aligned)
        climbs[c.set_name] = max(climbs.get(c.set_name, 0), int(stats[S_CLIMBS]))
    assert climbs["chain"] == 47 and climbs["lens"] == 0 and climbs["one_byte"] == 0
    # the climbs the set was built for: '<s>a"' ends four parents up at '<s>a'; '<sz' ends at -1 and is no hit
    rc, got, hit, _, _, _ = run_model(model, b'<s>a"', [0, 5], stt.literals("chain"))
    assert rc == OK and got == [(0, 4, stt.vocabulary()["<s>a"])]
    rc, got, hit, _, _, stats = run_model(model, b"<sz", [0, 3], stt.literals("chain_noroot"))
    assert rc == OK and got == [] and stats[S_CANDIDATES] == 1 and stats[S_HITS] == 0
    # maxlen 1: every hit is a head
    rc, got, _, _, _, stats = run_model(model, b"||||", [0, 4], stt.literals("one_byte"))
    assert stats[S_HEADS] == stats[S_HITS] == 4 and stats[S_REMATCHES] == 0 and stats[S_MAXLEN] == 1
    # one cluster: a head, the rest by the walk
    rc, got, _, _, _, stats = run_model(model, b"|" * 100, [0, 100], stt.literals("one_and_48"))
    assert len(got) == 100 and stats[S_HEADS] == 1 and stats[S_REMATCHES] == 99


def _fuzz_case(rng: random.Random, k: int):
    lits = {s.encode(): 200000 + j for j, s in enumerate(stt._soup_set(rng, k % 3 == 2))}
    text = stt.soup_text(rng, list(lits))
    cut = sorted(rng.randrange(len(text) + 1) for _ in range(rng.randrange(5)))
    return text, [0] + cut + [len(text)], lits


def test_model_equals_the_truths_on_the_fuzz(model):
    rng = random.Random(2024)
    cutsum = 0
    for k in range(FUZZ_CASES):
        text, offs, lits = _fuzz_case(rng, k)
        check(model, text, offs, lits, ("fuzz", k), aligned=k & 1)
        cutsum += 1
    assert cutsum == FUZZ_CASES


def test_model_reports_the_overflow_exit(small_model, model):
    """n candidates against n / 32 + 8: SCRATCH, the first candidate without room is the cap-th, the listed ones are still matched."""
    lits = stt.literals("one_byte")
    for n in (8, 9, 10, 33, 300):
        text = b"|" * n
        rc, got, _, _, _, stats = run_model(small_model, text, [0, n], lits)
        cap = n // 32 + 8
        assert stats[S_CAP] == cap and stats[S_CANDIDATES] == n
        if n <= cap:
            assert rc == OK and len(got) == n
        else:
            assert rc == SCRATCH and stats[S_FIRST_LOST] == cap and got == [(p, 1, lits[b"|"]) for p in range(cap)]
    # the product's capacity: 256 KiB of candidates against n / 32 + 4096
    n = 256 << 10
    rc, got, _, _, _, stats = run_model(model, b"|" * n, [0, n], lits)
    assert rc == SCRATCH and stats[S_CAP] == n // 32 + 4096 and stats[S_FIRST_LOST] == stats[S_CAP] and len(got) == stats[S_CAP]
    # under the cap nothing is lost
    rc, got, _, _, _, stats = run_model(small_model, b"x" * 64 + b"|" * 10 + b"x" * 64, [0, 138], lits)
    assert rc == OK and stats[S_CAP] == 12 and len(got) == 10
    # input the model refuses
    assert run_model(model, b"abc", [0, 2], lits)[0] == BAD_INPUT
    assert run_model(model, b"abc", [0, 3], {b"x" * 49: 1})[0] == BAD_INPUT
