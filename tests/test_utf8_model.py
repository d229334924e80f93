"""UTF-8 validation and repair without a GPU: the two truths of tests/utf8_truth.py (the interpreter's codec and the unit walker) against
each other, td_utf8_host through the C ABI and the CPU model of the kernels' decomposition (tests/twin/utf8_model.cpp over
tokendagger_amd/csrc/td_utf8_args.h) at tile sizes 64, 256 and 4096 against both, the window screen against the walker, and every
argument error of the contract."""
import ctypes
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import utf8_truth as ut
from tokendagger_amd import capi
from tokendagger_amd.capi import utf8_host  # noqa: F401  (the feature under test: without it nothing here runs)

ROOT = Path(__file__).resolve().parents[1]
TILES = [64, 256, 4096]
POLICIES = [ut.REPLACE, ut.IGNORE]


@pytest.fixture(scope="module")
def cases():
    """Built once, shared and left unchanged: tile -> {name: (text, offsets, {policy: truth})}."""
    return {tile: {name: (text, offs, {p: ut.truth(text, offs, p) for p in POLICIES}) for name, (text, offs) in ut.limit_cases(tile).items()}
            for tile in TILES}


def test_exports_and_names():
    lib = capi.load_library()
    for n in ("td_utf8_host", "td_utf8_check_device", "td_utf8_device", "td_utf8", "td_encode_batch_utf8"):
        assert n in capi.EXPORTS_UTF8 and hasattr(lib, n)
    for n in ("utf8_check", "utf8_device", "utf8", "encode_batch_utf8"):
        assert callable(getattr(capi.HipTokenizer, n))
    assert (capi.TD_UTF8_REPLACE, capi.TD_UTF8_IGNORE) == (0, 1)
    import tokendagger
    for n in ("validate_batch", "repair_batch", "encode_batch_to_numpy_repaired"):
        assert callable(getattr(tokendagger.Tokenizer, n))
    hdr = (ROOT / "include" / "tokendagger_hip.h").read_text()
    for n in capi.EXPORTS_UTF8:
        assert f"int {n}(" in hdr


def test_truths_agree_on_every_short_string():
    """All 406 901 strings of length <= 4 over the 25 boundary bytes: the walker is the codec, the context rule is the walker, and the
    host statement (one call, a document a string) is both."""
    strings = list(ut.exhaustive(4))
    assert len(strings) == sum(25 ** k for k in range(5)) == 406901
    for s in strings:
        r = ut.walk(s, ut.REPLACE)[0]
        assert r == s.decode("utf-8", "replace").encode() and ut.walk(s, ut.IGNORE)[0] == s.decode("utf-8", "ignore").encode(), s
        starts = set(ut.unit_starts(s))
        assert all(ut.starts_by_context(s, p) == (p in starts) for p in range(len(s))), s
    text, offs = ut.batch(strings)
    for policy in POLICIES:
        out, ooff, flags, first, nbad, counts = utf8_host(text, offs, policy)
        want = b"".join(s.decode("utf-8", ut.ERRORS[policy]).encode() for s in strings)
        assert bytes(out) == want and counts[0] == len(want)
        assert np.array_equal(flags, np.asarray([s.decode("utf-8", "ignore").encode() != s for s in strings], dtype=np.uint8))
        assert np.array_equal(nbad, np.asarray([s.decode("utf-8", "replace").count("�") for s in strings])), "no string here holds U+FFFD"


def test_truths_agree_on_random_strings():
    rng = np.random.default_rng(38)
    pool = np.frombuffer(ut.BOUNDARY, dtype=np.uint8)
    docs = [bytes(pool[rng.integers(0, 25, size=int(rng.integers(5, 12)))]) for _ in range(20000)]
    for s in docs:
        for policy in POLICIES:
            assert ut.walk(s, policy)[0] == ut.codec(s, policy), s
        starts = set(ut.unit_starts(s))
        assert all(ut.starts_by_context(s, p) == (p in starts) for p in range(len(s))), s
    text, offs = ut.batch(docs)
    for policy in POLICIES:
        ut.same(utf8_host(text, offs, policy), ut.truth(text, offs, policy, ut.codec_walk), policy)


@pytest.mark.parametrize("tile", TILES)
def test_host_equals_the_truths(cases, tile):
    assert len(cases[tile]) > 150
    for name, (text, offs, want) in cases[tile].items():
        for policy in POLICIES:
            ut.same(utf8_host(text, offs, policy), want[policy], (name, policy))
            if tile == 64:
                assert bytes(ut.truth(text, offs, policy, ut.codec_walk)[0]) == bytes(want[policy][0]), name
    text, offs, want = cases[tile]["a tile of strays"]
    assert want[ut.REPLACE][5][0] == len(text) + 2 * tile and want[ut.IGNORE][5][0] == len(text) - tile
    text, offs, want = cases[tile]["begins with continuation bytes, ends in a lead"]
    assert want[0][5].tolist() == [len(text) + 3 * 2, 2, 3, 3, 1, 1, 0, 0]  # (three subparts of one byte become three bytes each)


# ---- the model ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    src = ROOT / "tests" / "twin" / "utf8_model.cpp"
    out = ROOT / "tests" / "twin" / "_build" / "libutf8model.so"
    out.parent.mkdir(parents=True, exist_ok=True)
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))  # (td_utf8_args.h takes __host__ __device__ from HIP's host header)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__",
                           f"-I{rocm / 'include'}", str(src), "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.utf8_model.restype = i32
    lib.utf8_model.argtypes = [vp, vp, i64, i32, i32, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.utf8_screen.restype = i32
    lib.utf8_screen.argtypes = [vp]
    return lib


def run_model(lib, text, offs, policy, tile, shift=0, cap=None):
    """-> (rc, (out, out_offsets, flags, first_bad, n_bad, counts), (check flags, check first_bad), stats)"""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    n_docs = len(offs) - 1
    cap = 3 * int(offs[-1]) if cap is None else cap
    out = np.full(max(cap, 1) + 8, 0xEE, dtype=np.uint8)
    ooff = np.full(n_docs + 1, -7, dtype=np.int64)
    cf, fl = (np.zeros(max(n_docs, 1), dtype=np.uint8) for _ in range(2))
    cfirst, first, nbad = (np.zeros(max(n_docs, 1), dtype=np.int64) for _ in range(3))
    counts, stats = np.zeros(8, dtype=np.int64), np.zeros(6, dtype=np.int64)
    rc = lib.utf8_model(text.ctypes.data if len(text) else None, offs.ctypes.data, n_docs, policy, tile, shift, out.ctypes.data, cap,
                        ooff.ctypes.data, cf.ctypes.data, cfirst.ctypes.data, fl.ctypes.data, first.ctypes.data, nbad.ctypes.data,
                        counts.ctypes.data, stats.ctypes.data)
    assert np.all(out[cap:] == 0xEE), "bytes behind the capacity were written"
    return (rc, (out[:int(counts[0])] if rc == 0 else out[:cap], ooff, fl[:n_docs], first[:n_docs], nbad[:n_docs], counts),
            (cf[:n_docs], cfirst[:n_docs]), stats)


@pytest.mark.parametrize("tile", TILES)
def test_model_equals_the_host_statement(model, cases, tile):
    seen = np.zeros(6, dtype=np.int64)
    for name, (text, offs, want) in cases[tile].items():
        for policy in POLICIES:
            for shift in (range(16) if tile == 64 or name.startswith("shorter than a window") else (0, 5, 15)):
                rc, got, (cf, cfirst), stats = run_model(model, text, offs, policy, tile, shift)
                assert rc == 0, (name, shift, rc)
                ut.same(got, want[policy], (name, policy, shift))
                assert np.array_equal(cf, want[policy][2]) and np.array_equal(cfirst, want[policy][3]), (name, shift, "the check", cfirst, want[policy][3])
                seen = np.maximum(seen, stats)
    assert seen[0] >= 3 and seen[1] > 0 and seen[2] > 0 and seen[3] > 0 and seen[4] > 0, seen  # (every path of the decomposition was taken)


def test_the_screen_is_exact_on_well_formed_text_and_catches_every_subpart(model):
    """u8_window_suspect on a window with four bytes of text on either side: never set when the 24 bytes are well-formed with whole units,
    always set when a byte of the window belongs to an ill-formed subpart of that text whose unit starts and ends inside the 24 bytes'
    three-byte margins."""
    rng = np.random.default_rng(5)
    good = [c.encode() for c in ("a", "é", "€", "😀", "ࠀ", "퟿", "\U00010000", "\U0010ffff", "\x7f", "߿")]
    for _ in range(4000):
        s = b""
        while len(s) < 40:
            s += good[int(rng.integers(0, len(good)))]
        # cut at unit starts so that the 24 bytes are well-formed text by themselves
        starts = ut.unit_starts(s)
        for p in starts[:6]:
            if p + 24 in starts:
                w = np.frombuffer(s[p:p + 24], dtype=np.uint8).copy()
                assert model.utf8_screen(w.ctypes.data) == 0, s[p:p + 24]
    pool = np.frombuffer(ut.BOUNDARY, dtype=np.uint8)
    for _ in range(60000):
        w = pool[rng.integers(0, 25, size=24)].copy()
        w[:3], w[21:] = 0x41, 0x41  # (the margins a unit needs: the text's rule and the 24 bytes' rule agree on bytes 3 .. 20)
        s = bytes(w)
        ill_in_window = False
        for p in ut.unit_starts(s):
            n, wf = ut.unit(s, p)
            if not wf and p + n > 4 and p < 20:
                ill_in_window = True
        if ill_in_window:
            assert model.utf8_screen(w.ctypes.data) == 1, s


def test_model_capacity(model):
    text, offs = ut.batch([b"\x80" * 40, b"abc"])
    rc, got, _, _ = run_model(model, text, offs, ut.REPLACE, 64, 0, cap=122)
    assert rc == 5 and got[5][0] == 123 and np.all(got[0] == 0xEE) and np.all(got[1] == -7)
    rc, got, _, _ = run_model(model, text, offs, ut.REPLACE, 64, 0, cap=123)
    assert rc == 0 and len(got[0]) == 123
    rc, got, _, _ = run_model(model, text, offs, ut.IGNORE, 64, 0, cap=3)
    assert rc == 0 and bytes(got[0]) == b"abc" and got[1].tolist() == [0, 0, 3]


# ---- the host statement's contract -------------------------------------------------------------------------------------------------------

def test_argument_errors_write_nothing():
    lib = capi.load_library()
    text = np.frombuffer(b"ab\xe2\x82cd\xff\xe2\x82\xac12", dtype=np.uint8).copy()
    good = np.asarray([0, 6, 12], dtype=np.int64)

    def call(offs=good, n_docs=None, have_text=True, have_out=True, cap=64, have_counts=True, have_offs=True, out=None, policy=0):
        o = np.ascontiguousarray(offs, dtype=np.int64)
        outb = np.full(64, 0xEE, dtype=np.uint8) if out is None else out
        ooff, counts = np.full(8, -7, dtype=np.int64), np.full(8, -7, dtype=np.int64)
        fl, first, nbad = np.full(8, 7, dtype=np.uint8), np.full(8, -7, dtype=np.int64), np.full(8, -7, dtype=np.int64)
        rc = lib.td_utf8_host(text.ctypes.data if have_text else None, o.ctypes.data if have_offs else None, len(o) - 1 if n_docs is None else n_docs,
                              policy, outb.ctypes.data if have_out else None, cap, ooff.ctypes.data, fl.ctypes.data, first.ctypes.data,
                              nbad.ctypes.data, counts.ctypes.data if have_counts else None)
        untouched = (np.all(outb[:64] == 0xEE) and np.all(ooff == -7) and np.all(fl == 7) and np.all(first == -7) and np.all(nbad == -7) and
                     np.all(counts == -7))
        return rc, untouched, counts

    rc, untouched, counts = call()
    assert rc == capi.TD_OK and not untouched and counts.tolist() == [15, 2, 2, 3, 0, 0, 0, 0]
    for kw in (dict(offs=[1, 6, 12]), dict(offs=[0, 7, 6]), dict(offs=[0, -1, 12]), dict(n_docs=-1), dict(have_text=False), dict(have_counts=False),
               dict(have_offs=False), dict(cap=-1), dict(have_out=False, cap=5), dict(out=text[4:]), dict(out=text), dict(policy=2),
               dict(policy=-1)):
        rc, untouched, _ = call(**kw)
        assert rc == capi.TD_E_INVALID and (untouched or "out" in kw), kw
    # a NULL out with capacity 0: flags and counts alone
    rc, untouched, counts = call(have_out=False, cap=0)
    assert rc == capi.TD_OK and counts.tolist() == [15, 2, 2, 3, 0, 0, 0, 0]
    # an empty batch needs no text
    rc, _, counts = call(offs=[0, 0], have_text=False)
    assert rc == capi.TD_OK and counts[0] == 0
    with pytest.raises(capi.TokenDaggerHipError) as e:
        utf8_host(text, [0, 13])
    assert e.value.code == capi.TD_E_INVALID


def test_capacity_is_exact():
    text, offs = ut.batch([b"\x80" * 100, "€".encode() * 10 + b"\xe2\x82", b"plain"])
    need = 300 + 33 + 5
    assert utf8_host(text, offs, want_text=False)[5][0] == need
    with pytest.raises(capi.TokenDaggerHipError) as e:
        utf8_host(text, offs, capacity=need - 1)
    assert e.value.code == capi.TD_E_CAPACITY and e.value.counts[0] == need
    out, ooff, _, _, _, _ = utf8_host(text, offs, capacity=need)
    assert len(out) == need and ooff.tolist() == [0, 300, 333, 338]
    # the bounds are met exactly: 3 x under REPLACE, 1 x under IGNORE
    t3, o3 = ut.batch([b"\x80" * 777])
    assert utf8_host(t3, o3)[5][0] == 3 * 777 and utf8_host(t3, o3, ut.IGNORE)[5][0] == 0
    clean, oc = ut.batch([ut.filler(500)])
    assert len(utf8_host(clean, oc, ut.IGNORE, capacity=500)[0]) == 500


@pytest.mark.parametrize("policy", POLICIES)
def test_repaired_text_is_clean_and_repairs_to_itself(cases, policy):
    for name, (text, offs, _) in cases[256].items():
        out, ooff, flags, first, nbad, counts = utf8_host(text, offs, policy)
        again = utf8_host(out, ooff, policy)
        assert bytes(again[0]) == bytes(out) and np.array_equal(again[1], ooff), name
        assert not again[2].any() and (again[3] == -1).all() and not again[4].any() and again[5][1:4].tolist() == [0, 0, 0], name
