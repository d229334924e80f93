"""NFC normalisation without a GPU: the two truths of tests/nfc_truth.py against each other, td_nfc_host through the C ABI and the CPU
model of the kernels' decomposition (tests/twin/nfc_model.cpp over tokendagger_amd/csrc/td_nfc_args.h) at tile sizes 64, 256 and 4096
against both and against the fixture tests/golden/nfc_golden.npz, and every argument error of the contract.  The comparisons with the
interpreter's unicodedata run only when its Unicode version is the tables'; the fixture tests always run."""
import ctypes
import os
import subprocess
import unicodedata as ud
from pathlib import Path

import numpy as np
import pytest

import nfc_truth as nt
from tokendagger_amd import capi
from tokendagger_amd.capi import nfc_host, nfc_info  # noqa: F401  (the feature under test: without it nothing here runs)

ROOT = Path(__file__).resolve().parents[1]
TABLE_VERSION = nfc_info(capi.TD_NFC_INFO_UNICODE_VERSION)
live = pytest.mark.skipif(nt.UNICODE_VERSION != TABLE_VERSION,
                          reason=f"unicodedata is Unicode {nt.UNICODE_VERSION}, the tables are {TABLE_VERSION}: the fixture tests cover this")
TILES = [64, 256, 4096]


@pytest.fixture(scope="module")
def golden():
    with np.load(ROOT / "tests" / "golden" / "nfc_golden.npz") as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def cases():
    """Built once, shared and left unchanged: tile -> {name: (text, offsets, truth)}."""
    if nt.UNICODE_VERSION != TABLE_VERSION:
        return {}
    return {tile: {name: (text, offs, nt.truth(text, offs)) for name, (text, offs) in nt.limit_cases(tile).items()} for tile in TILES}


def test_info_and_exports():
    assert TABLE_VERSION == 130000 and nfc_info(capi.TD_NFC_INFO_TABLE_BYTES) == 56290 and nfc_info(7) == -1
    lib = capi.load_library()
    for n in ("td_nfc_info", "td_nfc_host", "td_nfc_check_device", "td_nfc_device", "td_nfc", "td_encode_batch_nfc"):
        assert n in capi.EXPORTS and hasattr(lib, n)
    for n in ("nfc_check", "nfc_device", "nfc", "encode_batch_nfc"):
        assert callable(getattr(capi.HipTokenizer, n))


def test_fixture_is_the_tables_version(golden):
    assert int(golden["unicode_version"][0]) == TABLE_VERSION and int(golden["n_non_boundary"][0]) == 2060
    assert len(golden["group"]) == len(golden["offsets"]) - 1 and set(golden["group"].tolist()) == {0, 1, 2, 3, 4, 5}
    assert int((golden["group"] == 0).sum()) == 5 * 2060 and int((golden["group"] == 5).sum()) == 0x2FA1E - 0x2F800


def test_host_equals_the_fixture(golden):
    out, ooff, flags, changed, counts = nfc_host(golden["text"], golden["offsets"])
    assert np.array_equal(ooff, golden["want_offsets"]) and bytes(out) == bytes(golden["want"])
    docs, want = nt.docs_of(golden["text"], golden["offsets"]), nt.docs_of(golden["want"], golden["want_offsets"])
    assert np.array_equal(changed, np.asarray([a != b for a, b in zip(docs, want)], dtype=np.uint8))
    assert not np.any(changed & ~flags.astype(bool)), "a document that changed was proven"
    assert counts[0] == len(golden["want"]) and counts[2] == int(changed.sum()) and counts[1] == int(flags.sum())


@live
def test_known_answers():
    known = [([0x65, 0x301], [0xE9]), ([0x61, 0x301, 0x323], [0x1EA1, 0x301]), ([0x212B], [0xC5]), ([0x1100, 0x1161], [0xAC00]),
             ([0x1100, 0x1161, 0x11A8], [0xAC01]), ([0xAC00, 0x11A8], [0xAC01]), ([0x344], [0x308, 0x301]), ([0x1D15E], [0x1D157, 0x1D165]),
             ([0x2F800], [0x4E3D]), ([0x3B9, 0x308, 0x301], [0x390]), ([0x61, 0x327, 0x301], [0xE1, 0x327])]
    for src, want in known:
        src, want = "".join(map(chr, src)), "".join(map(chr, want))
        for fn in (nt.nfc_by_runs, nt.nfc_uax15, lambda b: bytes(nfc_host(b, [0, len(b)])[0])):
            assert fn(src.encode()) == want.encode() == ud.normalize("NFC", src).encode(), (src, fn)
    # the 3 x bound is met exactly
    assert len(ud.normalize("NFC", chr(0x1D1C0)).encode()) == 3 * len(chr(0x1D1C0).encode())


@live
def test_truths_agree_on_random_strings():
    rng = np.random.default_rng(15)
    non_boundary = [c for c in range(0x300, 0x30000) if not 0xD800 <= c <= 0xDFFF and not nt.is_boundary_cp(c)]
    assert len([c for c in range(0x30000, 0x110000) if not nt.is_boundary_cp(c)]) == 0 and len(non_boundary) == 2060
    pool = non_boundary + [0x61, 0x65, 0x41, 0x1100, 0x1105, 0xAC00, 0xAC01, 0x915, 0x4E00, 0x3B1, 0x20]
    for it in range(3000):
        s = "".join(chr(pool[i]) for i in rng.integers(0, len(pool), size=int(rng.integers(1, 9)))).encode()
        a, b = nt.nfc_by_runs(s), nt.nfc_uax15(s)
        assert a == b, (it, s)
        out, _, flags, changed, _ = nfc_host(s, [0, len(s)])
        assert bytes(out) == a and flags[0] == nt.doc_flag(s) and changed[0] == (a != s), (it, s)
        assert flags[0] or a == s, ("proven wrongly", s)


@live
@pytest.mark.parametrize("tile", TILES)
def test_host_equals_the_truths(cases, tile):
    for name, (text, offs, want) in cases[tile].items():
        nt.same(nfc_host(text, offs), want, name)
        if tile == 64 or "@" not in name:
            assert bytes(nt.truth(text, offs, nt.nfc_uax15)[0]) == bytes(want[0]), name


# ---- the model ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    src = ROOT / "tests" / "twin" / "nfc_model.cpp"
    out = ROOT / "tests" / "twin" / "_build" / "libnfcmodel.so"
    out.parent.mkdir(parents=True, exist_ok=True)
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))  # (td_nfc_args.h takes __host__ __device__ from HIP's host header)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__",
                           f"-I{rocm / 'include'}", str(src), "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.nfc_model.restype = i32
    lib.nfc_model.argtypes = [vp, vp, i64, i32, i32, vp, i64, vp, vp, vp, vp, vp, vp]
    return lib


def run_model(lib, text, offs, tile, shift=0, cap=None):
    """-> (rc, (out, out_offsets, flags, changed, counts), check_flags, stats)"""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    n_docs = len(offs) - 1
    cap = 3 * int(offs[-1]) if cap is None else cap
    out = np.full(max(cap, 1) + 8, 0xEE, dtype=np.uint8)
    ooff = np.full(n_docs + 1, -1, dtype=np.int64)
    cf, fl, ch = (np.zeros(max(n_docs, 1), dtype=np.uint8) for _ in range(3))
    counts, stats = np.zeros(8, dtype=np.int64), np.zeros(6, dtype=np.int64)
    rc = lib.nfc_model(text.ctypes.data if len(text) else None, offs.ctypes.data, n_docs, tile, shift, out.ctypes.data, cap, ooff.ctypes.data,
                       cf.ctypes.data, fl.ctypes.data, ch.ctypes.data, counts.ctypes.data, stats.ctypes.data)
    assert np.all(out[cap:] == 0xEE), "bytes behind the capacity were written"
    return rc, (out[:int(counts[0])] if rc == 0 else out[:cap], ooff, fl[:n_docs], ch[:n_docs], counts), cf[:n_docs], stats


@live
@pytest.mark.parametrize("tile", TILES)
def test_model_equals_the_truths(model, cases, tile):
    seen = np.zeros(6, dtype=np.int64)
    for name, (text, offs, want) in cases[tile].items():
        for shift in ((0, 5, 15) if "@" not in name or tile == 64 else (0,)):
            rc, got, check_flags, stats = run_model(model, text, offs, tile, shift)
            assert rc == 0, (name, shift, rc)
            nt.same(got, want, (name, shift))
            assert np.array_equal(check_flags, want[2]), (name, shift, "the check's flags")
            host = nfc_host(text, offs)
            assert np.array_equal(got[4], host[4]), (name, shift, "counts", got[4], host[4])
            seen = np.maximum(seen, stats)
    assert seen[0] >= 3 and seen[1] > 0 and seen[2] > 0 and seen[4] > 0, seen  # (every path of the decomposition was taken)


@pytest.mark.parametrize("tile", TILES)
def test_counts_of_windows_proven_by_their_bytes(model, tile):
    """Opaque bytes and the longest segment are counted in the windows that are copied without a look at the tables too: bytes below 0xCC
    in whole aligned windows, ASCII whose length is a multiple of 16."""
    c = nt.limit_cases(tile)
    for name, opaque in (("ascii, whole windows", 0), ("ascii, whole tiles", 0), ("stray continuation bytes in whole windows", 15),
                         ("ill-formed below 0xCC", 8 * 40), ("documents cut two-byte letters below 0xCC", 12)):
        text, offs = c[name]
        want = [len(text), 0, 0, 0, 0, opaque, 1, 0]
        assert nfc_host(text, offs)[4].tolist() == want, name
        for shift in (0, 9):
            rc, got, check_flags, stats = run_model(model, text, offs, tile, shift)
            assert rc == 0 and got[4].tolist() == want and bytes(got[0]) == bytes(text) and not check_flags.any(), (name, shift, got[4])
            assert shift or stats[1] + stats[3] < stats[0] * tile // 16 or opaque == 0, "no window was walked for its opaque bytes"


def test_model_equals_the_fixture(model, golden):
    for tile, shift in ((64, 3), (4096, 0)):
        rc, got, check_flags, _ = run_model(model, golden["text"], golden["offsets"], tile, shift)
        assert rc == 0 and bytes(got[0]) == bytes(golden["want"]) and np.array_equal(got[1], golden["want_offsets"])
        host = nfc_host(golden["text"], golden["offsets"])
        assert np.array_equal(check_flags, host[2]) and np.array_equal(got[2], host[2]) and np.array_equal(got[3], host[3])
        assert np.array_equal(got[4], host[4])


def test_model_capacity(model):
    text, offs = nt.batch([nt.U(0x1D1C0) * 40, b"abc"])
    rc, got, _, _ = run_model(model, text, offs, 64, 0, cap=3 * 160 + 3 - 1)
    assert rc == 5 and got[4][0] == 483 and np.all(got[0] == 0xEE) and np.all(got[1] == -1)
    rc, got, _, _ = run_model(model, text, offs, 64, 0, cap=483)
    assert rc == 0 and len(got[0]) == 483


# ---- the host statement's contract -------------------------------------------------------------------------------------------------------

def test_argument_errors():
    lib = capi.load_library()
    text = np.frombuffer(nt.U(0x65, 0x301) * 4, dtype=np.uint8).copy()
    good = np.asarray([0, 6, 12], dtype=np.int64)

    def call(offs=good, n_docs=None, have_text=True, have_out=True, cap=64, have_counts=True, have_offs=True, out=None):
        o = np.ascontiguousarray(offs, dtype=np.int64)
        outb = np.full(64, 0xEE, dtype=np.uint8) if out is None else out
        ooff, counts = np.full(8, -1, dtype=np.int64), np.full(8, -1, dtype=np.int64)
        fl, ch = np.full(8, 7, dtype=np.uint8), np.full(8, 7, dtype=np.uint8)
        rc = lib.td_nfc_host(text.ctypes.data if have_text else None, o.ctypes.data if have_offs else None, len(o) - 1 if n_docs is None else n_docs,
                             outb.ctypes.data if have_out else None, cap, ooff.ctypes.data, fl.ctypes.data, ch.ctypes.data,
                             counts.ctypes.data if have_counts else None)
        untouched = np.all(outb[:64] == 0xEE) and np.all(ooff == -1) and np.all(fl == 7) and np.all(ch == 7) and np.all(counts == -1)
        return rc, untouched, counts

    rc, untouched, counts = call()
    assert rc == capi.TD_OK and not untouched and counts[0] == 8
    for kw in (dict(offs=[1, 6, 12]), dict(offs=[0, 7, 6]), dict(offs=[0, -1, 12]), dict(n_docs=-1), dict(have_text=False), dict(have_counts=False),
               dict(have_offs=False), dict(cap=-1), dict(have_out=False, cap=5), dict(out=text[4:]), dict(out=text)):
        rc, untouched, _ = call(**kw)
        assert rc == capi.TD_E_INVALID and (untouched or "out" in kw), kw
    # a NULL out with capacity 0: flags and counts alone
    rc, untouched, counts = call(have_out=False, cap=0)
    assert rc == capi.TD_OK and counts[0] == 8 and counts[1] == 2 and counts[2] == 2
    # an empty batch needs no text
    rc, _, counts = call(offs=[0, 0], have_text=False)
    assert rc == capi.TD_OK and counts[0] == 0
    with pytest.raises(capi.TokenDaggerHipError) as e:
        nfc_host(text, [0, 13])
    assert e.value.code == capi.TD_E_INVALID


def test_capacity_is_exact():
    text, offs = nt.batch([nt.U(0x1D1C0) * 100, nt.U(0x61, 0x301, 0x323) * 10, b"plain"])
    need = 3 * 400 + 5 * 10 + 5
    _, _, _, _, counts = nfc_host(text, offs, want_text=False)
    assert counts[0] == need
    with pytest.raises(capi.TokenDaggerHipError) as e:
        nfc_host(text, offs, capacity=need - 1)
    assert e.value.code == capi.TD_E_CAPACITY and e.value.counts[0] == need
    out, ooff, _, _, _ = nfc_host(text, offs, capacity=need)
    assert len(out) == need and ooff.tolist() == [0, 1200, 1250, 1255]
    # the 3 x bound is met exactly, and a capacity of 3 x the input always fits
    t3, o3 = nt.batch([nt.U(0x1D1C0) * 777])
    out, _, _, changed, counts = nfc_host(t3, o3)
    assert counts[0] == 3 * len(t3) == len(out) and changed.tolist() == [1]


@live
def test_nfc_text_is_left_alone_and_nfc_is_idempotent():
    for form in ("NFC", "NFD"):
        text, offs = nt.batch([nt.mixed(5000, form), nt.filler(100), nt.mixed(333, form)])
        out, ooff, flags, changed, counts = nfc_host(text, offs)
        if form == "NFC":
            assert bytes(out) == bytes(text) and np.array_equal(ooff, offs) and not changed.any() and counts[2] == 0
        else:
            assert changed.tolist() == [1, 0, 1] and flags.tolist() == [1, 0, 1] and len(out) < len(text)
        again = nfc_host(out, ooff)
        assert bytes(again[0]) == bytes(out) and np.array_equal(again[1], ooff) and not again[3].any()
