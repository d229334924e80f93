"""Text statistics without a GPU: the truth (tests/textstats_truth.py), td_text_stats_host through the C ABI and the CPU model of the
kernels' decomposition (tests/twin/textstats_model.cpp over tokendagger_amd/csrc/td_textstats_args.h: windows at every base shift, tiles
of 64, 256 and 4096 bytes, the tiles' carries, their prefix maxima, the lanes' walk) must all be EQUAL, on the frame's seams and on a few
thousand random small texts of an alphabet that makes events dense."""
import ctypes
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import textstats_truth as tt
from tokendagger_amd.capi import text_stats_host  # noqa: F401  (the feature under test: without it nothing here runs)

ROOT = Path(__file__).resolve().parents[1]
TILES = [64, 256, 4096]
GROUPS = [tt.LOCAL, tt.RUNS, tt.LOCAL | tt.RUNS]


@pytest.fixture(scope="module")
def model():
    csrc = ROOT / "tokendagger_amd" / "csrc"
    out = ROOT / "tests" / "twin" / "_build" / "libtextstatsmodel.so"
    out.parent.mkdir(parents=True, exist_ok=True)
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))  # (td_rewrite_args.h takes hipError_t from HIP's host header)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__",
                           f"-I{rocm / 'include'}", str(ROOT / "tests" / "twin" / "textstats_model.cpp"), str(csrc / "td_tables.cpp"),
                           str(csrc / "td_regex.cpp"), "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.textstats_model.restype = i32
    lib.textstats_model.argtypes = [vp, vp, i64, i32, i32, i32, vp, vp, vp]
    return lib


def run_model(lib, text, offs, groups, tile, shift=0):
    """-> (stats, totals, info)"""
    buf = np.frombuffer(bytes(text), dtype=np.uint8).copy() if len(text) else np.zeros(1, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    n_docs = len(offs) - 1
    stats = np.full((max(n_docs, 1), tt.COLS), -7, dtype=np.int64)
    totals, info = np.full(tt.COLS, -7, dtype=np.int64), np.zeros(4, dtype=np.int64)
    rc = lib.textstats_model(buf.ctypes.data, offs.ctypes.data, n_docs, groups, tile, shift, stats.ctypes.data, totals.ctypes.data, info.ctypes.data)
    assert rc == 0
    return stats[:n_docs], totals, info


@pytest.fixture(scope="module")
def cases():
    """Built once, shared and left unchanged: tile -> {name: (text, offsets, (stats, totals))}."""
    return {tile: {name: (text, offs, tt.truth(text, offs)) for name, (text, offs) in tt.limit_cases(tile).items()} for tile in TILES}


def _only(want, groups):
    stats, totals = want[0].copy(), want[1].copy()
    drop = [c for c in range(tt.COLS) if c not in ((tt.LOCAL_COLS if groups & tt.LOCAL else []) + (tt.RUNS_COLS if groups & tt.RUNS else []))]
    stats[:, drop] = 0
    totals[drop] = 0
    return stats, totals


def test_the_cases_say_what_they_are_named_for(cases):
    c = cases[4096]
    s = c["nothing leaks into the next document"][2][0]
    assert s[1, tt.WORDS_ALPHA] == 1 and s[1, tt.WORDS] == 2 and s[1, tt.END_TERMINAL] == 0 and s[0, tt.END_TERMINAL] == 1
    s = c["nothing leaks, at a tile seam"][2][0]
    assert s[1, tt.WORDS_ALPHA] == 0 and s[1, tt.END_TERMINAL] == 0 and s[1, tt.WORDS] == 1
    s = c["a word of three tiles, its letter first"][2][0]
    assert s[0, tt.WORDS_ALPHA] == 1 and s[0, tt.WORD_MAX] == 3 * 4096 + 1 and s[0, tt.WORDS] == 2
    s = c["a word of three tiles without a letter, then a letter"][2][0]
    assert s[0, tt.WORDS_ALPHA] == 1 and s[0, tt.WORDS] == 2
    s = c["a long line, spaces, LF"][2][0]
    assert s[0, tt.END_TERMINAL] == 2 and s[0, tt.LINE_MAX] == 5 * 4096 // 2 + 5000
    for k in range(3):
        s = c[f"three dots astride the seam +{k}"][2][0]
        assert s[0, tt.END_ELLIPSIS] == 1 and s[0, tt.ELLIPSES] == 1 and s[0, tt.LINES_BLANK] == 1
    s = c["a bullet behind spaces"][2][0]
    assert s[0, tt.START_BULLET] == 3 and s[0, tt.LINES] == 4
    assert c["only LFs"][2][0][0, tt.LINES] == 37 == c["only LFs"][2][0][0, tt.LINES_BLANK]
    assert c["a final line with no LF"][2][0][0, [tt.LINES, tt.END_TERMINAL]].tolist() == [3, 3]


@pytest.mark.parametrize("tile", TILES)
def test_host_and_model_equal_the_truth(model, cases, tile):
    seen = np.zeros(4, dtype=np.int64)
    for name, (text, offs, want) in cases[tile].items():
        for groups in GROUPS:
            w = _only(want, groups)
            got = text_stats_host(np.frombuffer(bytes(text), dtype=np.uint8), offs, groups)
            assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]), (name, groups, "host")
            shifts = range(16) if tile == 64 or len(text) <= 17 else (0, 5, 15)
            for shift in (shifts if groups == tt.LOCAL | tt.RUNS else (3,)):
                stats, totals, info = run_model(model, text, offs, groups, tile, shift)
                bad = np.argwhere(stats != w[0])
                assert len(bad) == 0, (name, groups, shift, bad[:4], stats[bad[0][0]], w[0][bad[0][0]])
                assert np.array_equal(totals, w[1]), (name, groups, shift)
                seen = np.maximum(seen, info)
    assert seen[0] >= 3 and seen[1] >= (2 if tile <= 256 else 1) and seen[2] > 0 and seen[3] > 0, seen


def test_random_small_texts(model):
    n = 0
    for text, offs in tt.random_small(7, 3000):
        want = tt.truth(text, offs)
        got = text_stats_host(np.frombuffer(text, dtype=np.uint8), offs)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (text, offs, got[0], want[0])
        shift = n % 16
        stats, totals, _ = run_model(model, text, offs, tt.LOCAL | tt.RUNS, 64, shift)
        assert np.array_equal(stats, want[0]) and np.array_equal(totals, want[1]), (text, offs, shift, stats, want[0])
        n += 1
    assert n == 3000


def test_the_big_case(model):
    text, offs = tt.big_case()
    want = tt.truth(text, offs)
    got = text_stats_host(np.frombuffer(text, dtype=np.uint8), offs)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    stats, totals, info = run_model(model, text, offs, tt.LOCAL | tt.RUNS, 4096, 9)
    assert np.array_equal(stats, want[0]) and np.array_equal(totals, want[1]) and info[0] > 256 and info[1] == 2
    one = np.asarray([0, len(text)], dtype=np.int64)
    want1 = tt.truth(text, one)
    stats, totals, _ = run_model(model, text, one, tt.LOCAL | tt.RUNS, 4096, 0)
    assert np.array_equal(stats, want1[0]) and np.array_equal(totals, want1[1])
