"""Loss labels without a GPU: the two truths of tests/labels_truth.py against each other, the CPU model of the kernels'
decomposition (tests/twin/labels_model.cpp over tokendagger_amd/csrc/td_labels.h) against the walk, the spec's checks and
the three symbols through the C ABI."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import labels_truth as lt

ROOT = Path(__file__).resolve().parents[1]


def _same(x, y):
    for k, (p, q) in enumerate(zip(x, y)):
        assert p.dtype == q.dtype and np.array_equal(p, q), (k, p, q)


def test_hand_worked_example():
    # opener [7, 8], closer 9; documents [0, 9), [9, 9), [9, 12), [12, 13)
    #        0  1  2  3  4  5  6  7  8 | 9 10 11 | 12
    ids = [1, 7, 8, 2, 3, 9, 4, 7, 8,   8, 5, 9,   7]
    offs = [0, 9, 9, 12, 13]
    # doc 0: the opener ends at 2 -> 3, 4 and the closer at 5 are trained; 6 is outside; the opener at 7, 8 starts a second span
    #        that the document's end leaves unterminated.  doc 2: "8" alone is no opener (the 7 belongs to document 0), its closer
    #        has no effect.  doc 3: a one-id document.
    want = np.asarray([-100, -100, -100, 2, 3, 9, -100, -100, -100, -100, -100, -100, -100], dtype=np.int32)
    for f in (lt.labels_walk, lt.labels_numpy):
        labels, mask, toff, counts = f(ids, offs, [[7, 8]], [9])
        assert np.array_equal(labels, want)
        assert np.array_equal(mask, (want != -100).astype(np.uint8))
        assert toff.tolist() == [0, 3, 3, 3, 3] and counts.tolist() == [3, 2, 1, 0]
        labels, _, toff, counts = f(ids, offs, [[7, 8]], [9], ignore_index=-1, train_close=False)
        assert labels.tolist() == [-1, -1, -1, 2, 3, -1, -1, -1, -1, -1, -1, -1, -1] and counts.tolist() == [2, 2, 1, 0]


def test_named_cases():
    for f in (lt.labels_walk, lt.labels_numpy):
        # an opener that overlaps itself: [5, 5] on 5, 5, 5 opens at 1 (and is content at 2)
        labels, _, _, counts = f([5, 5, 5, 1], [0, 4], [[5, 5]], [])
        assert labels.tolist() == [-100, -100, 5, 1] and counts.tolist() == [2, 1, 1, 0]
        # openers that are a prefix / a suffix of each other: [1, 2] and [1, 2, 3]; [2, 3] and [1, 2, 3]
        labels, _, _, counts = f([1, 2, 3, 4, 0, 4], [0, 6], [[1, 2, 3], [1, 2]], [0])
        assert labels.tolist() == [-100, -100, 3, 4, 0, -100] and counts.tolist() == [3, 1, 0, 0]
        labels, _, _, counts = f([9, 2, 3, 4, 0, 1, 2, 3, 4], [0, 9], [[1, 2, 3], [2, 3]], [0])
        assert labels.tolist() == [-100, -100, -100, 4, 0, -100, -100, -100, 4] and counts.tolist() == [3, 2, 1, 0]
        # an opener cut by a document start, empty documents around it
        labels, _, toff, counts = f([1, 2, 3, 3], [0, 0, 1, 1, 4, 4], [[1, 2]], [])
        assert labels.tolist() == [-100] * 4 and counts.tolist() == [0, 0, 0, 0] and toff.tolist() == [0] * 6
        # no closer at all: a span runs to the document's end
        labels, _, toff, counts = f([1, 4, 4, 1, 4], [0, 3, 5], [[1]], [])
        assert labels.tolist() == [-100, 4, 4, -100, 4] and counts.tolist() == [3, 2, 2, 0] and toff.tolist() == [0, 2, 3]


def test_walk_equals_numpy_on_random_cases():
    rng = np.random.default_rng(11)
    seen_spans = seen_unterm = 0
    for _ in range(400):
        ids, offs, open, close, tc = lt.random_case(rng)
        w = lt.labels_walk(ids, offs, open, close, -7, tc)
        _same(w, lt.labels_numpy(ids, offs, open, close, -7, tc))
        seen_spans += int(w[3][1])
        seen_unterm += int(w[3][2])
    assert seen_spans > 1000 and seen_unterm > 100


# ---- the CPU model over the shared header ---------------------------------------------------------------------------------
class LabSpec(ctypes.Structure):  # td::LabSpec (tokendagger_amd/csrc/td_labels.h)
    _fields_ = [("n_open", ctypes.c_int32), ("n_close", ctypes.c_int32), ("ignore", ctypes.c_int32), ("train_close", ctypes.c_int32),
                ("open_len", ctypes.c_int32 * 8), ("open_ids", (ctypes.c_int32 * 8) * 8), ("close_ids", ctypes.c_int32 * 16)]


@pytest.fixture(scope="module")
def model():
    src = ROOT / "tests" / "twin" / "labels_model.cpp"
    out = ROOT / "tests" / "twin" / "_build" / "liblabelsmodel.so"
    out.parent.mkdir(parents=True, exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", str(src), "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    lib.labels_model.restype = ctypes.c_int
    lib.labels_model.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

    def run(ids, offs, open, close, ignore, tc, tile, rng):
        sp = LabSpec()
        sp.n_open, sp.n_close, sp.ignore, sp.train_close = len(open), len(close), ignore, int(tc)
        for k, o in enumerate(open):
            sp.open_len[k] = len(o)
            for j, v in enumerate(o):
                sp.open_ids[k][j] = int(v)
        for k, c in enumerate(close):
            sp.close_ids[k] = int(c)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        total = int(offs[-1])
        order = rng.permutation(-(-total // tile)).astype(np.int64)
        labels = np.full(max(total, 1), 12345, dtype=np.int32)
        mask = np.full(max(total, 1), 77, dtype=np.uint8)
        toff = np.full(len(offs), -1, dtype=np.int64)
        counts = np.full(4, -1, dtype=np.int64)
        assert lib.labels_model(ids.ctypes.data, offs.ctypes.data, len(offs) - 1, ctypes.addressof(sp), tile, order.ctypes.data,
                                labels.ctypes.data, mask.ctypes.data, toff.ctypes.data, counts.ctypes.data) == 0
        return labels[:total], mask[:total], toff, counts
    return run


@pytest.mark.parametrize("tile", [1, 2, 7, 64, 4096])
def test_model_equals_walk(model, tile):
    rng = np.random.default_rng(100 + tile)
    for it in range(150):
        ids, offs, open, close, tc = lt.random_case(rng, max_docs=12 if it % 10 else 400, max_len=40 if it % 10 else 60)
        _same(model(ids, offs, open, close, -3, tc, tile, rng), lt.labels_walk(ids, offs, open, close, -3, tc))
    # one long document whose only events are at its start, and one without any
    n = 3 * 4096 + 5
    for ids in (np.concatenate([[1, 2], np.full(n, 3)]), np.full(n, 3)):
        _same(model(ids, [0, len(ids)], [[1, 2]], [0], -100, True, tile, rng), lt.labels_numpy(ids, [0, len(ids)], [[1, 2]], [0]))


# ---- the C ABI without a device ----------------------------------------------------------------------------------------------
def test_symbols_exported_and_declared():
    import __graft_entry__ as g
    g.build_hip()
    from tokendagger_amd import capi
    lib = capi.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tokendagger_hip.h").read_text(), flags=re.S)
    for n in ("td_span_labels", "td_span_labels_device", "td_encode_batch_span_labels"):
        assert hasattr(lib, n), n
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
        assert n in capi.EXPORTS
    assert ctypes.sizeof(capi.LabelsSpec) == 8 + 64 + 256 + 8 + 64 + 8 + 8


def _good():
    from tokendagger_amd import capi
    return capi.labels_spec([[1, 2, 3], [4]], [5, 6], -100, True)


def _edit(**kw):
    sp = _good()
    for k, v in kw.items():
        setattr(sp, k, v)
    return sp


def _bad_specs():
    sp = [("n_open = 0", _edit(n_open=0), "n_open"), ("n_open = 9", _edit(n_open=9), "n_open"), ("n_close = -1", _edit(n_close=-1), "n_close"),
          ("n_close = 17", _edit(n_close=17), "n_close"), ("ignore_index above int32", _edit(ignore_index=1 << 31), "ignore_index"),
          ("ignore_index below int32", _edit(ignore_index=-(1 << 31) - 1), "ignore_index"), ("unknown flags", _edit(flags=2), "flags")]
    for name, ln in (("open_len = 0", 0), ("open_len = 9", 9)):
        s = _good()
        s.open_len[1] = ln
        sp.append((name, s, "open_len"))
    s = _good()
    s.open_ids[0][1] = -2
    sp.append(("a negative opener id", s, "negative"))
    s = _good()
    s.close_ids[1] = -1
    sp.append(("a negative closer id", s, "negative"))
    s = _good()
    s.close_ids[0] = 2
    sp.append(("a closer inside an opener", s, "closer"))
    return sp


def test_spec_errors_are_invalid_before_the_handle_is_touched():
    """The spec is checked before the handle is looked at, so a handle that is only an address will do here: no device."""
    import __graft_entry__ as g
    g.build_hip()
    from tokendagger_amd import capi
    lib = capi.load_library()
    fake = ctypes.create_string_buffer(64)
    h = ctypes.c_void_p(ctypes.addressof(fake))
    offs = np.zeros(2, dtype=np.int64)
    buf = np.zeros(8, dtype=np.int64)
    cases = _bad_specs()
    assert len(cases) == 12
    for name, sp, word in cases:
        calls = [lib.td_span_labels(h, None, 0, offs.ctypes.data, 1, ctypes.byref(sp), None, None, None, buf.ctypes.data),
                 lib.td_span_labels_device(h, None, 0, offs.ctypes.data, 1, ctypes.byref(sp), None, None, None, buf.ctypes.data, None),
                 lib.td_encode_batch_span_labels(h, None, offs.ctypes.data, 1, None, None, 0, ctypes.byref(sp), None, 0, buf.ctypes.data, None,
                                                 None, None, buf.ctypes.data, None)]
        for rc in calls:
            assert rc == capi.TD_E_INVALID, (name, rc)
            assert word in lib.td_last_error(h).decode(), (name, lib.td_last_error(h))


def test_labels_spec_helper_limits():
    from tokendagger_amd import capi
    with pytest.raises(ValueError):
        capi.labels_spec([[1]] * 9, [])
    with pytest.raises(ValueError):
        capi.labels_spec([[1] * 9], [])
    with pytest.raises(ValueError):
        capi.labels_spec([[1]], list(range(2, 19)))
    sp = capi.labels_spec([[1, 2]], [], ignore_index=-1, train_close=False)
    assert (sp.n_open, sp.open_len[0], sp.n_close, sp.ignore_index, sp.flags) == (1, 2, 0, -1, 0)
