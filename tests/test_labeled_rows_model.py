"""Label rows without a GPU: the two truths of tests/labeled_rows_truth.py agree (the index stream through the existing row truths
against the slot-by-slot brute force), and the header declares the labeled entry points that the built library exports."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import labeled_rows_truth as lr

ROOT = Path(__file__).resolve().parents[1]

NEW_FUNCTIONS = ["td_make_rows_labeled", "td_make_rows_labeled_device", "td_pack_rows_labeled", "td_pack_rows_labeled_device",
                 "td_window_rows_labeled", "td_window_rows_labeled_device", "td_encode_batch_span_label_rows"]


@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_index_stream_truth_equals_brute_force(layout):
    rng = np.random.default_rng(100 + lr.LAYOUTS.index(layout))
    rows_seen = masked = 0
    for it in range(150):
        src, ids, offs, S, kw = lr.random_case(rng, layout)
        a = lr.label_rows(layout, src, offs, S, **kw)
        b = lr.label_rows_brute(layout, src, offs, S, **kw)
        assert a.dtype == b.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), (layout, it, S, kw, offs.tolist())
        # the id rows of the same placement have the same shape, and hold BOS / EOS / pad exactly where the label rows hold theirs
        r = lr.id_rows(layout, np.arange(len(src), dtype=np.int32) + 3, offs, S, 0 if kw["bos"] else -1, 1 if kw["eos"] else -1, 2,
                       kw.get("overlap", 0), kw.get("drop_last", False), kw.get("truncate", False))[0]
        assert r.shape == a.shape
        assert np.array_equal(a[r == 0], np.full((r == 0).sum(), kw["bos_value"], np.int32))
        assert np.array_equal(a[r == 1], np.full((r == 1).sum(), kw["eos_value"], np.int32))
        assert np.array_equal(a[r == 2], np.full((r == 2).sum(), kw["pad_value"], np.int32))
        rows_seen += a.shape[0]
        masked += bool(kw.get("mask_overlap")) and kw.get("overlap", 0) > 0
    assert rows_seen > 300
    if layout == "windows":
        assert masked > 20


def test_overlap_mask_trains_every_id_once():
    rng = np.random.default_rng(7)
    for it in range(60):
        n_docs = int(rng.integers(1, 6))
        lens = rng.integers(0, 90, n_docs)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        n = int(offs[-1])
        src = (np.arange(n) + 1000).astype(np.int32)  # (distinct, and none of the fill values)
        bos, eos = bool(it & 1), bool(it & 2)
        S = int(rng.integers(3 + bos + eos, 20))
        C = S - bos - eos
        for overlap in sorted({0, 1, C - 1}):
            kw = dict(bos=bos, eos=eos, bos_value=-1, eos_value=-2, pad_value=-3, overlap=overlap)
            on = lr.label_rows("windows", src, offs, S, mask_overlap=True, **kw)
            off = lr.label_rows("windows", src, offs, S, mask_overlap=False, **kw)
            assert np.array_equal(np.sort(on[on >= 1000]), src)
            assert (off >= 1000).sum() >= n and set(off[off >= 1000].tolist()) == set(src.tolist())
            if overlap == 0:
                assert np.array_equal(on, off)


def _declared():
    hdr = (ROOT / "include" / "tokendagger_hip.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return hdr, sorted(set(re.findall(r"\b(td_[a-z_]+)\s*\(", hdr)))


def test_header_declares_and_library_exports_the_labeled_entry_points():
    import __graft_entry__ as g
    g.build_hip()
    from tokendagger_amd import capi
    lib = capi.load_library()
    hdr, names = _declared()
    for fn in NEW_FUNCTIONS:
        assert fn in names, f"{fn} is not declared in include/tokendagger_hip.h"
        assert hasattr(lib, fn), f"{fn} declared but not exported"
        assert fn in capi.EXPORTS
    assert re.search(r"#define\s+TD_ROWLAB_MASK_OVERLAP\s+1\b", hdr)
    assert "typedef struct td_rows_labels" in hdr and "typedef struct td_label_rows_outputs" in hdr
    # the structs as ctypes sees them: six and eight 8-byte fields
    assert ctypes.sizeof(capi.RowsLabels) == 48 and ctypes.sizeof(capi.LabelRowsOutputs) == 64
    assert capi.TD_ROWLAB_MASK_OVERLAP == 1


def test_null_handle_is_invalid_not_a_crash():
    """With a null handle the labeled entry points return TD_E_INVALID, as their counterparts do (no device is needed to get there)."""
    import __graft_entry__ as g
    g.build_hip()
    from tokendagger_amd import capi
    lib = capi.load_library()
    spec = capi.rows_spec(8)
    lab = capi.rows_labels(1, 1)
    assert lib.td_make_rows_labeled(None, None, 0, None, 0, ctypes.byref(spec), None, 0, None, None, None, ctypes.byref(lab)) == capi.TD_E_INVALID
    assert lib.td_window_rows_labeled_device(None, None, 0, None, 0, ctypes.byref(spec), 0, None, 0, None, None, ctypes.byref(lab)) == capi.TD_E_INVALID
