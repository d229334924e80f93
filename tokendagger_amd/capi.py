"""ctypes view of the C ABI in include/tokendagger_hip.h (libtokendagger_hip.so).

This is the array-in / array-out surface used by bench.py, the GPU parity tests and the bulk
methods of `tokendagger_amd.Tokenizer`.  It performs no tokenization itself: every call goes to the
HIP library, and importing/constructing fails loudly when the library or a HIP device is missing.
"""
from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libtokendagger_hip.so"

TD_OK = 0
TD_E_CAPACITY = 5
TD_MODE_ENCODE = 0
TD_MODE_ORDINARY = 1
TD_E_INVALID = 1
TD_E_BAD_TOKEN = 8
TD_UNIT_BYTES, TD_UNIT_CHARS = 0, 1
TD_ROWS_CONCAT, TD_ROWS_PAD, TD_ROWS_BESTFIT, TD_ROWS_WINDOWS = 0, 1, 2, 3
TD_ROWS_DROP_LAST = 1
TD_ROWS_TRUNCATE = 2
TD_INFO_N_PAIRS, TD_INFO_MERGE_CLOSED, TD_INFO_MAX_ID, TD_INFO_TILE_BYTES = 1, 2, 3, 4
TD_INFO_WORKSPACE_BYTES, TD_INFO_N_SPECIAL, TD_INFO_LONG_PIECES, TD_INFO_FAR_PIECES = 5, 6, 7, 8
TD_OPT_LONG_POOL_BYTES = 1
TD_OPT_PROFILE = 2
TD_OPT_PIPE_CHUNK_BYTES = 3
TD_OPT_PIPE_THREADS = 4
TD_OPT_SMALL_PATH = 5
TD_OPT_FUSED = 6
TD_OPT_GRAPH = 7
TD_OPT_DEVICE_SPECIALS = 8
TD_OPT_DIRECT = 9
TD_OPT_PACK_SPLIT = 10
TD_OPT_DEDUPE = 11
TD_OPT_OVERLAP = 12
TD_OPT_GIANT_COOP_MIN = 13
TD_OPT_SPARSE = 14
TD_OPT_COUNTS_SEATS = 15
TD_OPT_COUNTS_FLUSH_TILES = 16
TD_COUNTS_ACCUMULATE = 1
TD_OPT_NGRAM_TAG_BITS = 17
TD_NGRAM_ACCUMULATE = 1
TD_NGRAM_MAX_LEN, TD_NGRAM_MAX_LENGTHS = 64, 8
TD_MINHASH_MAX_PERM = 1024
TD_NGRAM_INFO = {"patterns": 1, "distinct": 2, "lengths": 3, "max_len": 4, "slots": 5, "max_probe": 6, "device_bytes": 7}
TD_INFO_DEFERRED_TILES, TD_INFO_FLAGGED_TILES = 9, 10
TD_INFO_DIRECT_TILES = 11
TD_INFO_LB_TIMEOUTS = 12
TD_INFO_REPEATS, TD_INFO_LISTED_PIECES, TD_INFO_CHAR_SEEDS = 13, 14, 15
TD_INFO_SPARSE = 16
TD_OPT_WS_FILL = 18  # debugging: -1 off, 0..255 the byte every workspace buffer is filled with at allocation and before every step
TD_INFO_WS_FILLED_BYTES = 17
# which path answered the handle's small host calls since it was made: the one-launch kernels themselves, or the general path they handed to
TD_INFO_SMALL_ENCODES, TD_INFO_SMALL_ENCODE_HANDBACKS, TD_INFO_SMALL_DECODES, TD_INFO_SMALL_DECODE_HANDBACKS = 18, 19, 20, 21

EXPORTS = [
    "td_create", "td_clone", "td_destroy", "td_last_error", "td_encode_batch", "td_encode_device", "td_reserve",
    "td_device_status", "td_decode_bytes", "td_encode_with_special", "td_info", "td_set_option",
    "td_special_count", "td_special_get", "td_profile_read",
    "td_vocab_create", "td_vocab_destroy", "td_vocab_error", "td_vocab_load_tiktoken", "td_vocab_load_hf_special",
    "td_vocab_load_tekken", "td_vocab_load_json", "td_vocab_set_pattern", "td_vocab_pattern", "td_vocab_arrays",
    "td_create_from_vocab", "td_token_bytes", "td_single_token", "td_decode_device", "td_decode_batch", "td_encode_batch_with_special",
    "td_encode_with_special_strs", "td_encode_batch_with_special_strs", "td_profile_read_ex", "td_profile_segment_name",
    "td_comm_unique_id", "td_comm_create", "td_comm_destroy", "td_comm_gather_counts", "td_comm_bases", "td_comm_gather_tokens",
    "td_comm_last_error", "td_encode_device_with_special", "td_token_starts", "td_token_starts_device", "td_encode_batch_with_starts",
    "td_encode_device_with_starts", "td_make_rows_device", "td_make_rows", "td_encode_batch_rows",
    "td_pack_plan", "td_pack_rows", "td_pack_rows_device", "td_encode_batch_pack_rows",
    "td_window_plan", "td_window_rows", "td_window_rows_device", "td_encode_batch_window_rows",
    "td_span_labels", "td_span_labels_device", "td_encode_batch_span_labels",
    "td_make_rows_labeled", "td_make_rows_labeled_device", "td_pack_rows_labeled", "td_pack_rows_labeled_device",
    "td_window_rows_labeled", "td_window_rows_labeled_device", "td_encode_batch_span_label_rows",
    "td_select_plan", "td_select_docs", "td_select_docs_device", "td_encode_batch_select",
    "td_join_plan", "td_join_fields", "td_join_fields_device", "td_encode_batch_join",
    "td_range_plan", "td_range_labels", "td_range_labels_device", "td_encode_batch_range_labels", "td_encode_batch_range_label_rows",
    "td_token_counts_host", "td_token_counts", "td_token_counts_device", "td_encode_batch_token_counts",
    "td_decode_rows_check", "td_decode_rows", "td_decode_rows_device",
    "td_ngram_set_create", "td_ngram_set_destroy", "td_ngram_set_info", "td_ngram_matches_host", "td_ngram_matches_device",
    "td_ngram_matches", "td_encode_batch_ngram_matches",
    "td_minhash_params", "td_minhash_host", "td_minhash_device", "td_minhash", "td_encode_batch_minhash",
    "td_nfc_info", "td_nfc_host", "td_nfc_check_device", "td_nfc_device", "td_nfc", "td_encode_batch_nfc",
    "td_text_stats_host", "td_text_stats_device", "td_text_stats", "td_encode_batch_text_stats",
]


class TokenDaggerHipError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


_lib = None


def _share_hip_runtime_with_torch():
    """One process must not hold two HIP runtimes: PyTorch-ROCm wheels bundle their own libamdhip64.so.7 +
    libhsa-runtime64, and a second copy (the system one this library is linked against) cannot see the GPU
    once the first has claimed it.  When torch is installed, load ITS runtime first, globally, so that our
    DT_NEEDED libamdhip64.so.7 binds to it.  Set TOKENDAGGER_NO_TORCH=1 to use the system ROCm runtime."""
    import os
    if os.environ.get("TOKENDAGGER_NO_TORCH") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        hip = Path(list(spec.submodule_search_locations)[0]) / "lib" / "libamdhip64.so"
        if hip.exists():
            import torch  # noqa: F401  (loads the bundled runtime with the right rpaths)
            ctypes.CDLL(str(hip), mode=ctypes.RTLD_GLOBAL)
    except Exception:  # torch broken or absent: fall back to the system runtime
        return


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    import os
    lib_path = Path(os.environ.get("TD_HIP_LIB", str(LIB_PATH)))  # TD_HIP_LIB: kernel-tuning builds only
    if not lib_path.exists():
        raise ImportError(
            f"{lib_path} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'); "
            "tokendagger_amd has no CPU fallback")
    _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(str(lib_path), mode=ctypes.RTLD_GLOBAL)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.td_encode_device_with_special.restype = i32
    lib.td_encode_device_with_special.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp]
    lib.td_token_starts.restype = i32
    lib.td_token_starts.argtypes = [vp, vp, i64, vp, i64, i32, vp]
    lib.td_token_starts_device.restype = i32
    lib.td_token_starts_device.argtypes = [vp, vp, i64, vp, i64, i32, vp, vp]
    lib.td_encode_batch_with_starts.restype = i32
    lib.td_encode_batch_with_starts.argtypes = [vp, vp, vp, i64, i32, vp, vp, i64, i32, vp, i64, vp, vp, ctypes.POINTER(i64)]
    lib.td_encode_device_with_starts.restype = i32
    lib.td_encode_device_with_starts.argtypes = [vp, vp, i64, vp, i64, i32, i32, vp, i64, vp, vp, vp]
    lib.td_make_rows_device.restype = i32
    lib.td_make_rows_device.argtypes = [vp, vp, i64, vp, i64, vp, vp, i64, vp, vp, vp, vp]
    lib.td_make_rows.restype = i32
    lib.td_make_rows.argtypes = [vp, vp, i64, vp, i64, vp, vp, i64, vp, vp, vp]
    lib.td_encode_batch_rows.restype = i32
    lib.td_encode_batch_rows.argtypes = [vp, vp, vp, i64, i32, vp, vp, i64, vp, vp, vp]
    lib.td_pack_plan.restype = i32
    lib.td_pack_plan.argtypes = [vp, i64, vp, vp, vp, vp]
    lib.td_pack_rows.restype = i32
    lib.td_pack_rows.argtypes = [vp, vp, i64, vp, i64, vp, vp, i64, vp]
    lib.td_pack_rows_device.restype = i32
    lib.td_pack_rows_device.argtypes = [vp, vp, i64, vp, i64, vp, vp, i64, vp, vp]
    lib.td_encode_batch_pack_rows.restype = i32
    lib.td_encode_batch_pack_rows.argtypes = [vp, vp, vp, i64, i32, vp, vp, i64, vp]
    lib.td_window_plan.restype = i32
    lib.td_window_plan.argtypes = [vp, i64, vp, i64, vp, vp]
    lib.td_window_rows.restype = i32
    lib.td_window_rows.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp]
    lib.td_window_rows_device.restype = i32
    lib.td_window_rows_device.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp]
    lib.td_encode_batch_window_rows.restype = i32
    lib.td_encode_batch_window_rows.argtypes = [vp, vp, vp, i64, i32, vp, i64, vp, i64, vp]
    lib.td_span_labels_device.restype = i32
    lib.td_span_labels_device.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp]
    lib.td_span_labels.restype = i32
    lib.td_span_labels.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp, vp]
    lib.td_encode_batch_span_labels.restype = i32
    lib.td_encode_batch_span_labels.argtypes = [vp, vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, ctypes.POINTER(i64)]
    for fn, base in (("td_make_rows_labeled", lib.td_make_rows), ("td_make_rows_labeled_device", lib.td_make_rows_device),
                     ("td_pack_rows_labeled", lib.td_pack_rows), ("td_pack_rows_labeled_device", lib.td_pack_rows_device),
                     ("td_window_rows_labeled", lib.td_window_rows), ("td_window_rows_labeled_device", lib.td_window_rows_device)):
        getattr(lib, fn).restype = i32
        getattr(lib, fn).argtypes = [*base.argtypes, vp]  # (the counterpart's signature and a trailing td_rows_labels)
    lib.td_encode_batch_span_label_rows.restype = i32
    lib.td_encode_batch_span_label_rows.argtypes = [vp, vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp]
    lib.td_select_plan.restype = i32
    lib.td_select_plan.argtypes = [vp, i64, vp, i64, vp, vp, vp, vp]
    lib.td_select_docs_device.restype = i32
    lib.td_select_docs_device.argtypes = [vp, vp, vp, i64, vp, i64, vp, i64, vp, vp, vp, i64, vp, vp, vp, vp]
    lib.td_select_docs.restype = i32
    lib.td_select_docs.argtypes = [vp, vp, vp, i64, vp, i64, vp, i64, vp, vp, vp, i64, vp, vp, vp]
    lib.td_encode_batch_select.restype = i32
    lib.td_encode_batch_select.argtypes = [vp, vp, vp, i64, i32, vp, i64, vp, vp, i64, vp, vp, vp]
    lib.td_join_plan.restype = i32
    lib.td_join_plan.argtypes = [vp, i64, vp, vp, vp, vp, vp]
    lib.td_join_fields_device.restype = i32
    lib.td_join_fields_device.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp]
    lib.td_join_fields.restype = i32
    lib.td_join_fields.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp]
    lib.td_encode_batch_join.restype = i32
    lib.td_encode_batch_join.argtypes = [vp, vp, vp, i64, i32, vp, vp, vp]
    lib.td_range_plan.restype = i32
    lib.td_range_plan.argtypes = [vp, vp, i64, vp, vp, ctypes.POINTER(i64)]
    lib.td_range_labels_device.restype = i32
    lib.td_range_labels_device.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]
    lib.td_range_labels.restype = i32
    lib.td_range_labels.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.td_encode_batch_range_labels.restype = i32
    lib.td_encode_batch_range_labels.argtypes = [vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, ctypes.POINTER(i64)]
    lib.td_encode_batch_range_label_rows.restype = i32
    lib.td_encode_batch_range_label_rows.argtypes = [vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, i64, vp, vp]
    lib.td_token_counts_host.restype = i32
    lib.td_token_counts_host.argtypes = [vp, i64, vp, i64, vp, vp, vp, vp]
    lib.td_token_counts_device.restype = i32
    lib.td_token_counts_device.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp, vp]
    lib.td_token_counts.restype = i32
    lib.td_token_counts.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp]
    lib.td_decode_rows_check.restype = i32
    lib.td_decode_rows_check.argtypes = [vp, i64, vp, vp, i64, ctypes.POINTER(i64)]
    lib.td_decode_rows.restype = i32
    lib.td_decode_rows.argtypes = [vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp, vp, ctypes.POINTER(i64)]
    lib.td_decode_rows_device.restype = i32
    lib.td_decode_rows_device.argtypes = [vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp]
    lib.td_ngram_set_create.restype = i32
    lib.td_ngram_set_create.argtypes = [vp, vp, vp, i64, ctypes.POINTER(vp)]
    lib.td_ngram_set_destroy.restype = None
    lib.td_ngram_set_destroy.argtypes = [vp]
    lib.td_ngram_set_info.restype = i64
    lib.td_ngram_set_info.argtypes = [vp, i32]
    lib.td_ngram_matches_host.restype = i32
    lib.td_ngram_matches_host.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp]
    lib.td_ngram_matches_device.restype = i32
    lib.td_ngram_matches_device.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    lib.td_ngram_matches.restype = i32
    lib.td_ngram_matches.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp]
    lib.td_encode_batch_ngram_matches.restype = i32
    lib.td_encode_batch_ngram_matches.argtypes = [vp, vp, vp, i64, i32, vp, vp, vp, vp, vp, ctypes.POINTER(i64)]
    lib.td_minhash_params.restype = i32
    lib.td_minhash_params.argtypes = [ctypes.c_uint64, i64, vp, vp]
    lib.td_minhash_host.restype = i32
    lib.td_minhash_host.argtypes = [vp, i64, vp, i64, vp, vp, vp, vp]
    lib.td_minhash_device.restype = i32
    lib.td_minhash_device.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp, vp]
    lib.td_minhash.restype = i32
    lib.td_minhash.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp]
    lib.td_encode_batch_minhash.restype = i32
    lib.td_encode_batch_minhash.argtypes = [vp, vp, vp, i64, i32, vp, vp, vp, vp, ctypes.POINTER(i64)]
    lib.td_nfc_info.restype = i64
    lib.td_nfc_info.argtypes = [i32]
    lib.td_nfc_host.restype = i32
    lib.td_nfc_host.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp]
    lib.td_nfc_check_device.restype = i32
    lib.td_nfc_check_device.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp]
    lib.td_nfc_device.restype = i32
    lib.td_nfc_device.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, vp, vp, vp]
    lib.td_nfc.restype = i32
    lib.td_nfc.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, vp, vp]
    lib.td_encode_batch_nfc.restype = i32
    lib.td_encode_batch_nfc.argtypes = [vp, vp, vp, i64, i32, vp, i64, vp, vp, i64, vp, vp, vp]
    lib.td_utf8_host.restype = i32
    lib.td_utf8_host.argtypes = [vp, vp, i64, i32, vp, i64, vp, vp, vp, vp, vp]
    lib.td_utf8_check_device.restype = i32
    lib.td_utf8_check_device.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp]
    lib.td_utf8_device.restype = i32
    lib.td_utf8_device.argtypes = [vp, vp, i64, vp, i64, i32, vp, i64, vp, vp, vp, vp, vp, vp]
    lib.td_utf8.restype = i32
    lib.td_utf8.argtypes = [vp, vp, vp, i64, i32, vp, i64, vp, vp, vp, vp, vp]
    lib.td_encode_batch_utf8.restype = i32
    lib.td_encode_batch_utf8.argtypes = [vp, vp, vp, i64, i32, i32, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp]
    lib.td_text_stats_host.restype = i32
    lib.td_text_stats_host.argtypes = [vp, vp, i64, i32, vp, vp]
    lib.td_text_stats_device.restype = i32
    lib.td_text_stats_device.argtypes = [vp, vp, i64, vp, i64, i32, vp, vp, vp]
    lib.td_text_stats.restype = i32
    lib.td_text_stats.argtypes = [vp, vp, vp, i64, i32, vp, vp]
    lib.td_encode_batch_text_stats.restype = i32
    lib.td_encode_batch_text_stats.argtypes = [vp, vp, vp, i64, i32, i32, vp, i64, vp, vp, vp]
    lib.td_encode_batch_token_counts.restype = i32
    lib.td_encode_batch_token_counts.argtypes = [vp, vp, vp, i64, i32, vp, vp, vp, vp, ctypes.POINTER(i64)]
    lib.td_comm_unique_id.restype = i32
    lib.td_comm_unique_id.argtypes = [vp]
    lib.td_comm_create.restype = i32
    lib.td_comm_create.argtypes = [vp, i32, i32, i32, ctypes.POINTER(vp)]
    lib.td_comm_destroy.argtypes = [vp]
    lib.td_comm_gather_counts.restype = i32
    lib.td_comm_gather_counts.argtypes = [vp, vp, vp, vp]
    lib.td_comm_bases.restype = i32
    lib.td_comm_bases.argtypes = [vp, i32, i32, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64)]
    lib.td_comm_gather_tokens.restype = i32
    lib.td_comm_gather_tokens.argtypes = [vp, vp, vp, i32, vp, i64, vp]
    lib.td_comm_last_error.restype = ctypes.c_char_p
    lib.td_create.restype = i32
    lib.td_create.argtypes = [ctypes.c_char_p, i64, vp, vp, vp, i64, vp, vp, vp, i32, ctypes.POINTER(vp)]
    lib.td_destroy.argtypes = [vp]
    lib.td_clone.restype = i32
    lib.td_clone.argtypes = [vp, ctypes.POINTER(vp)]
    lib.td_last_error.restype = ctypes.c_char_p
    lib.td_last_error.argtypes = [vp]
    lib.td_encode_batch.restype = i32
    lib.td_encode_batch.argtypes = [vp, vp, vp, i64, i32, vp, i64, vp, ctypes.POINTER(i64)]
    lib.td_encode_device.restype = i32
    lib.td_encode_device.argtypes = [vp, vp, i64, vp, i64, i32, vp, i64, vp, vp]
    lib.td_reserve.restype = i32
    lib.td_reserve.argtypes = [vp, i64, i64]
    lib.td_device_status.restype = i32
    lib.td_device_status.argtypes = [vp, vp, ctypes.POINTER(i64)]
    lib.td_decode_bytes.restype = i32
    lib.td_decode_bytes.argtypes = [vp, vp, i64, vp, i64, ctypes.POINTER(i64)]
    lib.td_encode_with_special.restype = i32
    lib.td_encode_with_special.argtypes = [vp, vp, i64, vp, i64, vp, i64, ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_int32)]
    lib.td_info.restype = i64
    lib.td_info.argtypes = [vp, i32]
    lib.td_set_option.restype = i32
    lib.td_set_option.argtypes = [vp, i32, i64]
    lib.td_profile_read.restype = i32
    lib.td_profile_read.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64)]
    lib.td_profile_read_ex.restype = i32
    lib.td_profile_read_ex.argtypes = [vp, ctypes.POINTER(ctypes.c_double), i32, ctypes.POINTER(i64)]
    lib.td_profile_segment_name.restype = ctypes.c_char_p
    lib.td_profile_segment_name.argtypes = [i32]
    lib.td_special_count.restype = i64
    lib.td_special_count.argtypes = [vp]
    lib.td_special_get.restype = i32
    lib.td_special_get.argtypes = [vp, i64, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_int32)]
    lib.td_encode_batch_with_special.restype = i32
    lib.td_encode_batch_with_special.argtypes = [vp, vp, vp, i64, vp, i64, vp, i64, vp, ctypes.POINTER(i64)]
    lib.td_encode_with_special_strs.restype = i32
    lib.td_encode_with_special_strs.argtypes = [vp, vp, i64, vp, vp, i64, vp, i64, ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_int32)]
    lib.td_encode_batch_with_special_strs.restype = i32
    lib.td_encode_batch_with_special_strs.argtypes = [vp, vp, vp, i64, vp, vp, i64, vp, i64, vp, ctypes.POINTER(i64)]
    lib.td_decode_batch.restype = i32
    lib.td_decode_batch.argtypes = [vp, vp, vp, i64, vp, i64, vp, ctypes.POINTER(i64)]
    lib.td_decode_device.restype = i32
    lib.td_decode_device.argtypes = [vp, vp, i64, vp, i64, vp, vp]
    lib.td_token_bytes.restype = i32
    lib.td_token_bytes.argtypes = [vp, ctypes.c_int32, ctypes.POINTER(vp), ctypes.POINTER(i64)]
    lib.td_single_token.restype = i32
    lib.td_single_token.argtypes = [vp, vp, i64, ctypes.POINTER(ctypes.c_int32)]
    lib.td_vocab_create.restype = i32
    lib.td_vocab_create.argtypes = [ctypes.POINTER(vp)]
    lib.td_vocab_destroy.argtypes = [vp]
    lib.td_vocab_error.restype = ctypes.c_char_p
    lib.td_vocab_error.argtypes = [vp]
    for fn in ("td_vocab_load_tiktoken", "td_vocab_load_tekken", "td_vocab_set_pattern"):
        getattr(lib, fn).restype = i32
        getattr(lib, fn).argtypes = [vp, ctypes.c_char_p]
    lib.td_vocab_load_hf_special.restype = i32
    lib.td_vocab_load_hf_special.argtypes = [vp, ctypes.c_char_p, i32]
    lib.td_vocab_load_json.restype = i32
    lib.td_vocab_load_json.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p]
    lib.td_vocab_pattern.restype = ctypes.c_char_p
    lib.td_vocab_pattern.argtypes = [vp]
    lib.td_vocab_arrays.restype = i32
    lib.td_vocab_arrays.argtypes = [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(i64)]
    lib.td_create_from_vocab.restype = i32
    lib.td_create_from_vocab.argtypes = [vp, i32, ctypes.POINTER(vp)]
    _lib = lib
    return lib


def _pack(items: list[tuple[bytes, int]]):
    ranks = np.asarray([r for _, r in items], dtype=np.int32)
    offs = np.zeros(len(items) + 1, dtype=np.int64)
    if items:
        np.cumsum([len(b) for b, _ in items], out=offs[1:])
    blob = np.frombuffer(b"".join(b for b, _ in items) or b"\0", dtype=np.uint8).copy()
    return blob, offs, ranks


class RowsSpec(ctypes.Structure):
    """td_rows_spec (include/tokendagger_hip.h): -1 for no BOS / EOS."""
    _fields_ = [("layout", ctypes.c_int64), ("seq_len", ctypes.c_int64), ("bos_id", ctypes.c_int64), ("eos_id", ctypes.c_int64),
                ("pad_id", ctypes.c_int64), ("flags", ctypes.c_int64)]


def rows_spec(seq_len: int, layout: int = TD_ROWS_CONCAT, bos: int = -1, eos: int = -1, pad: int = 0, drop_last: bool = False) -> RowsSpec:
    return RowsSpec(layout, seq_len, bos, eos, pad, TD_ROWS_DROP_LAST if drop_last else 0)


def rows_capacity_of(spec: RowsSpec, n_ids: int, n_docs: int) -> int:
    """The rows td_make_rows writes for n_ids ids in n_docs documents."""
    if spec.layout == TD_ROWS_PAD:
        return n_docs
    t = n_ids + n_docs * ((spec.bos_id >= 0) + (spec.eos_id >= 0))
    return t // spec.seq_len if spec.flags & TD_ROWS_DROP_LAST else -(-t // spec.seq_len)


class PackOutputs(ctypes.Structure):
    """td_pack_outputs (include/tokendagger_hip.h): addresses, 0 / None for an output not wanted."""
    _fields_ = [("ids", ctypes.c_void_p), ("positions", ctypes.c_void_p), ("cu_seqlens", ctypes.c_void_p), ("row_lengths", ctypes.c_void_p),
                ("seg_docs", ctypes.c_void_p)]


def pack_spec(seq_len: int, bos: int = -1, eos: int = -1, pad: int = 0, truncate: bool = False) -> RowsSpec:
    """A TD_ROWS_BESTFIT spec: whole documents packed into rows by best-fit decreasing."""
    return RowsSpec(TD_ROWS_BESTFIT, seq_len, bos, eos, pad, TD_ROWS_TRUNCATE if truncate else 0)


def pack_rows_capacity_of(spec: RowsSpec, n_ids: int, n_docs: int) -> int:
    """A bound on the rows td_pack_rows writes without planning first: floor(2 T / S) + 1, T = n_ids + n_docs * (b + e)."""
    t = n_ids + n_docs * ((spec.bos_id >= 0) + (spec.eos_id >= 0))
    return 2 * t // spec.seq_len + 1


def pack_plan(tok_offsets, spec: RowsSpec, placement: bool = False):
    """td_pack_plan (host only, no device): counts int64[4] = rows, real slots, segments, documents cut; with placement=True
    also (doc_row, doc_slot) int64[n_docs], where each document's packed chunk sits (-1: none)."""
    lib = load_library()
    o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
    n_docs = len(o) - 1
    if n_docs < 0:
        raise ValueError("tok_offsets must have n_docs + 1 entries")
    counts = np.zeros(4, dtype=np.int64)
    row = np.empty(max(n_docs, 1), dtype=np.int64) if placement else None
    slot = np.empty(max(n_docs, 1), dtype=np.int64) if placement else None
    rc = lib.td_pack_plan(o.ctypes.data, n_docs, ctypes.byref(spec), counts.ctypes.data, row.ctypes.data if placement else None,
                          slot.ctypes.data if placement else None)
    if rc != TD_OK:
        raise TokenDaggerHipError(rc, "td_pack_plan: invalid spec or tok_offsets")
    return (counts, row[:n_docs], slot[:n_docs]) if placement else counts


class WindowOutputs(ctypes.Structure):
    """td_window_outputs (include/tokendagger_hip.h): addresses, 0 / None for an output not wanted."""
    _fields_ = [("ids", ctypes.c_void_p), ("positions", ctypes.c_void_p), ("row_lengths", ctypes.c_void_p), ("row_docs", ctypes.c_void_p),
                ("row_starts", ctypes.c_void_p)]


def windows_spec(seq_len: int, bos: int = -1, eos: int = -1, pad: int = 0) -> RowsSpec:
    """A TD_ROWS_WINDOWS spec: one document per row, a longer document continues in overlapping rows of its own."""
    return RowsSpec(TD_ROWS_WINDOWS, seq_len, bos, eos, pad, 0)


def window_plan(tok_offsets, spec: RowsSpec, overlap: int = 0, first_row: bool = False):
    """td_window_plan (host only, no device): counts int64[4] = rows, real slots, documents with more than one window, the
    largest window count; with first_row=True also first_row int64[n_docs + 1], the first row of every document."""
    lib = load_library()
    o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
    n_docs = len(o) - 1
    if n_docs < 0:
        raise ValueError("tok_offsets must have n_docs + 1 entries")
    counts = np.zeros(4, dtype=np.int64)
    fr = np.empty(n_docs + 1, dtype=np.int64) if first_row else None
    rc = lib.td_window_plan(o.ctypes.data, n_docs, ctypes.byref(spec), overlap, counts.ctypes.data, fr.ctypes.data if first_row else None)
    if rc != TD_OK:
        raise TokenDaggerHipError(rc, "td_window_plan: invalid spec, overlap or tok_offsets")
    return (counts, fr) if first_row else counts


TD_ROWLAB_MASK_OVERLAP = 1


class RowsLabels(ctypes.Structure):
    """td_rows_labels (include/tokendagger_hip.h): the label stream of a labeled row call.  src / dst are addresses."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("bos_value", ctypes.c_int64), ("eos_value", ctypes.c_int64),
                ("pad_value", ctypes.c_int64), ("flags", ctypes.c_int64)]


def rows_labels(src: int = 0, dst: int = 0, bos_value: int = -100, eos_value: int = -100, pad_value: int = -100,
                mask_overlap: bool = False, flags: int | None = None) -> RowsLabels:
    """src / dst: raw addresses (0: NULL); flags: given as they are when not None (the library checks them)."""
    return RowsLabels(src or None, dst or None, bos_value, eos_value, pad_value,
                      flags if flags is not None else (TD_ROWLAB_MASK_OVERLAP if mask_overlap else 0))


class LabelRowsOutputs(ctypes.Structure):
    """td_label_rows_outputs (include/tokendagger_hip.h): addresses, None for an output not wanted or not of the layout."""
    _fields_ = [("ids", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("positions", ctypes.c_void_p), ("aux", ctypes.c_void_p),
                ("row_lengths", ctypes.c_void_p), ("seg_docs", ctypes.c_void_p), ("row_docs", ctypes.c_void_p), ("row_starts", ctypes.c_void_p)]


TD_LABELS_MAX_OPEN, TD_LABELS_MAX_OPEN_LEN, TD_LABELS_MAX_CLOSE, TD_LABELS_TRAIN_CLOSE = 8, 8, 16, 1


class SelectSpec(ctypes.Structure):
    """td_select_spec (include/tokendagger_hip.h)."""
    _fields_ = [("min_len", ctypes.c_int64), ("max_len", ctypes.c_int64), ("flags", ctypes.c_int64)]


def select_spec(min_len: int = 0, max_len: int | None = None, flags: int = 0) -> SelectSpec:
    """Listed documents with fewer than min_len or more than max_len ids are dropped; max_len None (or -1): no limit."""
    return SelectSpec(min_len, -1 if max_len is None else max_len, flags)


def _sel_array(sel):
    if sel is None:
        return None
    a = np.ascontiguousarray(sel, dtype=np.int64)
    return a if a.size else np.zeros(1, dtype=np.int64)[:0]  # (an empty list is not the identity: its address is not NULL)


def select_plan(tok_offsets, sel=None, spec: SelectSpec | None = None, outputs: bool = True):
    """td_select_plan (host only, no device): counts int64[4] = kept entries K, kept ids T, entries dropped below min_len, above
    max_len; with outputs=True also out_offsets int64[K + 1] and out_docs int64[K].  sel None: the identity.  An error carries
    .counts ([0]: the position of a bad entry, -1 for an argument error)."""
    lib = load_library()
    spec = spec if spec is not None else select_spec()
    o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
    n_docs = len(o) - 1
    if n_docs < 0:
        raise ValueError("tok_offsets must have n_docs + 1 entries")
    sl = _sel_array(sel)
    n_sel = n_docs if sl is None else len(sl)
    counts = np.zeros(4, dtype=np.int64)
    offs = np.empty(n_sel + 1, dtype=np.int64) if outputs else None
    docs = np.empty(max(n_sel, 1), dtype=np.int64) if outputs else None
    rc = lib.td_select_plan(o.ctypes.data, n_docs, sl.ctypes.data if sl is not None else None, n_sel, ctypes.byref(spec), counts.ctypes.data,
                            offs.ctypes.data if outputs else None, docs.ctypes.data if outputs else None)
    if rc != TD_OK:
        ex = TokenDaggerHipError(rc, "td_select_plan: invalid spec or arguments" if counts[0] < 0 else
                                 f"td_select_plan: sel[{int(counts[0])}] is not a document in 0 .. n_docs - 1 with valid offsets")
        ex.counts = counts
        raise ex
    k = int(counts[0])
    return (counts, offs[:k + 1], docs[:k]) if outputs else counts


TD_JOIN_MAX_FIELDS, TD_JOIN_MAX_LITERAL = 8, 16
TD_JOIN_KEEP_TAIL, TD_JOIN_TRAIN, TD_JOIN_TRAIN_BEFORE = 1, 2, 4  # td_join_field.flags
TD_JOIN_FIELD_MAJOR, TD_JOIN_TRAIN_TAIL = 1, 2                    # td_join_spec.flags
TD_JOIN_SHRINK_ORDER, TD_JOIN_SHRINK_LONGEST = 0, 1


class JoinField(ctypes.Structure):
    """td_join_field (include/tokendagger_hip.h)."""
    _fields_ = [("before", ctypes.c_int64 * TD_JOIN_MAX_LITERAL), ("n_before", ctypes.c_int64), ("max_len", ctypes.c_int64),
                ("shrink_rank", ctypes.c_int64), ("type_value", ctypes.c_int64), ("flags", ctypes.c_int64)]


class JoinSpec(ctypes.Structure):
    """td_join_spec (include/tokendagger_hip.h)."""
    _fields_ = [("n_fields", ctypes.c_int64), ("fields", JoinField * TD_JOIN_MAX_FIELDS), ("tail", ctypes.c_int64 * TD_JOIN_MAX_LITERAL),
                ("n_tail", ctypes.c_int64), ("tail_type", ctypes.c_int64), ("max_total", ctypes.c_int64), ("shrink", ctypes.c_int64),
                ("ignore_index", ctypes.c_int64), ("flags", ctypes.c_int64)]


class JoinOutputs(ctypes.Structure):
    """td_join_outputs (include/tokendagger_hip.h): host or device addresses."""
    _fields_ = [("ids", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("types", ctypes.c_void_p), ("ids_capacity", ctypes.c_int64),
                ("offsets", ctypes.c_void_p), ("examples", ctypes.c_void_p), ("field_len", ctypes.c_void_p)]


def join_field(before=(), max_len: int | None = None, shrink_rank: int = 0, type_value: int = 0, keep_tail: bool = False,
               train: bool = False, train_before: bool = False, flags: int | None = None) -> dict:
    """One field of a join_spec: literal ids in front of the body, the body's cap, its rank in the cut for max_total (0: never
    cut), its type value, and what is trained.  flags, where given, replaces the three booleans."""
    fl = flags if flags is not None else (TD_JOIN_KEEP_TAIL * keep_tail | TD_JOIN_TRAIN * train | TD_JOIN_TRAIN_BEFORE * train_before)
    return {"before": [int(x) for x in before], "max_len": -1 if max_len is None else int(max_len), "shrink_rank": int(shrink_rank),
            "type_value": int(type_value), "flags": int(fl)}


def join_spec(fields, tail=(), tail_type: int = 0, train_tail: bool = False, max_total: int | None = None,
              shrink: int | str = TD_JOIN_SHRINK_ORDER, field_major: bool = False, ignore_index: int = -100, flags: int | None = None,
              n_fields: int | None = None) -> JoinSpec:
    """td_join_spec from join_field(...) dicts.  shrink: TD_JOIN_SHRINK_ORDER / "order" or TD_JOIN_SHRINK_LONGEST / "longest".
    Counts that the structure cannot hold raise ValueError; everything else is left to the library's checks (flags and n_fields,
    where given, are passed as they are)."""
    fields = list(fields)
    tail = [int(x) for x in tail]
    if len(fields) > TD_JOIN_MAX_FIELDS or len(tail) > TD_JOIN_MAX_LITERAL or any(len(f["before"]) > TD_JOIN_MAX_LITERAL for f in fields):
        raise ValueError("a join has at most 8 fields and 16 literal ids a place")
    sp = JoinSpec()
    sp.n_fields = len(fields) if n_fields is None else n_fields
    for i, f in enumerate(fields):
        for q, x in enumerate(f["before"]):
            sp.fields[i].before[q] = x
        sp.fields[i].n_before = f.get("n_before", len(f["before"]))
        sp.fields[i].max_len, sp.fields[i].shrink_rank = f["max_len"], f["shrink_rank"]
        sp.fields[i].type_value, sp.fields[i].flags = f["type_value"], f["flags"]
    for q, x in enumerate(tail):
        sp.tail[q] = x
    sp.n_tail, sp.tail_type = len(tail), tail_type
    sp.max_total = -1 if max_total is None else max_total
    sp.shrink = {"order": TD_JOIN_SHRINK_ORDER, "longest": TD_JOIN_SHRINK_LONGEST}.get(shrink, shrink)
    sp.ignore_index = ignore_index
    sp.flags = flags if flags is not None else (TD_JOIN_FIELD_MAJOR * field_major | TD_JOIN_TRAIN_TAIL * train_tail)
    return sp


def join_plan(tok_offsets, spec: JoinSpec, outputs: bool = True):
    """td_join_plan (host only, no device): counts int64[4] = kept examples E, kept slots T, examples dropped, examples truncated;
    with outputs=True also out_offsets int64[E + 1], out_examples int64[E] and out_field_len int32[E, K].  An error carries
    .counts ([0]: the example with bad offsets, -1 for an argument error)."""
    lib = load_library()
    o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
    n_docs = len(o) - 1
    if n_docs < 0:
        raise ValueError("tok_offsets must have n_docs + 1 entries")
    K = max(int(spec.n_fields), 1)
    n_ex = n_docs // K
    counts = np.zeros(4, dtype=np.int64)
    offs = np.empty(n_ex + 1, dtype=np.int64) if outputs else None
    exs = np.empty(max(n_ex, 1), dtype=np.int64) if outputs else None
    flen = np.empty(max(n_ex, 1) * K, dtype=np.int32) if outputs else None
    rc = lib.td_join_plan(o.ctypes.data, n_docs, ctypes.byref(spec), counts.ctypes.data, offs.ctypes.data if outputs else None,
                          exs.ctypes.data if outputs else None, flen.ctypes.data if outputs else None)
    if rc != TD_OK:
        ex = TokenDaggerHipError(rc, "td_join_plan: invalid spec or arguments" if counts[0] < 0 else
                                 f"td_join_plan: example {int(counts[0])} has a document without valid offsets")
        ex.counts = counts
        raise ex
    e = int(counts[0])
    return (counts, offs[:e + 1], exs[:e], flen[:e * K].reshape(e, K)) if outputs else counts


TD_DECODE_KEEP_STOP, TD_DECODE_SKIP_NEGATIVE, TD_DECODE_SKIP_SPECIAL = 1, 2, 4


class DecodeSpec(ctypes.Structure):
    """td_decode_spec (include/tokendagger_hip.h).  Build it with decode_spec: that keeps the lists alive beside the pointers."""
    _fields_ = [("row_stride", ctypes.c_int64), ("skip_ids", ctypes.c_void_p), ("n_skip", ctypes.c_int64),
                ("stop_ids", ctypes.c_void_p), ("n_stop", ctypes.c_int64), ("flags", ctypes.c_int64)]


def decode_spec(row_stride: int = 0, skip=(), stop=(), keep_stop: bool = False, skip_negative: bool = False, skip_special: bool = False,
                flags: int = 0) -> DecodeSpec:
    """row_stride 0: segments by tok_offsets; >= 1: rows of that many ids.  skip / stop: iterables of ids."""
    sk = np.ascontiguousarray(np.asarray(list(skip), dtype=np.int64).astype(np.int32))
    st = np.ascontiguousarray(np.asarray(list(stop), dtype=np.int64).astype(np.int32))
    flags |= (TD_DECODE_KEEP_STOP if keep_stop else 0) | (TD_DECODE_SKIP_NEGATIVE if skip_negative else 0) | (TD_DECODE_SKIP_SPECIAL if skip_special else 0)
    spec = DecodeSpec(row_stride, sk.ctypes.data if len(sk) else None, len(sk), st.ctypes.data if len(st) else None, len(st), flags)
    spec._keep = (sk, st)
    return spec


def _decode_rows_args(ids, tok_offsets, lengths, n_segs, spec: DecodeSpec):
    """The arrays of a host decode-rows call -> (ids int32 (flat), offsets int64 | None, lengths int32 | None, n_segs)."""
    t = np.ascontiguousarray(ids, dtype=np.int32)
    if spec.row_stride == 0:
        if tok_offsets is None:
            raise ValueError("the offsets form (row_stride 0) needs tok_offsets")
        o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
        return t.reshape(-1), o, None, len(o) - 1
    ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
    if n_segs is None:
        n_segs = len(ln) if ln is not None else (t.shape[0] if t.ndim == 2 else t.size // int(spec.row_stride))
    return t.reshape(-1), None, ln, int(n_segs)


def decode_rows_check(spec: DecodeSpec | None, n_tokens: int, tok_offsets=None, lengths=None, n_segs: int | None = None) -> None:
    """td_decode_rows_check (host only, no device): raises TokenDaggerHipError(TD_E_INVALID) with .pos = the offending index (-1: an
    argument as such)."""
    lib = load_library()
    o = None if tok_offsets is None else np.ascontiguousarray(tok_offsets, dtype=np.int64)
    ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
    if n_segs is None:
        n_segs = len(o) - 1 if o is not None else (len(ln) if ln is not None else 0)
    pos = ctypes.c_int64(0)
    rc = lib.td_decode_rows_check(ctypes.byref(spec) if spec is not None else None, n_tokens, o.ctypes.data if o is not None else None,
                                  ln.ctypes.data if ln is not None else None, n_segs, ctypes.byref(pos))
    if rc != TD_OK:
        ex = TokenDaggerHipError(rc, f"td_decode_rows_check: invalid arguments (index {pos.value})")
        ex.pos = int(pos.value)
        raise ex


class CountsSpec(ctypes.Structure):
    """td_counts_spec (include/tokendagger_hip.h)."""
    _fields_ = [("n_bins", ctypes.c_int64), ("n_groups", ctypes.c_int64), ("flags", ctypes.c_int64)]


def counts_spec(n_bins: int, n_groups: int = 1, accumulate: bool = False, flags: int = 0) -> CountsSpec:
    """Values 0 .. n_bins - 1 are counted, per group 0 .. n_groups - 1; accumulate: add to the counts that are there."""
    return CountsSpec(n_bins, n_groups, flags | (TD_COUNTS_ACCUMULATE if accumulate else 0))


def _counts_args(ids, tok_offsets, groups, spec: CountsSpec, counts):
    """The arrays of a host counts call: ids, offsets | None, groups | None, n_docs, counts (int64[n_groups * n_bins]: the caller's
    with TD_COUNTS_ACCUMULATE, else a new one), info."""
    t = np.ascontiguousarray(ids, dtype=np.int32)
    o = None if tok_offsets is None else np.ascontiguousarray(tok_offsets, dtype=np.int64)
    g = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
    n_docs = 0 if o is None else len(o) - 1
    if g is not None and len(g) != n_docs:
        raise ValueError("groups must have one entry per document")
    size = max(int(spec.n_bins) * int(spec.n_groups), 0)
    if spec.flags & TD_COUNTS_ACCUMULATE:
        if counts is None or counts.dtype != np.int64 or not counts.flags.c_contiguous or counts.size != size:
            raise ValueError("TD_COUNTS_ACCUMULATE needs counts: a contiguous int64 array of n_groups * n_bins entries")
    else:
        counts = np.empty(min(size, 1 << 28) or 1, dtype=np.int64)
    if g is not None and g.size == 0:
        g = np.zeros(1, dtype=np.int32)[:0]  # (an empty list's address is not NULL)
    return t, o, g, n_docs, counts, np.zeros(4, dtype=np.int64)


def _counts_shape(counts, spec: CountsSpec):
    return counts.reshape(int(spec.n_groups), int(spec.n_bins))


def token_counts_host(ids, tok_offsets=None, groups=None, spec: CountsSpec | None = None, counts=None, n_tokens: int | None = None):
    """td_token_counts_host (host only, no device) -> (counts int64[n_groups, n_bins], info int64[4] = counted, negative, too_large,
    0).  An error carries .info ([0]: the document of a bad group, -1 for an argument error)."""
    lib = load_library()
    if spec is None:
        raise ValueError("a counts_spec is required")
    t, o, g, n_docs, counts, info = _counts_args(ids, tok_offsets, groups, spec, counts)
    rc = lib.td_token_counts_host(t.ctypes.data if len(t) else None, len(t) if n_tokens is None else n_tokens,
                                  o.ctypes.data if o is not None else None, n_docs, g.ctypes.data if g is not None else None,
                                  ctypes.byref(spec), counts.ctypes.data, info.ctypes.data)
    if rc != TD_OK:
        ex = TokenDaggerHipError(rc, "td_token_counts_host: invalid spec, offsets or arguments" if info[0] < 0 else
                                 f"td_token_counts_host: doc_group[{int(info[0])}] is outside [0, n_groups)")
        ex.info = info
        raise ex
    return _counts_shape(counts, spec), info


class NgramSpec(ctypes.Structure):
    """td_ngram_spec (include/tokendagger_hip.h)."""
    _fields_ = [("ignore_index", ctypes.c_int64), ("flags", ctypes.c_int64)]


def ngram_spec(ignore_index: int = -100, accumulate: bool = False, flags: int = 0) -> NgramSpec:
    """ignore_index: what a covered label becomes; accumulate: add to the pattern counts that are there."""
    return NgramSpec(ignore_index, flags | (TD_NGRAM_ACCUMULATE if accumulate else 0))


def ngram_patterns(sequences, offsets=None):
    """A pattern list as the C ABI takes it -> (pat_ids int32, pat_offsets int64).  sequences: a list of id lists, or flat ids with
    offsets[n_pats + 1].  Nothing is checked here: the library does that (TD_E_INVALID with a message)."""
    if offsets is not None:
        return np.ascontiguousarray(sequences, dtype=np.int32), np.ascontiguousarray(offsets, dtype=np.int64)
    seqs = [np.asarray(q, dtype=np.int32).reshape(-1) for q in sequences]
    offs = np.zeros(len(seqs) + 1, dtype=np.int64)
    if seqs:
        np.cumsum([len(q) for q in seqs], out=offs[1:])
    ids = np.concatenate(seqs).astype(np.int32) if seqs else np.zeros(0, dtype=np.int32)
    return np.ascontiguousarray(ids), offs


def _ngram_outputs(total: int, n_docs: int, n_pats: int, spec: NgramSpec, cover: bool, labels, doc_stats: bool, pattern_counts):
    """The host arrays of a matches call -> (cover | None, labels | None (a copy of the caller's), doc_stats | None, pattern_counts |
    None, counts).  pattern_counts: True for a new array, an int64[n_pats] array to use (TD_NGRAM_ACCUMULATE adds to it), False / None."""
    cv = np.zeros(max(total, 1), dtype=np.uint8) if cover else None
    lb = None
    if labels is not None:
        lb = np.array(labels, dtype=np.int32, copy=True).reshape(-1)
        if len(lb) < total:
            raise ValueError("labels must have an entry for every id")
    ds = np.zeros((max(n_docs, 1), 2), dtype=np.int64) if doc_stats else None
    pc = None
    if isinstance(pattern_counts, np.ndarray):
        if pattern_counts.dtype != np.int64 or not pattern_counts.flags.c_contiguous or pattern_counts.size != n_pats:
            raise ValueError("pattern_counts must be a contiguous int64 array with one entry per pattern")
        pc = pattern_counts
    elif pattern_counts:
        if spec.flags & TD_NGRAM_ACCUMULATE:
            raise ValueError("TD_NGRAM_ACCUMULATE needs the pattern_counts array to add to")
        pc = np.zeros(n_pats, dtype=np.int64)
    return cv, lb, ds, pc, np.zeros(4, dtype=np.int64)


def _ngram_result(total, n_docs, cv, lb, ds, pc, counts):
    return (cv[:total] if cv is not None else None, lb, ds[:n_docs] if ds is not None else None, pc, counts)


def _ptr(a):
    return a.ctypes.data if a is not None else None


def ngram_matches_host(sequences, ids, tok_offsets, spec: NgramSpec | None = None, offsets=None, cover: bool = True, labels=None,
                       doc_stats: bool = True, pattern_counts=True, n_tokens: int | None = None):
    """td_ngram_matches_host (host only, no device) -> (cover uint8[total] | None, labels int32 | None, doc_stats int64[n_docs, 2] |
    None, pattern_counts int64[n_pats] | None, counts int64[4] = occurrences, covered ids, documents with an occurrence, 0)."""
    lib = load_library()
    spec = spec if spec is not None else ngram_spec()
    pi, po = ngram_patterns(sequences, offsets)
    t = np.ascontiguousarray(ids, dtype=np.int32)
    o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
    n_docs, n_pats = len(o) - 1, len(po) - 1
    total = int(o[-1]) if 0 <= int(o[-1]) <= len(t) else 0
    cv, lb, ds, pc, counts = _ngram_outputs(total, n_docs, max(n_pats, 1), spec, cover, labels, doc_stats, pattern_counts)
    rc = lib.td_ngram_matches_host(pi.ctypes.data if len(pi) else None, po.ctypes.data, n_pats, t.ctypes.data if len(t) else None,
                                   len(t) if n_tokens is None else n_tokens, o.ctypes.data, n_docs, ctypes.byref(spec), _ptr(cv), _ptr(lb),
                                   _ptr(ds), _ptr(pc), counts.ctypes.data)
    if rc != TD_OK:
        raise TokenDaggerHipError(rc, "td_ngram_matches_host: invalid patterns, offsets, spec or arguments")
    return _ngram_result(total, n_docs, cv, lb, ds, pc, counts)


class MinhashSpec(ctypes.Structure):
    """td_minhash_spec (include/tokendagger_hip.h)."""
    _fields_ = [("k", ctypes.c_int64), ("num_perm", ctypes.c_int64), ("seed", ctypes.c_uint64), ("bands", ctypes.c_int64),
                ("rows", ctypes.c_int64), ("flags", ctypes.c_int64)]


def minhash_spec(k: int = 5, num_perm: int = 128, seed: int = 1, bands: int = 0, rows: int | None = None, flags: int = 0) -> MinhashSpec:
    """k ids a shingle, num_perm permutations of the family `seed`; bands > 0 asks for band keys of `rows` signature entries each
    (None: num_perm // bands)."""
    if rows is None:
        rows = num_perm // bands if bands > 0 else 0
    return MinhashSpec(k, num_perm, seed, bands, rows, flags)


def minhash_params(seed: int, num_perm: int):
    """td_minhash_params -> (a uint64[num_perm], b uint64[num_perm]): h_j(x) = (a[j] * x + b[j] mod 2^64) >> 32."""
    lib = load_library()
    a, b = np.zeros(max(num_perm, 1), dtype=np.uint64), np.zeros(max(num_perm, 1), dtype=np.uint64)
    rc = lib.td_minhash_params(seed, num_perm, a.ctypes.data, b.ctypes.data)
    if rc != TD_OK:
        raise TokenDaggerHipError(rc, "td_minhash_params: num_perm must be in 1 .. 1024")
    return a[:num_perm], b[:num_perm]


def _minhash_args(ids, tok_offsets, spec: MinhashSpec):
    """-> (ids int32, offsets int64, n_docs, sig uint32[n_docs, num_perm], keys uint64[n_docs, bands] | None, counts int64[4])"""
    t = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
    n_docs = len(o) - 1
    return t, o, n_docs, _minhash_outputs(n_docs, spec)


def _minhash_outputs(n_docs: int, spec: MinhashSpec):
    np_, nb = max(int(spec.num_perm), 1), max(int(spec.bands), 0)
    sig = np.zeros((max(n_docs, 1), np_), dtype=np.uint32)
    keys = np.zeros((max(n_docs, 1), nb), dtype=np.uint64) if nb > 0 else None
    return sig, keys, np.zeros(4, dtype=np.int64)


def minhash_host(ids, tok_offsets, spec: MinhashSpec | None = None, n_tokens: int | None = None):
    """td_minhash_host (host only, no device) -> (sig uint32[n_docs, num_perm], band_keys uint64[n_docs, bands] | None, counts int64[4]
    = shingles hashed, documents with no id, documents of 1 .. k - 1 ids, 0)."""
    lib = load_library()
    spec = spec if spec is not None else minhash_spec()
    t, o, n_docs, (sig, keys, counts) = _minhash_args(ids, tok_offsets, spec)
    rc = lib.td_minhash_host(t.ctypes.data if len(t) else None, len(t) if n_tokens is None else n_tokens, o.ctypes.data, n_docs,
                             ctypes.byref(spec), sig.ctypes.data, _ptr(keys), counts.ctypes.data)
    if rc != TD_OK:
        raise TokenDaggerHipError(rc, "td_minhash_host: invalid offsets, spec or arguments")
    return sig[:n_docs], (keys[:n_docs] if keys is not None else None), counts


TD_NFC_INFO_UNICODE_VERSION, TD_NFC_INFO_TABLE_BYTES = 0, 1


def nfc_info(what: int) -> int:
    """td_nfc_info: TD_NFC_INFO_UNICODE_VERSION (major * 10000 + minor * 100 + patch) or TD_NFC_INFO_TABLE_BYTES; -1: no such value."""
    return int(load_library().td_nfc_info(what))


_NFC_PER_DOC = (np.uint8, np.uint8)            # flags, changed
_UTF8_PER_DOC = (np.uint8, np.int64, np.int64)  # flags, first_bad, n_bad


def _rewrite_args(text, doc_offsets, per_doc):
    """The arrays of a text rewrite (NFC, UTF-8) -> (text uint8, offsets int64, n_docs, out_doc_offsets int64[n_docs + 1], an array
    [n_docs] of each dtype in per_doc, counts int64[8])"""
    buf = _as_u8(text)
    o = np.ascontiguousarray(doc_offsets, dtype=np.int64)
    n_docs = len(o) - 1
    return (buf, o, n_docs, np.zeros(n_docs + 1, dtype=np.int64), *(np.zeros(max(n_docs, 1), dtype=d) for d in per_doc),
            np.zeros(8, dtype=np.int64))


def _rewrite_capacity(buf, o, capacity, growth=3):
    """The bytes a rewritten text can need where the caller names none: `growth` times the documents' bytes (three for NFC and for
    UTF-8 under REPLACE, one under IGNORE)."""
    return growth * int(o[-1]) if capacity is None and len(o) and 0 <= int(o[-1]) <= len(buf) else int(capacity or 0)


def _raise_with_counts(rc, message, counts):
    ex = TokenDaggerHipError(rc, message)
    ex.counts = counts
    raise ex


def _encode_rewritten(buf, o, n_docs, return_text, call):
    """td_encode_batch_nfc / _utf8: call(ids, cap, tok_offsets, text | None, text_cap) -> rc, with room for the text's own bytes and,
    only when that call asks for it, for three times as many (a rewrite rarely grows a text) -> (rc, ids, tok_offsets, text | None)"""
    n = int(o[-1]) if len(o) and 0 <= int(o[-1]) <= len(buf) else 0
    toff = np.zeros(n_docs + 1, dtype=np.int64)
    for cap in (n + 64, 3 * n + 64):
        ids = np.empty(cap, dtype=np.int32)
        out = np.empty(cap, dtype=np.uint8) if return_text else None
        rc = call(ids.ctypes.data, cap, toff.ctypes.data, _ptr(out), cap if return_text else 0)
        if rc != TD_E_CAPACITY:
            break
    return rc, ids, toff, out


def nfc_host(text, doc_offsets, capacity: int | None = None, want_text: bool = True):
    """td_nfc_host (host only, no device) -> (text uint8[counts[0]] | None, out_doc_offsets int64[n_docs + 1], flags uint8[n_docs]
    (0: proven NFC), changed uint8[n_docs], counts int64[8] = output bytes, documents not proven, documents changed, segments rewritten,
    code points in them, opaque bytes, longest segment, 0).  want_text=False: the sizing call.  capacity None: three times the input."""
    lib = load_library()
    buf, o, n_docs, ooff, flags, changed, counts = _rewrite_args(text, doc_offsets, _NFC_PER_DOC)
    if n_docs >= 0 and len(o) and int(o[-1]) > len(buf):
        raise TokenDaggerHipError(TD_E_INVALID, "td_nfc_host: doc_offsets end behind the text")
    cap = _rewrite_capacity(buf, o, capacity) if want_text else 0
    out = np.empty(max(cap, 1), dtype=np.uint8)
    rc = lib.td_nfc_host(buf.ctypes.data if len(buf) else None, o.ctypes.data if len(o) else None, n_docs, out.ctypes.data if want_text else None,
                         cap, ooff.ctypes.data, flags.ctypes.data, changed.ctypes.data, counts.ctypes.data)
    if rc != TD_OK:
        _raise_with_counts(rc, "td_nfc_host: output capacity too small" if rc == TD_E_CAPACITY else "td_nfc_host: invalid offsets or arguments", counts)
    return (out[:int(counts[0])] if want_text else None), ooff, flags[:n_docs], changed[:n_docs], counts


TD_UTF8_REPLACE, TD_UTF8_IGNORE = 0, 1
# (the UTF-8 entry points of include/tokendagger_hip.h)
EXPORTS_UTF8 = ["td_utf8_host", "td_utf8_check_device", "td_utf8_device", "td_utf8", "td_encode_batch_utf8"]


def utf8_host(text, doc_offsets, policy: int = TD_UTF8_REPLACE, capacity: int | None = None, want_text: bool = True):
    """td_utf8_host (host only, no device) -> (text uint8[counts[0]] | None, out_doc_offsets int64[n_docs + 1], flags uint8[n_docs]
    (0: well-formed), first_bad int64[n_docs] (-1: none), n_bad int64[n_docs], counts int64[8] = output bytes, documents ill-formed,
    subparts, bytes in subparts, documents that begin with a continuation byte, documents that end in a cut character, 0, 0).
    want_text=False: the sizing call.  capacity None: what the policy can need."""
    lib = load_library()
    buf, o, n_docs, ooff, flags, first, nbad, counts = _rewrite_args(text, doc_offsets, _UTF8_PER_DOC)
    if n_docs >= 0 and len(o) and int(o[-1]) > len(buf):
        raise TokenDaggerHipError(TD_E_INVALID, "td_utf8_host: doc_offsets end behind the text")
    cap = _rewrite_capacity(buf, o, capacity, 1 if policy == TD_UTF8_IGNORE else 3) if want_text else 0
    out = np.empty(max(cap, 1), dtype=np.uint8)
    rc = lib.td_utf8_host(buf.ctypes.data if len(buf) else None, o.ctypes.data if len(o) else None, n_docs, policy,
                          out.ctypes.data if want_text else None, cap, ooff.ctypes.data, flags.ctypes.data, first.ctypes.data, nbad.ctypes.data,
                          counts.ctypes.data)
    if rc != TD_OK:
        _raise_with_counts(rc, "td_utf8_host: output capacity too small" if rc == TD_E_CAPACITY else "td_utf8_host: invalid offsets or arguments", counts)
    return (out[:int(counts[0])] if want_text else None), ooff, flags[:n_docs], first[:n_docs], nbad[:n_docs], counts


TD_TS_COLS, TD_TS_LOCAL, TD_TS_RUNS = 21, 1, 2
TD_TS_ALL = TD_TS_LOCAL | TD_TS_RUNS
# stats[:, c] by name (include/tokendagger_hip.h, COLUMNS)
TS_COLUMNS = ("bytes", "chars", "upper", "lower", "letter_other", "mark", "number", "space", "non_ascii", "words", "words_alpha",
              "word_max_bytes", "lines", "lines_blank", "line_max_bytes", "lines_end_terminal", "lines_end_ellipsis", "lines_start_bullet",
              "hashes", "ellipses", "curly")


def _text_stats_args(text, doc_offsets):
    """-> (text uint8, offsets int64, n_docs, stats int64[max(n_docs, 1), 21], totals int64[21])"""
    buf = _as_u8(text)
    o = np.ascontiguousarray(doc_offsets, dtype=np.int64)
    n_docs = len(o) - 1
    return buf, o, n_docs, np.zeros((max(n_docs, 1), TD_TS_COLS), dtype=np.int64), np.zeros(TD_TS_COLS, dtype=np.int64)


def text_stats_host(text, doc_offsets, groups: int = TD_TS_ALL):
    """td_text_stats_host (host only, no device) -> (stats int64[n_docs, 21], totals int64[21])."""
    lib = load_library()
    buf, o, n_docs, stats, totals = _text_stats_args(text, doc_offsets)
    if n_docs >= 0 and len(o) and int(o[-1]) > len(buf):
        raise TokenDaggerHipError(TD_E_INVALID, "td_text_stats_host: doc_offsets end behind the text")
    rc = lib.td_text_stats_host(buf.ctypes.data if len(buf) else None, o.ctypes.data if len(o) else None, n_docs, groups, stats.ctypes.data,
                                totals.ctypes.data)
    if rc != TD_OK:
        raise TokenDaggerHipError(rc, "td_text_stats_host: invalid offsets, groups or arguments")
    return stats[:n_docs], totals


class NgramSet:
    """Owns one td_ngram_set: a de-duplicated pattern list and its lookup table on a tokenizer's device.  Immutable; any handle on
    that device may use it.  A context manager; close() frees the device memory at once, so the work that uses the set must be done."""

    def __init__(self, tok: "HipTokenizer", sequences, offsets=None):
        self._lib = tok._lib
        self._h = None
        pi, po = ngram_patterns(sequences, offsets)
        h = ctypes.c_void_p()
        tok._check(self._lib.td_ngram_set_create(tok._h, pi.ctypes.data if len(pi) else None, po.ctypes.data, len(po) - 1, ctypes.byref(h)))
        self._h = h
        self.n_pats = len(po) - 1

    @property
    def info(self) -> dict[str, int]:
        """patterns, distinct, lengths, max_len, slots, max_probe, device_bytes."""
        return {k: int(self._lib.td_ngram_set_info(self._h, v)) for k, v in TD_NGRAM_INFO.items()}

    def close(self):
        if getattr(self, "_h", None):
            self._lib.td_ngram_set_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class LabelsSpec(ctypes.Structure):
    """td_labels_spec (include/tokendagger_hip.h): opener id sequences, closer ids, ignore_index, flags."""
    _fields_ = [("n_open", ctypes.c_int64), ("open_len", ctypes.c_int64 * TD_LABELS_MAX_OPEN),
                ("open_ids", (ctypes.c_int32 * TD_LABELS_MAX_OPEN_LEN) * TD_LABELS_MAX_OPEN), ("n_close", ctypes.c_int64),
                ("close_ids", ctypes.c_int32 * TD_LABELS_MAX_CLOSE), ("ignore_index", ctypes.c_int64), ("flags", ctypes.c_int64)]


def labels_spec(open, close, ignore_index: int = -100, train_close: bool = True) -> LabelsSpec:
    """open: opener id sequences (at most 8 of at most 8 ids); close: closer ids (at most 16).  What fits the struct is passed
    on as it is: the library checks the rest (TD_E_INVALID with a message)."""
    open = [[int(i) for i in o] for o in open]
    close = [int(c) for c in close]
    if len(open) > TD_LABELS_MAX_OPEN:
        raise ValueError(f"{len(open)} openers: a td_labels_spec holds at most {TD_LABELS_MAX_OPEN}")
    if len(close) > TD_LABELS_MAX_CLOSE:
        raise ValueError(f"{len(close)} closers: a td_labels_spec holds at most {TD_LABELS_MAX_CLOSE}")
    sp = LabelsSpec()
    sp.n_open, sp.n_close, sp.ignore_index, sp.flags = len(open), len(close), int(ignore_index), TD_LABELS_TRAIN_CLOSE if train_close else 0
    for k, o in enumerate(open):
        if len(o) > TD_LABELS_MAX_OPEN_LEN:
            raise ValueError(f"opener {k} has {len(o)} ids: an opener holds at most {TD_LABELS_MAX_OPEN_LEN}")
        sp.open_len[k] = len(o)
        for j, i in enumerate(o):
            sp.open_ids[k][j] = i
    for k, c in enumerate(close):
        sp.close_ids[k] = c
    return sp


TD_RANGE_OVERLAP, TD_RANGE_INSIDE, TD_RANGE_START = 0, 1, 2
RANGE_RULES = {"overlap": TD_RANGE_OVERLAP, "inside": TD_RANGE_INSIDE, "start": TD_RANGE_START}


class RangeSpec(ctypes.Structure):
    """td_range_spec (include/tokendagger_hip.h): the rule, ignore_index, flags."""
    _fields_ = [("rule", ctypes.c_int64), ("ignore_index", ctypes.c_int64), ("flags", ctypes.c_int64)]


def range_spec(rule="overlap", ignore_index: int = -100, flags: int = 0) -> RangeSpec:
    """rule: "overlap" (an id with a marked byte is trained), "inside" (all of its bytes), "start" (its first byte), or a TD_RANGE_*
    value; what fits the struct is passed on as it is, the library checks it."""
    if isinstance(rule, str):
        if rule not in RANGE_RULES:
            raise ValueError(f"rule must be one of {sorted(RANGE_RULES)}, not {rule!r}")
        rule = RANGE_RULES[rule]
    return RangeSpec(int(rule), int(ignore_index), int(flags))


def as_ranges(ranges, n_docs: int | None = None):
    """Byte ranges in either form -> (range_offsets int64[n_docs + 1], ranges int64[n, 2], both contiguous): a pair
    (range_offsets, array[n, 2]), or one sequence of (begin, end) pairs per document."""
    if isinstance(ranges, tuple) and len(ranges) == 2 and isinstance(ranges[1], np.ndarray) and ranges[1].ndim == 2:
        ro = np.ascontiguousarray(ranges[0], dtype=np.int64)
        rg = np.ascontiguousarray(ranges[1], dtype=np.int64)
    else:
        per = [np.asarray(r, dtype=np.int64).reshape(-1, 2) for r in ranges]
        ro = np.zeros(len(per) + 1, dtype=np.int64)
        if per:
            np.cumsum([len(r) for r in per], out=ro[1:])
        rg = np.ascontiguousarray(np.concatenate(per) if per else np.zeros((0, 2), dtype=np.int64))
    if rg.ndim != 2 or rg.shape[1] != 2:
        raise ValueError("ranges must have the shape [n, 2]")
    if len(ro) < 1 or (n_docs is not None and len(ro) != n_docs + 1):
        raise ValueError("ranges must have an entry (range_offsets: n_docs + 1 entries) for every document")
    if len(ro) and int(ro[-1]) > len(rg):
        raise ValueError("range_offsets end above the number of ranges")
    return ro, rg


def range_plan(ranges, doc_lens=None):
    """td_range_plan (host only, no device): the structural checks of byte ranges -> counts int64[2] = non-empty ranges, marked
    bytes.  doc_lens: the documents' byte lengths (a range may not end above its document's).  An error carries .bad: the first
    bad document (range_offsets) or the first bad global range index."""
    lib = load_library()
    ro, rg = as_ranges(ranges)
    n_docs = len(ro) - 1
    dl = None if doc_lens is None else np.ascontiguousarray(doc_lens, dtype=np.int64)
    if dl is not None and len(dl) != n_docs:
        raise ValueError("doc_lens must have an entry for every document")
    counts = np.zeros(2, dtype=np.int64)
    bad = ctypes.c_int64(-1)
    rc = lib.td_range_plan(ro.ctypes.data, rg.ctypes.data if len(rg) else None, n_docs, dl.ctypes.data if dl is not None else None,
                           counts.ctypes.data, ctypes.byref(bad))
    if rc != TD_OK:
        ex = TokenDaggerHipError(rc, f"td_range_plan: invalid range_offsets or ranges at index {bad.value}")
        ex.bad = bad.value
        raise ex
    return counts


def chars_to_bytes(text, doc_offsets, ranges):
    """Ranges in characters -> the same in bytes, on the host (one numpy pass over the text): index k of a document is its k-th
    byte that is not a UTF-8 continuation byte, k equal to their number is the document's end.  Returns (range_offsets, ranges)."""
    buf = _as_u8(text)
    offs = np.ascontiguousarray(doc_offsets, dtype=np.int64)
    ro, rg = as_ranges(ranges, len(offs) - 1)
    lead = np.flatnonzero((buf[:int(offs[-1])] & 0xC0) != 0x80).astype(np.int64)  # the positions of the characters' first bytes
    first = np.searchsorted(lead, offs)  # characters in front of every document (and of the text's end)
    doc = np.repeat(np.arange(len(offs) - 1), np.diff(ro))
    k = rg[:int(ro[-1])]
    n_chars = (first[1:] - first[:-1])[doc][:, None]
    if ((k < 0) | (k > n_chars)).any():
        raise ValueError("a character range lies outside its document")
    g = first[doc][:, None] + k
    table = np.concatenate([lead, [0]])
    out = np.where(k == n_chars, offs[1:][doc][:, None], table[np.minimum(g, len(lead))]) - offs[:-1][doc][:, None]
    return ro, np.ascontiguousarray(out, dtype=np.int64)


def _as_u8(data) -> np.ndarray:
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(0, dtype=np.uint8)


class Vocab:
    """A `td_vocab`: vocabulary files read by the C++ loaders (tiktoken .model, HF tokenizer_config.json,
    tekken.json, the reference wrapper's JSON files).  Host only: works without a GPU."""

    def __init__(self):
        self._lib = load_library()
        h = ctypes.c_void_p()
        if self._lib.td_vocab_create(ctypes.byref(h)) != TD_OK:
            raise TokenDaggerHipError(1, "td_vocab_create failed")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.td_vocab_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc: int):
        if rc != TD_OK:
            raise TokenDaggerHipError(rc, self._lib.td_vocab_error(self._h).decode("utf-8", "replace"))
        return self

    @staticmethod
    def _p(path) -> bytes:
        import os
        return os.fsencode(str(path))

    def load_tiktoken(self, path):
        return self._check(self._lib.td_vocab_load_tiktoken(self._h, self._p(path)))

    def load_hf_special(self, path, also_mergeable: bool = False):
        return self._check(self._lib.td_vocab_load_hf_special(self._h, self._p(path), int(also_mergeable)))

    def load_tekken(self, path):
        return self._check(self._lib.td_vocab_load_tekken(self._h, self._p(path)))

    def load_json(self, vocab_path=None, special_path=None):
        return self._check(self._lib.td_vocab_load_json(self._h, self._p(vocab_path) if vocab_path else None,
                                                        self._p(special_path) if special_path else None))

    def set_pattern(self, pat_str: str):
        return self._check(self._lib.td_vocab_set_pattern(self._h, pat_str.encode("utf-8")))

    @property
    def pattern(self) -> str:
        return self._lib.td_vocab_pattern(self._h).decode("utf-8")

    def arrays(self, special: bool = False):
        """-> (bytes uint8[total], offsets int64[n+1], ranks int32[n]) copies of the loaded tokens."""
        b, o, r = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        n = ctypes.c_int64(0)
        self._check(self._lib.td_vocab_arrays(self._h, int(special), ctypes.byref(b), ctypes.byref(o), ctypes.byref(r),
                                              ctypes.byref(n)))
        cnt = n.value
        offs = np.ctypeslib.as_array(ctypes.cast(o, ctypes.POINTER(ctypes.c_int64)), shape=(cnt + 1,)).copy()
        ranks = (np.ctypeslib.as_array(ctypes.cast(r, ctypes.POINTER(ctypes.c_int32)), shape=(cnt,)).copy()
                 if cnt else np.zeros(0, dtype=np.int32))
        total = int(offs[-1])
        blob = (np.ctypeslib.as_array(ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)), shape=(total,)).copy()
                if total else np.zeros(0, dtype=np.uint8))
        return blob, offs, ranks

    def __len__(self) -> int:
        n = ctypes.c_int64(0)
        self._lib.td_vocab_arrays(self._h, 0, None, None, None, ctypes.byref(n))
        return n.value

    def mergeable_ranks(self) -> dict[bytes, int]:
        blob, offs, ranks = self.arrays(False)
        raw = blob.tobytes()
        return {raw[offs[i]:offs[i + 1]]: int(ranks[i]) for i in range(len(ranks))}

    def special_tokens(self) -> dict[str, int]:
        blob, offs, ranks = self.arrays(True)
        raw = blob.tobytes()
        return {raw[offs[i]:offs[i + 1]].decode("utf-8"): int(ranks[i]) for i in range(len(ranks))}


def load_tiktoken_bpe(path) -> dict[bytes, int]:
    """tiktoken.load.load_tiktoken_bpe for a local file, through the C++ loader."""
    return Vocab().load_tiktoken(path).mergeable_ranks()


class HipTokenizer:
    """Owns one `td_tokenizer` handle (device tables + workspace on one GPU)."""

    @classmethod
    def from_vocab(cls, vocab: Vocab, device: int = -1) -> "HipTokenizer":
        """td_create_from_vocab: no Python-side token objects at all."""
        self = cls.__new__(cls)
        self._lib = load_library()
        self._h = None
        h = ctypes.c_void_p()
        rc = self._lib.td_create_from_vocab(vocab._h, device, ctypes.byref(h))
        if rc != TD_OK:
            raise TokenDaggerHipError(rc, self._lib.td_last_error(None).decode("utf-8", "replace"))
        self._h = h
        return self

    def __init__(self, pat_str: str, mergeable_ranks: dict[bytes, int], special_tokens: dict[str, int] | None = None,
                 device: int = -1):
        self._lib = load_library()
        self._h = None
        special_tokens = special_tokens or {}
        b, o, r = _pack(list(mergeable_ranks.items()))
        sb, so, sr = _pack([(k.encode("utf-8"), v) for k, v in special_tokens.items()])
        h = ctypes.c_void_p()
        rc = self._lib.td_create(pat_str.encode("utf-8"), len(r), b.ctypes.data, o.ctypes.data, r.ctypes.data,
                                 len(sr), sb.ctypes.data, so.ctypes.data, sr.ctypes.data, device, ctypes.byref(h))
        if rc != TD_OK:
            raise TokenDaggerHipError(rc, self._lib.td_last_error(None).decode("utf-8", "replace"))
        self._h = h

    @classmethod
    def borrow(cls, handle: int) -> "HipTokenizer":
        """The methods of this class on a td_tokenizer that someone else owns (closing the result does nothing)."""
        self = cls.__new__(cls)
        self._lib = load_library()
        self._h = ctypes.c_void_p(handle)
        self._borrowed = True
        return self

    def clone(self) -> "HipTokenizer":
        """td_clone: a second handle on the same device tables (own lock, workspace and streams) — one per host thread / HIP
        stream for concurrent encodes.  Either handle may be closed first."""
        other = type(self).__new__(type(self))
        other._lib = self._lib
        other._h = None
        h = ctypes.c_void_p()
        rc = self._lib.td_clone(self._h, ctypes.byref(h))
        if rc != TD_OK:
            raise TokenDaggerHipError(rc, self._lib.td_last_error(None).decode("utf-8", "replace"))
        other._h = h
        return other

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                self._lib.td_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc: int):
        if rc != TD_OK:
            raise TokenDaggerHipError(rc, self._lib.td_last_error(self._h).decode("utf-8", "replace"))

    # ---- host-buffer API --------------------------------------------------------------------
    def encode_batch(self, text, doc_offsets, mode: int = TD_MODE_ENCODE, capacity: int | None = None):
        """text: bytes / uint8 array of all documents concatenated; doc_offsets: int64[n_docs+1].
        -> (tokens int32[total], offsets int64[n_docs+1])"""
        buf = _as_u8(text)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        n_docs = len(offs) - 1
        n = int(offs[-1]) if len(offs) else 0
        cap = capacity if capacity is not None else max(16, n // 3 + 16)
        out_offs = np.empty(n_docs + 1, dtype=np.int64)
        ntok = ctypes.c_int64(0)
        for _ in range(2):
            toks = np.empty(cap, dtype=np.int32)
            rc = self._lib.td_encode_batch(self._h, buf.ctypes.data if n else None, offs.ctypes.data, n_docs, mode,
                                           toks.ctypes.data, cap, out_offs.ctypes.data, ctypes.byref(ntok))
            if rc == TD_E_CAPACITY and capacity is None and ntok.value > cap:
                cap = ntok.value
                continue
            break
        self._check(rc)
        return toks[:ntok.value], out_offs

    def encode(self, data, mode: int = TD_MODE_ENCODE) -> np.ndarray:
        buf = _as_u8(data)
        toks, _ = self.encode_batch(buf, np.asarray([0, len(buf)], dtype=np.int64), mode)
        return toks

    def encode_with_special(self, data, allowed_ids) -> tuple[np.ndarray, int]:
        buf = _as_u8(data)
        ids = np.ascontiguousarray(sorted(allowed_ids), dtype=np.int32)
        cap = len(buf) + 16
        toks = np.empty(cap, dtype=np.int32)
        ntok = ctypes.c_int64(0)
        last = ctypes.c_int32(0)
        rc = self._lib.td_encode_with_special(self._h, buf.ctypes.data if len(buf) else None, len(buf),
                                              ids.ctypes.data if len(ids) else None, len(ids), toks.ctypes.data, cap,
                                              ctypes.byref(ntok), ctypes.byref(last))
        self._check(rc)
        return toks[:ntok.value].copy(), last.value

    @staticmethod
    def _pack_strs(strs):
        enc = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in strs]
        offs = np.zeros(len(enc) + 1, dtype=np.int64)
        if enc:
            np.cumsum([len(b) for b in enc], out=offs[1:])
        blob = np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8).copy()
        return blob, offs

    def encode_with_special_strs(self, data, allowed) -> tuple[np.ndarray, int]:
        """allowed: the special-token STRINGS that may be cut out (tiktoken's allowed_special)."""
        buf = _as_u8(data)
        ab, ao = self._pack_strs(list(allowed))
        cap = len(buf) + 16
        toks = np.empty(cap, dtype=np.int32)
        ntok = ctypes.c_int64(0)
        last = ctypes.c_int32(0)
        rc = self._lib.td_encode_with_special_strs(self._h, buf.ctypes.data if len(buf) else None, len(buf), ab.ctypes.data,
                                                   ao.ctypes.data, len(ao) - 1, toks.ctypes.data, cap, ctypes.byref(ntok),
                                                   ctypes.byref(last))
        self._check(rc)
        return toks[:ntok.value].copy(), last.value

    def encode_batch_with_special_strs(self, text, doc_offsets, allowed):
        buf = _as_u8(text)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        ab, ao = self._pack_strs(list(allowed))
        n_docs = len(offs) - 1
        n = int(offs[-1]) if len(offs) else 0
        cap = n + 16
        out_offs = np.empty(n_docs + 1, dtype=np.int64)
        toks = np.empty(cap, dtype=np.int32)
        ntok = ctypes.c_int64(0)
        rc = self._lib.td_encode_batch_with_special_strs(self._h, buf.ctypes.data if n else None, offs.ctypes.data, n_docs,
                                                         ab.ctypes.data, ao.ctypes.data, len(ao) - 1, toks.ctypes.data, cap,
                                                         out_offs.ctypes.data, ctypes.byref(ntok))
        self._check(rc)
        return toks[:ntok.value].copy(), out_offs

    # ---- start offsets (TD_UNIT_BYTES / TD_UNIT_CHARS) ---------------------------------------
    def token_starts(self, tokens, tok_offsets=None, unit: int = TD_UNIT_BYTES, n_tokens: int | None = None) -> np.ndarray:
        """td_token_starts: ids (all documents concatenated) + int64 tok_offsets (default: one document) -> int64 starts."""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        o = np.ascontiguousarray([0, len(t)] if tok_offsets is None else tok_offsets, dtype=np.int64)
        n = len(t) if n_tokens is None else n_tokens
        out = np.empty(max(n, 1), dtype=np.int64)
        self._check(self._lib.td_token_starts(self._h, t.ctypes.data if len(t) else None, n, o.ctypes.data, len(o) - 1, unit,
                                              out.ctypes.data))
        return out[:int(o[-1])]

    # ---- training rows (TD_ROWS_*) ------------------------------------------------------------------
    @staticmethod
    def _rows_buffers(kind: str, spec: RowsSpec, rows: int, n_docs: int, *want: bool):
        """The host outputs of a rows call -> (arrays, their addresses, counts): ids, then positions and the further outputs of
        `kind` where wanted (None otherwise).  "rows": aux; "pack": cu_seqlens, row_lengths, seg_docs; "windows": row_lengths,
        row_docs, row_starts."""
        slots, nseg = rows * spec.seq_len, n_docs + 2 * rows + 1
        sizes = {"rows": [(n_docs + rows + 1 if spec.layout == TD_ROWS_CONCAT else n_docs, np.int32)],
                 "pack": [(nseg, np.int32), (rows, np.int32), (nseg, np.int64)],
                 "windows": [(rows, np.int32), (rows, np.int64), (rows, np.int64)]}[kind]
        b = [np.empty(max(n, 1), dtype=dt) if w else None for w, (n, dt) in zip((True, *want), [(slots, np.int32)] * 2 + sizes)]
        return b, [x.ctypes.data if x is not None else None for x in b], np.zeros(4, dtype=np.int64)

    @staticmethod
    def _rows_result(kind: str, spec: RowsSpec, b, counts, n_docs: int):
        """The arrays of _rows_buffers cut to what the call wrote: ids and positions as [rows, S], the further outputs, counts."""
        r, S, c2 = int(counts[0]), spec.seq_len, int(counts[2])
        lens = {"rows": [c2 + 1 if spec.layout == TD_ROWS_CONCAT else n_docs], "pack": [c2 + 1, r, c2], "windows": [r, r, r]}[kind]
        return (*(x[:r * S].reshape(r, S).copy() if x is not None else None for x in b[:2]),
                *(x[:n].copy() if x is not None else None for x, n in zip(b[2:], lens)), counts)

    def make_rows(self, ids, tok_offsets, spec: RowsSpec, positions: bool = False, aux: bool = True, rows_capacity: int | None = None):
        """td_make_rows -> (ids int32[rows, S], positions int32[rows, S] or None, aux or None, counts int64[4]).
        aux: cu_seqlens (CONCAT, int32[n_seg + 1]) or lengths (PAD, int32[n_docs])."""
        t = np.ascontiguousarray(ids, dtype=np.int32)
        o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
        n_docs = len(o) - 1
        rows = rows_capacity if rows_capacity is not None else rows_capacity_of(spec, int(o[-1]) if len(o) else 0, n_docs)
        b, (d_out, d_pos, d_aux), counts = self._rows_buffers("rows", spec, rows, n_docs, positions, aux)
        self._check(self._lib.td_make_rows(self._h, t.ctypes.data if len(t) else None, len(t), o.ctypes.data, n_docs, ctypes.byref(spec),
                                           d_out, rows, d_pos, d_aux, counts.ctypes.data))
        return self._rows_result("rows", spec, b, counts, n_docs)

    def make_rows_device(self, d_ids: int, n_tokens: int, d_tok_offsets: int, n_docs: int, spec: RowsSpec, d_out_ids: int,
                         rows_capacity: int, d_positions: int = 0, d_aux: int = 0, d_counts: int = 0, stream: int = 0):
        """td_make_rows_device: raw device pointers, asynchronous on `stream`; check with device_status(stream)."""
        self._check(self._lib.td_make_rows_device(self._h, d_ids or None, n_tokens, d_tok_offsets, n_docs, ctypes.byref(spec), d_out_ids or None,
                                                  rows_capacity, d_positions or None, d_aux or None, d_counts or None, stream or None))

    def encode_batch_rows(self, text, doc_offsets, spec: RowsSpec, mode: int = TD_MODE_ENCODE, positions: bool = False, aux: bool = True,
                          rows_capacity: int | None = None):
        """td_encode_batch_rows: encode + td_make_rows in one call; same result tuple as make_rows.  The default capacity is
        the most rows the text can need (one id per byte)."""
        buf = _as_u8(text)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        n_docs = len(offs) - 1
        rows = rows_capacity if rows_capacity is not None else rows_capacity_of(spec, int(offs[-1]) if len(offs) else 0, n_docs)
        b, (d_out, d_pos, d_aux), counts = self._rows_buffers("rows", spec, rows, n_docs, positions, aux)
        self._check(self._lib.td_encode_batch_rows(self._h, buf.ctypes.data if len(buf) else None, offs.ctypes.data, n_docs, mode,
                                                   ctypes.byref(spec), d_out, rows, d_pos, d_aux, counts.ctypes.data))
        return self._rows_result("rows", spec, b, counts, n_docs)

    # ---- best-fit rows (TD_ROWS_BESTFIT) --------------------------------------------------------------------
    def pack_rows(self, ids, tok_offsets, spec: RowsSpec, positions: bool = False, cu_seqlens: bool = True, lengths: bool = False,
                  docs: bool = False, rows_capacity: int | None = None):
        """td_pack_rows -> (ids int32[rows, S], positions int32[rows, S] | None, cu_seqlens int32[segs + 1] | None,
        row_lengths int32[rows] | None, seg_docs int64[segs] | None, counts int64[4]).  The default capacity is the exact rows
        (td_pack_plan)."""
        t = np.ascontiguousarray(ids, dtype=np.int32)
        o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
        n_docs = len(o) - 1
        rows = rows_capacity if rows_capacity is not None else int(pack_plan(o, spec)[0])
        b, addr, counts = self._rows_buffers("pack", spec, rows, n_docs, positions, cu_seqlens, lengths, docs)
        outs = PackOutputs(*addr)
        self._check(self._lib.td_pack_rows(self._h, t.ctypes.data if len(t) else None, len(t), o.ctypes.data, n_docs, ctypes.byref(spec),
                                           ctypes.byref(outs), rows, counts.ctypes.data))
        return self._rows_result("pack", spec, b, counts, n_docs)

    def pack_rows_device(self, d_ids: int, n_tokens: int, d_tok_offsets: int, n_docs: int, spec: RowsSpec, d_out_ids: int,
                         rows_capacity: int, d_positions: int = 0, d_cu_seqlens: int = 0, d_row_lengths: int = 0, d_seg_docs: int = 0,
                         stream: int = 0) -> np.ndarray:
        """td_pack_rows_device: raw device pointers.  Synchronises once on `stream` to plan; returns counts int64[4] (host);
        the output kernels then run asynchronously on `stream`."""
        outs = PackOutputs(d_out_ids or None, d_positions or None, d_cu_seqlens or None, d_row_lengths or None, d_seg_docs or None)
        counts = np.zeros(4, dtype=np.int64)
        rc = self._lib.td_pack_rows_device(self._h, d_ids or None, n_tokens, d_tok_offsets, n_docs, ctypes.byref(spec), ctypes.byref(outs),
                                           rows_capacity, counts.ctypes.data, stream or None)
        try:
            self._check(rc)
        except TokenDaggerHipError as ex:
            ex.counts = counts  # (TD_E_CAPACITY: counts[0] = the rows needed)
            raise
        return counts

    def encode_batch_pack_rows(self, text, doc_offsets, spec: RowsSpec, mode: int = TD_MODE_ENCODE, positions: bool = False,
                               cu_seqlens: bool = True, lengths: bool = False, docs: bool = False, rows_capacity: int | None = None):
        """td_encode_batch_pack_rows: encode + td_pack_rows in one call; same result tuple as pack_rows.  The default capacity is
        the bound for the most ids the text can give (one per byte)."""
        buf = _as_u8(text)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        n_docs = len(offs) - 1
        rows = rows_capacity if rows_capacity is not None else pack_rows_capacity_of(spec, int(offs[-1]) if len(offs) else 0, n_docs)
        if rows_capacity is None and cu_seqlens:
            rows = min(rows, ((1 << 31) - 1) // spec.seq_len)  # (cu_seqlens entries are int32)
        b, addr, counts = self._rows_buffers("pack", spec, rows, n_docs, positions, cu_seqlens, lengths, docs)
        outs = PackOutputs(*addr)
        self._check(self._lib.td_encode_batch_pack_rows(self._h, buf.ctypes.data if len(buf) else None, offs.ctypes.data, n_docs, mode,
                                                        ctypes.byref(spec), ctypes.byref(outs), rows, counts.ctypes.data))
        return self._rows_result("pack", spec, b, counts, n_docs)

    # ---- window rows (TD_ROWS_WINDOWS) ------------------------------------------------------------------------
    def window_rows(self, ids, tok_offsets, spec: RowsSpec, overlap: int = 0, positions: bool = False, lengths: bool = True,
                    docs: bool = True, starts: bool = True, rows_capacity: int | None = None):
        """td_window_rows -> (ids int32[rows, S], positions int32[rows, S] | None, row_lengths int32[rows] | None,
        row_docs int64[rows] | None, row_starts int64[rows] | None, counts int64[4]).  The default capacity is the exact rows
        (td_window_plan)."""
        t = np.ascontiguousarray(ids, dtype=np.int32)
        o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
        n_docs = len(o) - 1
        rows = rows_capacity if rows_capacity is not None else int(window_plan(o, spec, overlap)[0])
        b, addr, counts = self._rows_buffers("windows", spec, rows, n_docs, positions, lengths, docs, starts)
        outs = WindowOutputs(*addr)
        rc = self._lib.td_window_rows(self._h, t.ctypes.data if len(t) else None, len(t), o.ctypes.data, n_docs, ctypes.byref(spec), overlap,
                                      ctypes.byref(outs), rows, counts.ctypes.data)
        try:
            self._check(rc)
        except TokenDaggerHipError as ex:
            ex.counts = counts  # (TD_E_CAPACITY: counts[0] = the rows needed)
            raise
        return self._rows_result("windows", spec, b, counts, n_docs)

    def window_rows_device(self, d_ids: int, n_tokens: int, d_tok_offsets: int, n_docs: int, spec: RowsSpec, overlap: int, d_out_ids: int,
                           rows_capacity: int, d_positions: int = 0, d_row_lengths: int = 0, d_row_docs: int = 0, d_row_starts: int = 0,
                           d_counts: int = 0, stream: int = 0):
        """td_window_rows_device: raw device pointers, asynchronous on `stream`; check with device_status(stream)."""
        outs = WindowOutputs(d_out_ids or None, d_positions or None, d_row_lengths or None, d_row_docs or None, d_row_starts or None)
        self._check(self._lib.td_window_rows_device(self._h, d_ids or None, n_tokens, d_tok_offsets, n_docs, ctypes.byref(spec), overlap,
                                                    ctypes.byref(outs), rows_capacity, d_counts or None, stream or None))

    def encode_batch_window_rows(self, text, doc_offsets, spec: RowsSpec, overlap: int = 0, mode: int = TD_MODE_ENCODE,
                                 positions: bool = False, lengths: bool = True, docs: bool = True, starts: bool = True,
                                 rows_capacity: int | None = None):
        """td_encode_batch_window_rows: encode + td_window_rows in one call; same result tuple as window_rows.  The default
        capacity is the most rows the text can need (one id per byte: every document one row, and one more per `step` ids)."""
        buf = _as_u8(text)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        n_docs = len(offs) - 1
        step = spec.seq_len - (spec.bos_id >= 0) - (spec.eos_id >= 0) - overlap
        rows = rows_capacity if rows_capacity is not None else n_docs + (int(offs[-1]) if len(offs) else 0) // max(step, 1)
        b, addr, counts = self._rows_buffers("windows", spec, rows, n_docs, positions, lengths, docs, starts)
        outs = WindowOutputs(*addr)
        self._check(self._lib.td_encode_batch_window_rows(self._h, buf.ctypes.data if len(buf) else None, offs.ctypes.data, n_docs, mode,
                                                          ctypes.byref(spec), overlap, ctypes.byref(outs), rows, counts.ctypes.data))
        return self._rows_result("windows", spec, b, counts, n_docs)

    # ---- loss labels (td_labels_spec) ----------------------------------------------------------------------------
    def span_labels(self, ids, tok_offsets, spec: LabelsSpec, mask: bool = False, trained_offsets: bool = False, n_tokens: int | None = None):
        """td_span_labels -> (labels int32[total], mask uint8[total] | None, trained_offsets int64[n_docs + 1] | None,
        counts int64[4] = trained ids, spans, unterminated documents, 0)."""
        t = np.ascontiguousarray(ids, dtype=np.int32)
        o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
        n_docs, total = len(o) - 1, int(o[-1])
        lab = np.empty(max(total, 1), dtype=np.int32)
        m = np.empty(max(total, 1), dtype=np.uint8) if mask else None
        to = np.empty(n_docs + 1, dtype=np.int64) if trained_offsets else None
        counts = np.zeros(4, dtype=np.int64)
        self._check(self._lib.td_span_labels(self._h, t.ctypes.data if len(t) else None, len(t) if n_tokens is None else n_tokens, o.ctypes.data,
                                             n_docs, ctypes.byref(spec), lab.ctypes.data, m.ctypes.data if mask else None,
                                             to.ctypes.data if trained_offsets else None, counts.ctypes.data))
        return lab[:total], m[:total] if mask else None, to, counts

    def span_labels_device(self, d_ids: int, n_tokens: int, d_tok_offsets: int, n_docs: int, spec: LabelsSpec, d_labels: int, d_mask: int = 0,
                           d_trained_offsets: int = 0, d_counts: int = 0, stream: int = 0):
        """td_span_labels_device: raw device pointers, asynchronous on `stream`; check with device_status(stream)."""
        self._check(self._lib.td_span_labels_device(self._h, d_ids or None, n_tokens, d_tok_offsets, n_docs, ctypes.byref(spec), d_labels or None,
                                                    d_mask or None, d_trained_offsets or None, d_counts or None, stream or None))

    def encode_batch_span_labels(self, text, doc_offsets, allowed, spec: LabelsSpec, mask: bool = False, trained_offsets: bool = False):
        """td_encode_batch_span_labels: encode_batch_with_special_strs + span_labels in one call ->
        (tokens int32[total], offsets int64[n_docs + 1], labels, mask | None, trained_offsets | None, counts)."""
        buf = _as_u8(text)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        ab, ao = self._pack_strs(list(allowed))
        n_docs = len(offs) - 1
        n = int(offs[-1]) if len(offs) else 0
        cap = n + 16
        out_offs = np.empty(n_docs + 1, dtype=np.int64)
        toks, lab = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32)
        m = np.empty(cap, dtype=np.uint8) if mask else None
        to = np.empty(n_docs + 1, dtype=np.int64) if trained_offsets else None
        counts = np.zeros(4, dtype=np.int64)
        ntok = ctypes.c_int64(0)
        self._check(self._lib.td_encode_batch_span_labels(self._h, buf.ctypes.data if n else None, offs.ctypes.data, n_docs, ab.ctypes.data,
                                                          ao.ctypes.data, len(ao) - 1, ctypes.byref(spec), toks.ctypes.data, cap,
                                                          out_offs.ctypes.data, lab.ctypes.data, m.ctypes.data if mask else None,
                                                          to.ctypes.data if trained_offsets else None, counts.ctypes.data, ctypes.byref(ntok)))
        k = ntok.value
        return toks[:k].copy(), out_offs, lab[:k].copy(), m[:k].copy() if mask else None, to, counts

    # ---- loss labels from byte ranges (td_range_spec) ------------------------------------------------------------
    range_spec = staticmethod(range_spec)
    range_plan = staticmethod(range_plan)

    def range_labels(self, ids, tok_offsets, ranges, spec: RangeSpec, mask: bool = False, trained_offsets: bool = False, starts=None,
                     n_tokens: int | None = None):
        """td_range_labels -> (labels int32[total], mask uint8[total] | None, trained_offsets int64[n_docs + 1] | None,
        counts int64[4] = trained ids, partially marked ids, marked bytes, 0).  ranges: see as_ranges.  starts None: the covered
        form; else int64 byte starts, one per id."""
        t = np.ascontiguousarray(ids, dtype=np.int32)
        o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
        n_docs, total = len(o) - 1, int(o[-1])
        ro, rg = as_ranges(ranges, n_docs)
        st = None if starts is None else np.ascontiguousarray(starts, dtype=np.int64)
        if st is not None and len(st) < total:
            raise ValueError("starts must have an entry for every id")
        lab = np.empty(max(total, 1), dtype=np.int32)
        m = np.empty(max(total, 1), dtype=np.uint8) if mask else None
        to = np.empty(n_docs + 1, dtype=np.int64) if trained_offsets else None
        counts = np.zeros(4, dtype=np.int64)
        self._check(self._lib.td_range_labels(self._h, t.ctypes.data if len(t) else None, len(t) if n_tokens is None else n_tokens, o.ctypes.data,
                                              n_docs, st.ctypes.data if st is not None and len(st) else None, ro.ctypes.data,
                                              rg.ctypes.data if len(rg) else None, ctypes.byref(spec), lab.ctypes.data,
                                              m.ctypes.data if mask else None, to.ctypes.data if trained_offsets else None, counts.ctypes.data))
        return lab[:total], m[:total] if mask else None, to, counts

    def range_labels_device(self, d_ids: int, n_tokens: int, d_tok_offsets: int, n_docs: int, d_range_offsets: int, d_ranges: int, n_ranges: int,
                            spec: RangeSpec, d_labels: int, d_mask: int = 0, d_trained_offsets: int = 0, d_counts: int = 0, d_starts: int = 0,
                            stream: int = 0):
        """td_range_labels_device: raw device pointers, asynchronous on `stream`; check with device_status(stream)."""
        self._check(self._lib.td_range_labels_device(self._h, d_ids or None, n_tokens, d_tok_offsets, n_docs, d_starts or None, d_range_offsets,
                                                     d_ranges or None, n_ranges, ctypes.byref(spec), d_labels or None, d_mask or None,
                                                     d_trained_offsets or None, d_counts or None, stream or None))

    def encode_batch_range_labels(self, text, doc_offsets, allowed, ranges, spec: RangeSpec, mask: bool = False, trained_offsets: bool = False):
        """td_encode_batch_range_labels: encode_batch_with_special_strs + range_labels (covered form) in one call ->
        (tokens int32[total], offsets int64[n_docs + 1], labels, mask | None, trained_offsets | None, counts)."""
        buf = _as_u8(text)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        ab, ao = self._pack_strs(list(allowed))
        n_docs = len(offs) - 1
        ro, rg = as_ranges(ranges, n_docs)
        n = int(offs[-1]) if len(offs) else 0
        cap = n + 16
        out_offs = np.empty(n_docs + 1, dtype=np.int64)
        toks, lab = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32)
        m = np.empty(cap, dtype=np.uint8) if mask else None
        to = np.empty(n_docs + 1, dtype=np.int64) if trained_offsets else None
        counts = np.zeros(4, dtype=np.int64)
        ntok = ctypes.c_int64(0)
        self._check(self._lib.td_encode_batch_range_labels(self._h, buf.ctypes.data if n else None, offs.ctypes.data, n_docs, ab.ctypes.data,
                                                           ao.ctypes.data, len(ao) - 1, ro.ctypes.data, rg.ctypes.data if len(rg) else None,
                                                           ctypes.byref(spec), toks.ctypes.data, cap, out_offs.ctypes.data, lab.ctypes.data,
                                                           m.ctypes.data if mask else None, to.ctypes.data if trained_offsets else None,
                                                           counts.ctypes.data, ctypes.byref(ntok)))
        k = ntok.value
        return toks[:k].copy(), out_offs, lab[:k].copy(), m[:k].copy() if mask else None, to, counts

    # ---- label rows (td_rows_labels): the labeled form of the row calls ---------------------------------------------
    def _check_counts(self, rc: int, counts):
        try:
            self._check(rc)
        except TokenDaggerHipError as ex:
            ex.counts = counts  # (TD_E_CAPACITY: counts[0] = the rows needed)
            raise

    def _labeled_host(self, kind: str, fn, ids, labels, tok_offsets, spec: RowsSpec, lab: RowsLabels, rows: int, want, extra=()):
        """A labeled host call: the result tuple of the counterpart, then the label rows int32[rows, S].  lab gives the fill values
        and the flags; its src / dst are set here."""
        t = np.ascontiguousarray(ids, dtype=np.int32)
        src = np.ascontiguousarray(labels, dtype=np.int32)
        o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
        n_docs = len(o) - 1
        if len(src) < len(t):
            raise ValueError("labels must have an entry for every id")
        b, addr, counts = self._rows_buffers(kind, spec, rows, n_docs, *want)
        dst = np.empty(max(rows * spec.seq_len, 1), dtype=np.int32)
        lab = RowsLabels((src if len(src) else np.zeros(1, np.int32)).ctypes.data, dst.ctypes.data, lab.bos_value, lab.eos_value,
                         lab.pad_value, lab.flags)
        outs = {"rows": None, "pack": PackOutputs, "windows": WindowOutputs}[kind]
        head = (self._h, t.ctypes.data if len(t) else None, len(t), o.ctypes.data, n_docs, ctypes.byref(spec))
        if outs is None:
            rc = fn(*head, addr[0], rows, addr[1], addr[2], counts.ctypes.data, ctypes.byref(lab))
        else:
            rc = fn(*head, *extra, ctypes.byref(outs(*addr)), rows, counts.ctypes.data, ctypes.byref(lab))
        self._check_counts(rc, counts)
        r = int(counts[0])
        return (*self._rows_result(kind, spec, b, counts, n_docs), dst[:r * spec.seq_len].reshape(r, spec.seq_len).copy())

    def make_rows_labeled(self, ids, labels, tok_offsets, spec: RowsSpec, lab: RowsLabels, positions: bool = False, aux: bool = True,
                          rows_capacity: int | None = None):
        """td_make_rows_labeled -> make_rows' tuple (ids, positions, aux, counts) and the label rows int32[rows, S]."""
        o = np.asarray(tok_offsets, dtype=np.int64)
        rows = rows_capacity if rows_capacity is not None else rows_capacity_of(spec, int(o[-1]) if len(o) else 0, len(o) - 1)
        return self._labeled_host("rows", self._lib.td_make_rows_labeled, ids, labels, o, spec, lab, rows, (positions, aux))

    def pack_rows_labeled(self, ids, labels, tok_offsets, spec: RowsSpec, lab: RowsLabels, positions: bool = False, cu_seqlens: bool = True,
                          lengths: bool = False, docs: bool = False, rows_capacity: int | None = None):
        """td_pack_rows_labeled -> pack_rows' tuple and the label rows int32[rows, S]."""
        o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
        rows = rows_capacity if rows_capacity is not None else int(pack_plan(o, spec)[0])
        return self._labeled_host("pack", self._lib.td_pack_rows_labeled, ids, labels, o, spec, lab, rows, (positions, cu_seqlens, lengths, docs))

    def window_rows_labeled(self, ids, labels, tok_offsets, spec: RowsSpec, lab: RowsLabels, overlap: int = 0, positions: bool = False,
                            lengths: bool = True, docs: bool = True, starts: bool = True, rows_capacity: int | None = None):
        """td_window_rows_labeled -> window_rows' tuple and the label rows int32[rows, S]."""
        o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
        rows = rows_capacity if rows_capacity is not None else int(window_plan(o, spec, overlap)[0])
        return self._labeled_host("windows", self._lib.td_window_rows_labeled, ids, labels, o, spec, lab, rows,
                                  (positions, lengths, docs, starts), extra=(overlap,))

    def make_rows_labeled_device(self, d_ids: int, n_tokens: int, d_tok_offsets: int, n_docs: int, spec: RowsSpec, d_out_ids: int,
                                 rows_capacity: int, lab: RowsLabels, d_positions: int = 0, d_aux: int = 0, d_counts: int = 0, stream: int = 0):
        """td_make_rows_labeled_device: raw device pointers (lab.src / lab.dst too), asynchronous on `stream`."""
        self._check(self._lib.td_make_rows_labeled_device(self._h, d_ids or None, n_tokens, d_tok_offsets, n_docs, ctypes.byref(spec),
                                                          d_out_ids or None, rows_capacity, d_positions or None, d_aux or None,
                                                          d_counts or None, stream or None, ctypes.byref(lab)))

    def pack_rows_labeled_device(self, d_ids: int, n_tokens: int, d_tok_offsets: int, n_docs: int, spec: RowsSpec, d_out_ids: int,
                                 rows_capacity: int, lab: RowsLabels, d_positions: int = 0, d_cu_seqlens: int = 0, d_row_lengths: int = 0,
                                 d_seg_docs: int = 0, stream: int = 0) -> np.ndarray:
        """td_pack_rows_labeled_device: raw device pointers; synchronises once on `stream` to plan; returns counts int64[4]."""
        outs = PackOutputs(d_out_ids or None, d_positions or None, d_cu_seqlens or None, d_row_lengths or None, d_seg_docs or None)
        counts = np.zeros(4, dtype=np.int64)
        rc = self._lib.td_pack_rows_labeled_device(self._h, d_ids or None, n_tokens, d_tok_offsets, n_docs, ctypes.byref(spec),
                                                   ctypes.byref(outs), rows_capacity, counts.ctypes.data, stream or None, ctypes.byref(lab))
        self._check_counts(rc, counts)
        return counts

    def window_rows_labeled_device(self, d_ids: int, n_tokens: int, d_tok_offsets: int, n_docs: int, spec: RowsSpec, overlap: int,
                                   d_out_ids: int, rows_capacity: int, lab: RowsLabels, d_positions: int = 0, d_row_lengths: int = 0,
                                   d_row_docs: int = 0, d_row_starts: int = 0, d_counts: int = 0, stream: int = 0):
        """td_window_rows_labeled_device: raw device pointers (lab.src / lab.dst too), asynchronous on `stream`."""
        outs = WindowOutputs(d_out_ids or None, d_positions or None, d_row_lengths or None, d_row_docs or None, d_row_starts or None)
        self._check(self._lib.td_window_rows_labeled_device(self._h, d_ids or None, n_tokens, d_tok_offsets, n_docs, ctypes.byref(spec),
                                                            overlap, ctypes.byref(outs), rows_capacity, d_counts or None, stream or None,
                                                            ctypes.byref(lab)))

    def _encode_label_rows(self, fn, text, doc_offsets, allowed, lspec_args, rspec: RowsSpec, lab: RowsLabels, overlap, positions, aux, lengths,
                           docs, starts, rows_capacity):
        """The body of the two text-to-label-rows calls; lspec_args: what `fn` takes between the allowed strings and the rows spec."""
        buf = _as_u8(text)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        ab, ao = self._pack_strs(list(allowed))
        n_docs = len(offs) - 1
        n = int(offs[-1]) if len(offs) else 0
        lay, S = rspec.layout, rspec.seq_len
        k = (rspec.bos_id >= 0) + (rspec.eos_id >= 0)
        if rows_capacity is not None:
            rows = rows_capacity
        elif lay == TD_ROWS_BESTFIT:
            rows = pack_rows_capacity_of(rspec, n, n_docs)
            if aux:
                rows = min(rows, ((1 << 31) - 1) // max(S, 1))
        elif lay == TD_ROWS_WINDOWS:
            rows = n_docs + n // max(S - k - overlap, 1)
        else:
            rows = rows_capacity_of(rspec, n, n_docs)
        kind = {TD_ROWS_BESTFIT: "pack", TD_ROWS_WINDOWS: "windows"}.get(lay, "rows")
        want = {"rows": (positions, aux), "pack": (positions, aux, lengths, docs), "windows": (positions, lengths, docs, starts)}[kind]
        b, addr, counts = self._rows_buffers(kind, rspec, rows, n_docs, *want)
        dst = np.empty(max(rows * S, 1), dtype=np.int32)
        none = None
        outs = {"rows": lambda: LabelRowsOutputs(addr[0], dst.ctypes.data, addr[1], addr[2], none, none, none, none),
                "pack": lambda: LabelRowsOutputs(addr[0], dst.ctypes.data, addr[1], addr[2], addr[3], addr[4], none, none),
                "windows": lambda: LabelRowsOutputs(addr[0], dst.ctypes.data, addr[1], none, addr[2], none, addr[3], addr[4])}[kind]()
        lcounts = np.zeros(4, dtype=np.int64)
        rc = fn(self._h, buf.ctypes.data if n else None, offs.ctypes.data, n_docs, ab.ctypes.data, ao.ctypes.data, len(ao) - 1, *lspec_args,
                ctypes.byref(rspec), overlap, ctypes.byref(lab), ctypes.byref(outs), rows, counts.ctypes.data, lcounts.ctypes.data)
        self._check_counts(rc, counts)
        r = int(counts[0])
        return (*self._rows_result(kind, rspec, b, counts, n_docs), dst[:r * S].reshape(r, S).copy(), lcounts)

    def encode_batch_span_label_rows(self, text, doc_offsets, allowed, lspec: LabelsSpec, rspec: RowsSpec, lab: RowsLabels, overlap: int = 0,
                                     positions: bool = False, aux: bool = True, lengths: bool = True, docs: bool = True, starts: bool = True,
                                     rows_capacity: int | None = None):
        """td_encode_batch_span_label_rows: chat text -> the layout's result tuple (as make_rows / pack_rows / window_rows give it,
        counts = the row counts), then the label rows int32[rows, S] and the labels' counts int64[4].  The default capacity is the
        most rows the text can need (one id per byte)."""
        return self._encode_label_rows(self._lib.td_encode_batch_span_label_rows, text, doc_offsets, allowed, (ctypes.byref(lspec),), rspec, lab,
                                       overlap, positions, aux, lengths, docs, starts, rows_capacity)

    def encode_batch_range_label_rows(self, text, doc_offsets, allowed, ranges, rgspec: RangeSpec, rspec: RowsSpec, lab: RowsLabels,
                                      overlap: int = 0, positions: bool = False, aux: bool = True, lengths: bool = True, docs: bool = True,
                                      starts: bool = True, rows_capacity: int | None = None):
        """td_encode_batch_range_label_rows: text and byte ranges -> what encode_batch_span_label_rows returns."""
        ro, rg = as_ranges(ranges, len(doc_offsets) - 1)
        return self._encode_label_rows(self._lib.td_encode_batch_range_label_rows, text, doc_offsets, allowed,
                                       (ro.ctypes.data, rg.ctypes.data if len(rg) else None, ctypes.byref(rgspec)), rspec, lab, overlap, positions,
                                       aux, lengths, docs, starts, rows_capacity)

    # ---- document selection (td_select_spec) ------------------------------------------------------------------
    def select_docs(self, ids, tok_offsets, sel=None, spec: SelectSpec | None = None, labels=None, docs: bool = True,
                    ids_capacity: int | None = None):
        """td_select_docs -> (ids int32[T], labels int32[T] | None, offsets int64[K + 1], docs int64[K] | None, counts int64[4]).
        sel None: the identity; labels: a second int32 stream moved by the same indices.  The default capacity is the exact T
        (td_select_plan).  An error carries .counts (TD_E_CAPACITY: counts[1] = the ids needed)."""
        spec = spec if spec is not None else select_spec()
        t = np.ascontiguousarray(ids, dtype=np.int32)
        o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32)
        if lab is not None and len(lab) != len(t):
            raise ValueError("labels must have one entry per id")
        n_docs = len(o) - 1
        sl = _sel_array(sel)
        n_sel = n_docs if sl is None else len(sl)
        cap = ids_capacity if ids_capacity is not None else int(select_plan(o, sl, spec, outputs=False)[1])
        out = np.empty(max(cap, 1), dtype=np.int32)
        out_lab = np.empty(max(cap, 1), dtype=np.int32) if lab is not None else None
        offs = np.empty(n_sel + 1, dtype=np.int64)
        dcs = np.empty(max(n_sel, 1), dtype=np.int64) if docs else None
        counts = np.zeros(4, dtype=np.int64)
        rc = self._lib.td_select_docs(self._h, t.ctypes.data if len(t) else None, lab.ctypes.data if lab is not None else None, len(t),
                                      o.ctypes.data, n_docs, sl.ctypes.data if sl is not None else None, n_sel, ctypes.byref(spec),
                                      out.ctypes.data, out_lab.ctypes.data if lab is not None else None, cap, offs.ctypes.data,
                                      dcs.ctypes.data if docs else None, counts.ctypes.data)
        self._check_counts(rc, counts)
        k, n = int(counts[0]), int(counts[1])
        return out[:n], (out_lab[:n] if lab is not None else None), offs[:k + 1], (dcs[:k] if docs else None), counts

    def select_docs_device(self, d_ids: int, n_tokens: int, d_tok_offsets: int, n_docs: int, d_sel: int, n_sel: int, spec: SelectSpec,
                           d_out_ids: int, ids_capacity: int, d_out_offsets: int, d_out_docs: int = 0, d_counts: int = 0, d_labels: int = 0,
                           d_out_labels: int = 0, stream: int = 0):
        """td_select_docs_device: raw device pointers (d_sel 0: the identity), asynchronous on `stream`; check with device_status(stream)."""
        self._check(self._lib.td_select_docs_device(self._h, d_ids or None, d_labels or None, n_tokens, d_tok_offsets, n_docs, d_sel or None,
                                                    n_sel, ctypes.byref(spec), d_out_ids or None, d_out_labels or None, ids_capacity,
                                                    d_out_offsets or None, d_out_docs or None, d_counts or None, stream or None))

    def encode_batch_select(self, text, doc_offsets, sel=None, spec: SelectSpec | None = None, mode: int = TD_MODE_ENCODE, docs: bool = True,
                            ids_capacity: int | None = None):
        """td_encode_batch_select: encode + td_select_docs in one call -> (ids, offsets, docs | None, counts).  The default capacity
        is the most ids the listed documents can have (one per byte)."""
        spec = spec if spec is not None else select_spec()
        buf = _as_u8(text)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        n_docs = len(offs) - 1
        sl = _sel_array(sel)
        n_sel = n_docs if sl is None else len(sl)
        if ids_capacity is not None:
            cap = ids_capacity
        elif sl is None:
            cap = int(offs[-1]) if len(offs) else 0
        else:
            ok = sl[(sl >= 0) & (sl < n_docs)]
            cap = int(np.diff(offs)[ok].sum())
        out = np.empty(max(cap, 1), dtype=np.int32)
        o_out = np.empty(n_sel + 1, dtype=np.int64)
        dcs = np.empty(max(n_sel, 1), dtype=np.int64) if docs else None
        counts = np.zeros(4, dtype=np.int64)
        rc = self._lib.td_encode_batch_select(self._h, buf.ctypes.data if len(buf) else None, offs.ctypes.data, n_docs, mode,
                                              sl.ctypes.data if sl is not None else None, n_sel, ctypes.byref(spec), out.ctypes.data, cap,
                                              o_out.ctypes.data, dcs.ctypes.data if docs else None, counts.ctypes.data)
        self._check_counts(rc, counts)
        k, n = int(counts[0]), int(counts[1])
        return out[:n], o_out[:k + 1], (dcs[:k] if docs else None), counts

    # ---- field joins (td_join_spec) ---------------------------------------------------------------------------
    @staticmethod
    def _join_buffers(cap: int, n_ex: int, K: int, labels: bool, types: bool, examples: bool, field_len: bool):
        b = {"ids": np.empty(max(cap, 1), dtype=np.int32),
             "labels": np.empty(max(cap, 1), dtype=np.int32) if labels else None,
             "types": np.empty(max(cap, 1), dtype=np.int32) if types else None,
             "offsets": np.empty(n_ex + 1, dtype=np.int64),
             "examples": np.empty(max(n_ex, 1), dtype=np.int64) if examples else None,
             "field_len": np.empty(max(n_ex, 1) * K, dtype=np.int32) if field_len else None}
        p = lambda a: a.ctypes.data if a is not None else None
        return b, JoinOutputs(p(b["ids"]), p(b["labels"]), p(b["types"]), cap, p(b["offsets"]), p(b["examples"]), p(b["field_len"]))

    @staticmethod
    def _join_result(b, counts, K: int):
        e, n = int(counts[0]), int(counts[1])
        cut = lambda a, k: a[:k] if a is not None else None
        fl = b["field_len"]
        return (b["ids"][:n], cut(b["labels"], n), cut(b["types"], n), b["offsets"][:e + 1], cut(b["examples"], e),
                fl[:e * K].reshape(e, K) if fl is not None else None, counts)

    def join_fields(self, ids, tok_offsets, spec: JoinSpec, labels: bool = True, types: bool = False, examples: bool = True,
                    field_len: bool = False, ids_capacity: int | None = None):
        """td_join_fields -> (ids int32[T], labels int32[T] | None, types int32[T] | None, offsets int64[E + 1], examples int64[E] |
        None, field_len int32[E, K] | None, counts int64[4]).  The default capacity is the exact T (td_join_plan).  An error carries
        .counts (TD_E_CAPACITY: counts[1] = the ids needed)."""
        t = np.ascontiguousarray(ids, dtype=np.int32)
        o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
        n_docs = len(o) - 1
        K = max(int(spec.n_fields), 1)
        cap = ids_capacity if ids_capacity is not None else int(join_plan(o, spec, outputs=False)[1])
        b, outs = self._join_buffers(cap, n_docs // K, K, labels, types, examples, field_len)
        counts = np.zeros(4, dtype=np.int64)
        rc = self._lib.td_join_fields(self._h, t.ctypes.data if len(t) else None, len(t), o.ctypes.data, n_docs, ctypes.byref(spec),
                                      ctypes.byref(outs), counts.ctypes.data)
        self._check_counts(rc, counts)
        return self._join_result(b, counts, K)

    def join_fields_device(self, d_ids: int, n_tokens: int, d_tok_offsets: int, n_docs: int, spec: JoinSpec, d_out_ids: int,
                           ids_capacity: int, d_out_offsets: int, d_counts: int, d_out_labels: int = 0, d_out_types: int = 0,
                           d_out_examples: int = 0, d_out_field_len: int = 0, stream: int = 0):
        """td_join_fields_device: raw device pointers, asynchronous on `stream`; check with device_status(stream)."""
        outs = JoinOutputs(d_out_ids or None, d_out_labels or None, d_out_types or None, ids_capacity, d_out_offsets or None,
                           d_out_examples or None, d_out_field_len or None)
        self._check(self._lib.td_join_fields_device(self._h, d_ids or None, n_tokens, d_tok_offsets, n_docs, ctypes.byref(spec),
                                                    ctypes.byref(outs), d_counts or None, stream or None))

    def encode_batch_join(self, text, doc_offsets, spec: JoinSpec, mode: int = TD_MODE_ENCODE, labels: bool = True, types: bool = False,
                          examples: bool = True, field_len: bool = False, ids_capacity: int | None = None):
        """td_encode_batch_join: encode (no special token allowed) + td_join_fields in one call; the result of join_fields.  The
        default capacity is the most slots the examples can have (one id per byte, and every literal)."""
        buf = _as_u8(text)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        n_docs = len(offs) - 1
        K = max(int(spec.n_fields), 1)
        n_ex = n_docs // K
        fixed = int(spec.n_tail) + sum(int(spec.fields[f].n_before) for f in range(min(K, TD_JOIN_MAX_FIELDS)))
        cap = ids_capacity if ids_capacity is not None else (int(offs[-1]) if len(offs) else 0) + max(fixed, 0) * n_ex
        b, outs = self._join_buffers(cap, n_ex, K, labels, types, examples, field_len)
        counts = np.zeros(4, dtype=np.int64)
        rc = self._lib.td_encode_batch_join(self._h, buf.ctypes.data if len(buf) else None, offs.ctypes.data, n_docs, mode,
                                            ctypes.byref(spec), ctypes.byref(outs), counts.ctypes.data)
        self._check_counts(rc, counts)
        return self._join_result(b, counts, K)

    # ---- token counts (td_counts_spec) ------------------------------------------------------------------------
    def token_counts(self, ids, tok_offsets=None, groups=None, spec: CountsSpec | None = None, counts=None, n_tokens: int | None = None):
        """td_token_counts -> (counts int64[n_groups, n_bins], info int64[4] = counted, negative, too_large, bad_group).  With
        TD_COUNTS_ACCUMULATE in the spec, `counts` is the array that is added to (and returned, reshaped)."""
        if spec is None:
            raise ValueError("a counts_spec is required")
        t, o, g, n_docs, counts, info = _counts_args(ids, tok_offsets, groups, spec, counts)
        self._check(self._lib.td_token_counts(self._h, t.ctypes.data if len(t) else None, len(t) if n_tokens is None else n_tokens,
                                              o.ctypes.data if o is not None else None, n_docs, g.ctypes.data if g is not None else None,
                                              ctypes.byref(spec), counts.ctypes.data, info.ctypes.data))
        return _counts_shape(counts, spec), info

    def token_counts_device(self, d_ids: int, n_tokens: int, d_tok_offsets: int, n_docs: int, d_doc_group: int, spec: CountsSpec, d_counts: int,
                            d_info: int, stream: int = 0):
        """td_token_counts_device: raw device pointers (d_tok_offsets, d_doc_group 0 with one group), asynchronous on `stream`; check
        with device_status(stream)."""
        self._check(self._lib.td_token_counts_device(self._h, d_ids or None, n_tokens, d_tok_offsets or None, n_docs, d_doc_group or None,
                                                     ctypes.byref(spec), d_counts or None, d_info or None, stream or None))

    def encode_batch_token_counts(self, text, doc_offsets, groups=None, spec: CountsSpec | None = None, mode: int = TD_MODE_ENCODE, counts=None):
        """td_encode_batch_token_counts: encode + token counts in one call, the ids stay on the device -> (counts, info, n_tokens)."""
        if spec is None:
            raise ValueError("a counts_spec is required")
        buf = _as_u8(text)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        _, _, g, n_docs, counts, info = _counts_args(np.zeros(0, dtype=np.int32), offs, groups, spec, counts)
        total = ctypes.c_int64(0)
        self._check(self._lib.td_encode_batch_token_counts(self._h, buf.ctypes.data if len(buf) else None, offs.ctypes.data, n_docs, mode,
                                                           g.ctypes.data if g is not None else None, ctypes.byref(spec), counts.ctypes.data,
                                                           info.ctypes.data, ctypes.byref(total)))
        return _counts_shape(counts, spec), info, int(total.value)

    # ---- n-gram matches (td_ngram_spec, td_ngram_set) ------------------------------------------------------------
    def ngram_set(self, sequences, offsets=None) -> NgramSet:
        """td_ngram_set_create: a list of id lists, or flat ids with offsets[n_pats + 1]."""
        return NgramSet(self, sequences, offsets)

    def ngram_matches(self, nset: NgramSet, ids, tok_offsets, spec: NgramSpec | None = None, cover: bool = True, labels=None,
                      doc_stats: bool = True, pattern_counts=False, n_tokens: int | None = None):
        """td_ngram_matches -> (cover | None, labels | None (the caller's, copied, with ignore_index where covered), doc_stats
        int64[n_docs, 2] | None, pattern_counts int64[n_pats] | None, counts int64[4])."""
        spec = spec if spec is not None else ngram_spec()
        t = np.ascontiguousarray(ids, dtype=np.int32)
        o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
        n_docs = len(o) - 1
        total = int(o[-1]) if 0 <= int(o[-1]) <= len(t) else 0
        cv, lb, ds, pc, counts = _ngram_outputs(total, n_docs, nset.n_pats, spec, cover, labels, doc_stats, pattern_counts)
        self._check(self._lib.td_ngram_matches(self._h, nset._h, t.ctypes.data if len(t) else None, len(t) if n_tokens is None else n_tokens,
                                               o.ctypes.data, n_docs, ctypes.byref(spec), _ptr(cv), _ptr(lb), _ptr(ds), _ptr(pc),
                                               counts.ctypes.data))
        return _ngram_result(total, n_docs, cv, lb, ds, pc, counts)

    def ngram_matches_device(self, nset: NgramSet, d_ids: int, n_tokens: int, d_tok_offsets: int, n_docs: int, spec: NgramSpec, d_cover: int,
                             d_labels: int, d_doc_stats: int, d_pattern_counts: int, d_counts: int, stream: int = 0):
        """td_ngram_matches_device: raw device pointers (0: that output is not wanted), asynchronous on `stream`; check with
        device_status(stream)."""
        self._check(self._lib.td_ngram_matches_device(self._h, nset._h, d_ids or None, n_tokens, d_tok_offsets or None, n_docs, ctypes.byref(spec),
                                                      d_cover or None, d_labels or None, d_doc_stats or None, d_pattern_counts or None,
                                                      d_counts or None, stream or None))

    def encode_batch_ngram_matches(self, text, doc_offsets, nset: NgramSet, spec: NgramSpec | None = None, mode: int = TD_MODE_ENCODE,
                                   doc_stats: bool = True, pattern_counts=False):
        """td_encode_batch_ngram_matches: encode + matches in one call, the ids stay on the device -> (doc_stats | None,
        pattern_counts | None, counts, n_tokens)."""
        spec = spec if spec is not None else ngram_spec()
        buf = _as_u8(text)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        n_docs = len(offs) - 1
        _, _, ds, pc, counts = _ngram_outputs(0, n_docs, nset.n_pats, spec, False, None, doc_stats, pattern_counts)
        total = ctypes.c_int64(0)
        self._check(self._lib.td_encode_batch_ngram_matches(self._h, buf.ctypes.data if len(buf) else None, offs.ctypes.data, n_docs, mode,
                                                            nset._h, ctypes.byref(spec), _ptr(ds), _ptr(pc), counts.ctypes.data,
                                                            ctypes.byref(total)))
        return (ds[:n_docs] if ds is not None else None), pc, counts, int(total.value)

    # ---- MinHash signatures (td_minhash_spec) -----------------------------------------------------------------------
    def minhash(self, ids, tok_offsets, spec: MinhashSpec | None = None, n_tokens: int | None = None):
        """td_minhash -> (sig uint32[n_docs, num_perm], band_keys uint64[n_docs, bands] | None, counts int64[4])."""
        spec = spec if spec is not None else minhash_spec()
        t, o, n_docs, (sig, keys, counts) = _minhash_args(ids, tok_offsets, spec)
        self._check(self._lib.td_minhash(self._h, t.ctypes.data if len(t) else None, len(t) if n_tokens is None else n_tokens, o.ctypes.data,
                                         n_docs, ctypes.byref(spec), sig.ctypes.data, _ptr(keys), counts.ctypes.data))
        return sig[:n_docs], (keys[:n_docs] if keys is not None else None), counts

    def minhash_device(self, d_ids: int, n_tokens: int, d_tok_offsets: int, n_docs: int, spec: MinhashSpec, d_sig: int, d_band_keys: int,
                       d_counts: int, stream: int):
        """td_minhash_device: raw device pointers (d_band_keys 0 with bands == 0), asynchronous on `stream`, which must not be the
        null stream; check with device_status(stream)."""
        self._check(self._lib.td_minhash_device(self._h, d_ids or None, n_tokens, d_tok_offsets or None, n_docs, ctypes.byref(spec),
                                                d_sig or None, d_band_keys or None, d_counts or None, stream or None))

    def encode_batch_minhash(self, text, doc_offsets, spec: MinhashSpec | None = None, mode: int = TD_MODE_ENCODE):
        """td_encode_batch_minhash: encode + signatures in one call, the ids stay on the device -> (sig, band_keys | None, counts,
        n_tokens)."""
        spec = spec if spec is not None else minhash_spec()
        buf = _as_u8(text)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        n_docs = len(offs) - 1
        sig, keys, counts = _minhash_outputs(n_docs, spec)
        total = ctypes.c_int64(0)
        self._check(self._lib.td_encode_batch_minhash(self._h, buf.ctypes.data if len(buf) else None, offs.ctypes.data, n_docs, mode,
                                                      ctypes.byref(spec), sig.ctypes.data, _ptr(keys), counts.ctypes.data, ctypes.byref(total)))
        return sig[:n_docs], (keys[:n_docs] if keys is not None else None), counts, int(total.value)

    # ---- Unicode NFC normalisation ------------------------------------------------------------------------------
    def nfc_check(self, d_text: int, n_bytes: int, d_doc_offsets: int, n_docs: int, d_flags: int, d_counts: int, stream: int):
        """td_nfc_check_device: raw device pointers, asynchronous on `stream`, which must not be the null stream; d_flags uint8[n_docs]
        (0: proven NFC), d_counts int64[8]; check with device_status(stream)."""
        self._check(self._lib.td_nfc_check_device(self._h, d_text or None, n_bytes, d_doc_offsets or None, n_docs, d_flags or None,
                                                  d_counts or None, stream or None))

    def nfc_device(self, d_text: int, n_bytes: int, d_doc_offsets: int, n_docs: int, d_out: int, out_capacity: int, d_out_doc_offsets: int,
                   d_changed: int, d_counts: int, stream: int):
        """td_nfc_device: raw device pointers (d_changed may be 0), asynchronous on `stream`; check with device_status(stream)."""
        self._check(self._lib.td_nfc_device(self._h, d_text or None, n_bytes, d_doc_offsets or None, n_docs, d_out or None, out_capacity,
                                            d_out_doc_offsets or None, d_changed or None, d_counts or None, stream or None))

    def nfc(self, text, doc_offsets, capacity: int | None = None, want_text: bool = True):
        """td_nfc: nfc_host's arguments and results, computed on the device."""
        buf, o, n_docs, ooff, flags, changed, counts = _rewrite_args(text, doc_offsets, _NFC_PER_DOC)
        cap = _rewrite_capacity(buf, o, capacity) if want_text else 0
        out = np.empty(max(cap, 1), dtype=np.uint8)
        rc = self._lib.td_nfc(self._h, buf.ctypes.data if len(buf) else None, o.ctypes.data, n_docs, out.ctypes.data if want_text else None, cap,
                              ooff.ctypes.data, flags.ctypes.data, changed.ctypes.data, counts.ctypes.data)
        if rc != TD_OK:
            _raise_with_counts(rc, self._lib.td_last_error(self._h).decode("utf-8", "replace"), counts)
        return (out[:int(counts[0])] if want_text else None), ooff, flags[:n_docs], changed[:n_docs], counts

    def encode_batch_nfc(self, text, doc_offsets, mode: int = TD_MODE_ENCODE, return_text: bool = False):
        """td_encode_batch_nfc: check, normalise where a document is flagged, encode -> (ids int32, tok_offsets int64[n_docs + 1],
        norm_text uint8 | None, norm_doc_offsets int64[n_docs + 1], changed uint8[n_docs], counts int64[8]).  Offsets refer to the
        normalised text."""
        buf, o, n_docs, noff, _, changed, counts = _rewrite_args(text, doc_offsets, _NFC_PER_DOC)
        rc, ids, toff, norm = _encode_rewritten(buf, o, n_docs, return_text, lambda ids, cap, toff, norm, norm_cap: self._lib.td_encode_batch_nfc(
            self._h, buf.ctypes.data if len(buf) else None, o.ctypes.data, n_docs, mode, ids, cap, toff, norm, norm_cap, noff.ctypes.data,
            changed.ctypes.data, counts.ctypes.data))
        self._check(rc)
        return ids[:int(toff[-1])], toff, (norm[:int(counts[0])] if return_text else None), noff, changed[:n_docs], counts

    # ---- UTF-8 validation and repair ----------------------------------------------------------------------------
    def utf8_check(self, d_text: int, n_bytes: int, d_doc_offsets: int, n_docs: int, d_flags: int, d_first_bad: int, d_counts: int, stream: int):
        """td_utf8_check_device: raw device pointers (d_first_bad may be 0), asynchronous on `stream`, which must not be the null stream;
        d_flags uint8[n_docs] (0: well-formed), d_first_bad int64[n_docs], d_counts int64[8]; check with device_status(stream)."""
        self._check(self._lib.td_utf8_check_device(self._h, d_text or None, n_bytes, d_doc_offsets or None, n_docs, d_flags or None,
                                                   d_first_bad or None, d_counts or None, stream or None))

    def utf8_device(self, d_text: int, n_bytes: int, d_doc_offsets: int, n_docs: int, policy: int, d_out: int, out_capacity: int,
                    d_out_doc_offsets: int, d_flags: int, d_first_bad: int, d_n_bad: int, d_counts: int, stream: int):
        """td_utf8_device: raw device pointers (d_flags, d_first_bad, d_n_bad may be 0), asynchronous on `stream`; check with
        device_status(stream)."""
        self._check(self._lib.td_utf8_device(self._h, d_text or None, n_bytes, d_doc_offsets or None, n_docs, policy, d_out or None, out_capacity,
                                             d_out_doc_offsets or None, d_flags or None, d_first_bad or None, d_n_bad or None, d_counts or None,
                                             stream or None))

    def utf8(self, text, doc_offsets, policy: int = TD_UTF8_REPLACE, capacity: int | None = None, want_text: bool = True,
             check_only: bool = False):
        """td_utf8: utf8_host's arguments and results, computed on the device.  check_only: no output, no offsets and no n_bad are asked
        for, which makes the call the check (one pass at read speed) -> (None, None, flags, first_bad, None, counts with [1] alone)."""
        buf, o, n_docs, ooff, flags, first, nbad, counts = _rewrite_args(text, doc_offsets, _UTF8_PER_DOC)
        want_text = want_text and not check_only
        cap = _rewrite_capacity(buf, o, capacity, 1 if policy == TD_UTF8_IGNORE else 3) if want_text else 0
        out = np.empty(max(cap, 1), dtype=np.uint8)
        rc = self._lib.td_utf8(self._h, buf.ctypes.data if len(buf) else None, o.ctypes.data, n_docs, policy, out.ctypes.data if want_text else None,
                               cap, None if check_only else ooff.ctypes.data, flags.ctypes.data, first.ctypes.data,
                               None if check_only else nbad.ctypes.data, counts.ctypes.data)
        if rc != TD_OK:
            _raise_with_counts(rc, self._lib.td_last_error(self._h).decode("utf-8", "replace"), counts)
        if check_only:
            return None, None, flags[:n_docs], first[:n_docs], None, counts
        return (out[:int(counts[0])] if want_text else None), ooff, flags[:n_docs], first[:n_docs], nbad[:n_docs], counts

    def encode_batch_utf8(self, text, doc_offsets, mode: int = TD_MODE_ENCODE, policy: int = TD_UTF8_REPLACE, return_text: bool = False):
        """td_encode_batch_utf8: check, repair where a document is flagged, encode -> (ids int32, tok_offsets int64[n_docs + 1],
        fixed_text uint8 | None, fixed_doc_offsets int64[n_docs + 1], flags uint8[n_docs], first_bad int64[n_docs], n_bad int64[n_docs],
        counts int64[8]).  Offsets refer to the repaired text."""
        buf, o, n_docs, foff, flags, first, nbad, counts = _rewrite_args(text, doc_offsets, _UTF8_PER_DOC)
        rc, ids, toff, fixed = _encode_rewritten(buf, o, n_docs, return_text, lambda ids, cap, toff, fixed, fixed_cap: self._lib.td_encode_batch_utf8(
            self._h, buf.ctypes.data if len(buf) else None, o.ctypes.data, n_docs, mode, policy, ids, cap, toff, fixed, fixed_cap, foff.ctypes.data,
            flags.ctypes.data, first.ctypes.data, nbad.ctypes.data, counts.ctypes.data))
        self._check(rc)
        return (ids[:int(toff[-1])], toff, (fixed[:int(counts[0])] if return_text else None), foff, flags[:n_docs], first[:n_docs],
                nbad[:n_docs], counts)

    # ---- per-document text statistics -----------------------------------------------------------------------------
    def text_stats_device(self, d_text: int, n_bytes: int, d_doc_offsets: int, n_docs: int, groups: int, d_stats: int, d_totals: int, stream: int):
        """td_text_stats_device: raw device pointers (d_totals may be 0), asynchronous on `stream`, which must not be the null stream;
        d_stats int64[n_docs, 21], d_totals int64[21]; check with device_status(stream)."""
        self._check(self._lib.td_text_stats_device(self._h, d_text or None, n_bytes, d_doc_offsets or None, n_docs, groups, d_stats or None,
                                                   d_totals or None, stream or None))

    def text_stats(self, text, doc_offsets, groups: int = TD_TS_ALL):
        """td_text_stats: text_stats_host's arguments and results, computed on the device."""
        buf, o, n_docs, stats, totals = _text_stats_args(text, doc_offsets)
        self._check(self._lib.td_text_stats(self._h, buf.ctypes.data if len(buf) else None, o.ctypes.data, n_docs, groups, stats.ctypes.data,
                                            totals.ctypes.data))
        return stats[:n_docs], totals

    def encode_batch_text_stats(self, text, doc_offsets, mode: int = TD_MODE_ENCODE, groups: int = TD_TS_ALL):
        """td_encode_batch_text_stats: one upload, the statistics and the encode -> (ids int32, tok_offsets int64[n_docs + 1],
        stats int64[n_docs, 21], totals int64[21])."""
        buf, o, n_docs, stats, totals = _text_stats_args(text, doc_offsets)
        n = int(o[-1]) if len(o) and 0 <= int(o[-1]) <= len(buf) else 0
        toff = np.zeros(n_docs + 1, dtype=np.int64)
        ids = np.empty(n + 64, dtype=np.int32)
        self._check(self._lib.td_encode_batch_text_stats(self._h, buf.ctypes.data if len(buf) else None, o.ctypes.data, n_docs, mode, groups,
                                                         ids.ctypes.data, len(ids), toff.ctypes.data, stats.ctypes.data, totals.ctypes.data))
        return ids[:int(toff[-1])], toff, stats[:n_docs], totals

    # ---- decode rows (td_decode_spec) ---------------------------------------------------------------------------
    def decode_rows(self, ids, spec: DecodeSpec, tok_offsets=None, lengths=None, n_segs: int | None = None, capacity: int | None = None):
        """td_decode_rows -> (bytes, out_offsets int64[n_segs + 1], seg_ids int64[n_segs], info int64[4] = bytes, ids emitted, ids
        skipped, segments stopped).  ids: flat, or [rows, row_stride] in the rows form.  capacity None: sized by the call itself
        (a second call when the first guess was short); given and too small: TokenDaggerHipError(TD_E_CAPACITY) that carries
        .n_bytes, .out_offsets, .seg_ids and .info."""
        t, o, ln, n = _decode_rows_args(ids, tok_offsets, lengths, n_segs, spec)
        offs, seg, info = np.zeros(n + 1, dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64), np.zeros(4, dtype=np.int64)
        cap = max(64, 8 * len(t)) if capacity is None else capacity
        nb = ctypes.c_int64(0)
        for _ in range(2):
            out = np.empty(max(cap, 1), dtype=np.uint8)
            rc = self._lib.td_decode_rows(self._h, t.ctypes.data if len(t) else None, len(t), o.ctypes.data if o is not None else None,
                                          ln.ctypes.data if ln is not None else None, n, ctypes.byref(spec), out.ctypes.data if cap else None,
                                          cap, offs.ctypes.data, seg.ctypes.data, info.ctypes.data, ctypes.byref(nb))
            if rc == TD_E_CAPACITY and capacity is None and nb.value > cap:
                cap = nb.value
                continue
            break
        if rc == TD_E_CAPACITY:
            ex = TokenDaggerHipError(rc, self._lib.td_last_error(self._h).decode("utf-8", "replace"))
            ex.n_bytes, ex.out_offsets, ex.seg_ids, ex.info = int(nb.value), offs, seg[:n], info
            raise ex
        self._check(rc)
        return out[:nb.value].tobytes(), offs, seg[:n], info

    def decode_rows_device(self, d_ids: int, n_tokens: int, d_tok_offsets: int, d_seg_len: int, n_segs: int, spec: DecodeSpec, d_out: int,
                           out_capacity: int, d_out_offsets: int, d_seg_ids: int, d_info: int, stream: int = 0):
        """td_decode_rows_device: raw device pointers (0 for the ones the form does not use), asynchronous on `stream`; check with
        device_status(stream)."""
        self._check(self._lib.td_decode_rows_device(self._h, d_ids or None, n_tokens, d_tok_offsets or None, d_seg_len or None, n_segs,
                                                    ctypes.byref(spec), d_out or None, out_capacity, d_out_offsets or None, d_seg_ids or None,
                                                    d_info or None, stream or None))

    def device_status_pos(self, stream: int = 0) -> tuple[int, int]:
        """td_device_status without raising: (code, err_pos)."""
        pos = ctypes.c_int64(0)
        rc = self._lib.td_device_status(self._h, stream or None, ctypes.byref(pos))
        return int(rc), int(pos.value)

    def token_starts_device(self, d_tokens: int, n_tokens: int, d_tok_offsets: int, n_docs: int, d_out_starts: int, unit: int = TD_UNIT_BYTES,
                            stream: int = 0):
        """Asynchronous on `stream`; check with device_status(stream)."""
        self._check(self._lib.td_token_starts_device(self._h, d_tokens, n_tokens, d_tok_offsets, n_docs, unit, d_out_starts, stream or None))

    def encode_batch_with_starts(self, text, doc_offsets, mode: int = TD_MODE_ENCODE, allowed=(), unit: int = TD_UNIT_BYTES,
                                 capacity: int | None = None):
        """td_encode_batch_with_starts: -> (tokens int32[total], offsets int64[n_docs+1], starts int64[total]).
        allowed: special-token strings that are cut out."""
        buf = _as_u8(text)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        ab, ao = self._pack_strs(list(allowed))
        n_docs = len(offs) - 1
        n = int(offs[-1]) if len(offs) else 0
        cap = capacity if capacity is not None else n + 16
        out_offs = np.empty(n_docs + 1, dtype=np.int64)
        toks = np.empty(max(cap, 1), dtype=np.int32)
        starts = np.empty(max(cap, 1), dtype=np.int64)
        ntok = ctypes.c_int64(0)
        rc = self._lib.td_encode_batch_with_starts(self._h, buf.ctypes.data if n else None, offs.ctypes.data, n_docs, mode, ab.ctypes.data,
                                                   ao.ctypes.data, len(ao) - 1, unit, toks.ctypes.data, cap, out_offs.ctypes.data,
                                                   starts.ctypes.data, ctypes.byref(ntok))
        self._check(rc)
        return toks[:ntok.value].copy(), out_offs, starts[:ntok.value].copy()

    def encode_device_with_starts(self, d_text: int, n_bytes: int, d_doc_offsets: int, n_docs: int, d_out_tokens: int, out_capacity: int,
                                  d_out_offsets: int, d_out_starts: int, unit: int = TD_UNIT_BYTES, stream: int = 0,
                                  mode: int = TD_MODE_ENCODE):
        """td_encode_device + the starts (int64, room for out_capacity), asynchronous on `stream`."""
        self._check(self._lib.td_encode_device_with_starts(self._h, d_text, n_bytes, d_doc_offsets, n_docs, mode, unit, d_out_tokens,
                                                           out_capacity, d_out_offsets, d_out_starts, stream or None))

    def decode_bytes(self, tokens) -> bytes:
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        nb = ctypes.c_int64(0)
        cap = max(64, 8 * len(t))
        for _ in range(2):
            out = np.empty(cap, dtype=np.uint8)
            rc = self._lib.td_decode_bytes(self._h, t.ctypes.data if len(t) else None, len(t), out.ctypes.data, cap,
                                           ctypes.byref(nb))
            if rc == TD_E_CAPACITY and nb.value > cap:
                cap = nb.value
                continue
            break
        self._check(rc)
        return out[:nb.value].tobytes()

    # ---- device-buffer API (pointers are raw device addresses, e.g. torch_tensor.data_ptr()) --
    def encode_batch_with_special(self, text, doc_offsets, allowed_ids):
        """encode_batch with allowed special tokens (ids): -> (tokens int32[total], offsets int64[n_docs+1])"""
        buf = _as_u8(text)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.int64)
        ids = np.ascontiguousarray(sorted(allowed_ids), dtype=np.int32)
        n_docs = len(offs) - 1
        n = int(offs[-1]) if len(offs) else 0
        cap = max(16, n // 3 + 16)
        out_offs = np.empty(n_docs + 1, dtype=np.int64)
        ntok = ctypes.c_int64(0)
        for _ in range(2):
            toks = np.empty(cap, dtype=np.int32)
            rc = self._lib.td_encode_batch_with_special(self._h, buf.ctypes.data if n else None, offs.ctypes.data, n_docs,
                                                        ids.ctypes.data if len(ids) else None, len(ids), toks.ctypes.data, cap,
                                                        out_offs.ctypes.data, ctypes.byref(ntok))
            if rc == TD_E_CAPACITY and ntok.value > cap:
                cap = ntok.value
                continue
            break
        self._check(rc)
        return toks[:ntok.value], out_offs

    def decode_batch(self, tokens, tok_offsets) -> tuple[bytes, np.ndarray]:
        """ids of all documents concatenated + int64 offsets -> (all bytes concatenated, int64 byte offsets)."""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        o = np.ascontiguousarray(tok_offsets, dtype=np.int64)
        n_docs = len(o) - 1
        out_offs = np.empty(n_docs + 1, dtype=np.int64)
        cap = max(64, 8 * len(t))
        nb = ctypes.c_int64(0)
        for _ in range(2):
            out = np.empty(cap, dtype=np.uint8)
            rc = self._lib.td_decode_batch(self._h, t.ctypes.data if len(t) else None, o.ctypes.data, n_docs, out.ctypes.data, cap,
                                           out_offs.ctypes.data, ctypes.byref(nb))
            if rc == TD_E_CAPACITY and nb.value > cap:
                cap = nb.value
                continue
            break
        self._check(rc)
        return out[:nb.value].tobytes(), out_offs

    def decode_device(self, d_tokens: int, n_tokens: int, d_out: int, out_capacity: int, d_n_bytes: int = 0, stream: int = 0):
        """Device pointers in, asynchronous on `stream`; check with device_status(stream)."""
        self._check(self._lib.td_decode_device(self._h, d_tokens, n_tokens, d_out, out_capacity, d_n_bytes or None, stream or None))

    def reserve(self, max_bytes: int, max_docs: int):
        self._check(self._lib.td_reserve(self._h, max_bytes, max_docs))

    def encode_device(self, d_text: int, n_bytes: int, d_doc_offsets: int, n_docs: int, d_out_tokens: int,
                      out_capacity: int, d_out_offsets: int, stream: int = 0, mode: int = TD_MODE_ENCODE):
        """Asynchronous on `stream`; d_out_offsets[n_docs] receives the total token count."""
        self._check(self._lib.td_encode_device(self._h, d_text, n_bytes, d_doc_offsets, n_docs, mode, d_out_tokens,
                                               out_capacity, d_out_offsets, stream))

    def encode_device_with_special(self, d_text: int, n_bytes: int, d_doc_offsets: int, n_docs: int, allowed_ids, d_out_tokens: int,
                                   out_capacity: int, d_out_offsets: int, stream: int = 0):
        """td_encode_device_with_special: allowed special tokens (ids) are searched for and cut out ON THE DEVICE."""
        ids = np.ascontiguousarray(np.asarray(sorted(set(int(i) for i in allowed_ids)), dtype=np.int32))
        self._check(self._lib.td_encode_device_with_special(self._h, ctypes.c_void_p(d_text), n_bytes, ctypes.c_void_p(d_doc_offsets), n_docs,
                                                            ids.ctypes.data_as(ctypes.c_void_p), len(ids), ctypes.c_void_p(d_out_tokens),
                                                            out_capacity, ctypes.c_void_p(d_out_offsets), ctypes.c_void_p(stream)))

    def device_status(self, stream: int = 0):
        pos = ctypes.c_int64(0)
        self._check(self._lib.td_device_status(self._h, stream, ctypes.byref(pos)))

    # ---- misc -------------------------------------------------------------------------------
    def info(self, what: int) -> int:
        return int(self._lib.td_info(self._h, what))

    def set_option(self, what: int, value: int):
        self._check(self._lib.td_set_option(self._h, what, value))

    def profile_read(self) -> tuple[float, float, int]:
        """-> (sum of td_split_tiles ms, sum of td_encode_tiles ms, calls) since the last read (TD_OPT_PROFILE=1)."""
        a = ctypes.c_double(0); b = ctypes.c_double(0); n = ctypes.c_int64(0)
        self._check(self._lib.td_profile_read(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)))
        return a.value, b.value, n.value

    def profile_read_all(self) -> tuple[dict[str, float], int]:
        """-> ({kernel segment: summed ms}, calls) since the last read (TD_OPT_PROFILE=1)."""
        names = []
        while True:
            nm = self._lib.td_profile_segment_name(len(names)).decode()
            if not nm:
                break
            names.append(nm)
        arr = (ctypes.c_double * len(names))()
        n = ctypes.c_int64(0)
        self._check(self._lib.td_profile_read_ex(self._h, arr, len(names), ctypes.byref(n)))
        return {nm: arr[i] for i, nm in enumerate(names)}, n.value

    def special_tokens(self) -> dict[str, int]:
        out = {}
        for i in range(self._lib.td_special_count(self._h)):
            s = ctypes.c_char_p(); n = ctypes.c_int64(0); tid = ctypes.c_int32(0)
            self._lib.td_special_get(self._h, i, ctypes.byref(s), ctypes.byref(n), ctypes.byref(tid))
            out[ctypes.string_at(s, n.value).decode("utf-8")] = tid.value
        return out


# ---------------------------------------------------------------------------------------------- multi-GPU epilogue
TD_COMM_ID_BYTES = 128


def comm_bases(table, rank: int) -> tuple[int, int, int, int]:
    """td_comm_bases: gathered {tokens, documents} per rank (host array of 2 * world int64) -> (token_base, doc_base,
    token_total, doc_total) of `rank`.  Host only: no device, no RCCL."""
    lib = load_library()
    t = np.ascontiguousarray(np.asarray(table, dtype=np.int64).reshape(-1))
    world = len(t) // 2
    tb, db, tt, dt = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    rc = lib.td_comm_bases(t.ctypes.data_as(ctypes.c_void_p), world, rank, ctypes.byref(tb), ctypes.byref(db), ctypes.byref(tt), ctypes.byref(dt))
    if rc != 0:
        raise TokenDaggerHipError(rc, (lib.td_comm_last_error() or b"").decode("utf-8", "replace"))
    return tb.value, db.value, tt.value, dt.value


def comm_unique_id() -> bytes:
    """td_comm_unique_id (rank 0): the 128 bytes every rank hands to RcclComm."""
    lib = load_library()
    buf = (ctypes.c_uint8 * TD_COMM_ID_BYTES)()
    rc = lib.td_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p))
    if rc != 0:
        raise TokenDaggerHipError(rc, (lib.td_comm_last_error() or b"").decode("utf-8", "replace"))
    return bytes(buf)


class RcclComm:
    """The path's only exchange behind the C ABI (td_comm_*): RCCL all-gather of {tokens, documents}, optional gather of the
    ids to one rank.  Pointers are raw device addresses (e.g. torch.Tensor.data_ptr())."""

    def __init__(self, unique_id: bytes, world: int, rank: int, device: int = -1):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        self.world, self.rank = world, rank
        idb = (ctypes.c_uint8 * TD_COMM_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self._lib.td_comm_create(ctypes.cast(idb, ctypes.c_void_p), world, rank, device, ctypes.byref(self._h)))

    def _check(self, rc: int):
        if rc != 0:
            raise TokenDaggerHipError(rc, (self._lib.td_comm_last_error() or b"").decode("utf-8", "replace"))

    def gather_counts(self, d_counts: int, d_table: int, stream: int = 0):
        self._check(self._lib.td_comm_gather_counts(self._h, ctypes.c_void_p(d_counts), ctypes.c_void_p(d_table), ctypes.c_void_p(stream)))

    def gather_tokens(self, d_tokens: int, table, root: int, d_root_tokens: int, root_capacity: int, stream: int = 0):
        t = np.ascontiguousarray(np.asarray(table, dtype=np.int64).reshape(-1))
        self._check(self._lib.td_comm_gather_tokens(self._h, ctypes.c_void_p(d_tokens), t.ctypes.data_as(ctypes.c_void_p), root,
                                                    ctypes.c_void_p(d_root_tokens), root_capacity, ctypes.c_void_p(stream)))

    def close(self):
        if self._h:
            self._lib.td_comm_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
