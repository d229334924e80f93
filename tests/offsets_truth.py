"""Brute-force truth for per-token start offsets (td_token_starts / td_encode_*_with_starts), host only.

A token's start is where its bytes begin in its document.  The truth is built the slow, obvious way: the pattern's pieces
(H.rx_split for generic patterns), the tokens placed inside the text they cover by cumulative byte length, and characters
counted by tiktoken's decode_with_offsets rule: chars(b) = bytes of doc[0:b] that are not continuation bytes,
start_char = max(0, chars(b) - (doc[b] is a continuation byte))."""
from __future__ import annotations

import numpy as np


def id_bytes(mergeable_ranks: dict, special: dict) -> list:
    """id -> token bytes (None where no token has the id)."""
    top = max(max(mergeable_ranks.values()), max(special.values()) if special else 0)
    out = [None] * (top + 1)
    for b, r in mergeable_ranks.items():
        out[r] = b
    for s, r in special.items():
        out[r] = s.encode("utf-8")
    return out


def id_lengths(table: list) -> np.ndarray:
    return np.asarray([len(b) if b is not None else 0 for b in table], dtype=np.int64)


def covered_byte_starts(ids, tok_offsets, lengths: np.ndarray) -> np.ndarray:
    """Per-document exclusive prefix sum of token byte lengths (patterns that cover every byte)."""
    ids = np.asarray(ids, dtype=np.int64)
    ln = lengths[ids] if len(ids) else np.zeros(0, np.int64)
    cs = np.concatenate([[0], np.cumsum(ln)])
    to = np.asarray(tok_offsets, dtype=np.int64)
    doc = np.repeat(np.arange(len(to) - 1), np.diff(to))
    return cs[:-1] - cs[to[doc]]


def is_cont(data: np.ndarray) -> np.ndarray:
    return (data & 0xC0) == 0x80


def char_starts(text, doc_offsets, tok_offsets, byte_starts) -> np.ndarray:
    """Byte starts (document-relative) -> tiktoken's character starts, by counting on the text."""
    t = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    nc = np.concatenate([[0], np.cumsum(~is_cont(t))]).astype(np.int64)
    do = np.asarray(doc_offsets, dtype=np.int64)
    to = np.asarray(tok_offsets, dtype=np.int64)
    doc = np.repeat(np.arange(len(to) - 1), np.diff(to))
    p = do[doc] + np.asarray(byte_starts, dtype=np.int64)
    c = nc[p] - nc[do[doc]] - is_cont(t[p]).astype(np.int64)
    return np.maximum(c, 0)


def decode_offsets_rule(token_bytes: list) -> list:
    """tiktoken's Encoding.decode_with_offsets on the concatenated token bytes."""
    text_len, offsets = 0, []
    for tb in token_bytes:
        offsets.append(max(0, text_len - (0x80 <= tb[0] < 0xC0)))
        text_len += sum(1 for c in tb if not 0x80 <= c < 0xC0)
    return offsets


def split_arrays(pattern: str, data: bytes):
    """The pieces of one document as (starts, ends) int64 arrays (H.rx_split without a Python tuple per piece)."""
    import ctypes
    import helpers as H
    H.build_twin()
    lib = ctypes.CDLL(str(H.TWIN_SO))
    lib.twin_rx_split.restype = ctypes.c_int64
    lib.twin_rx_split.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_int64, ctypes.c_char_p, ctypes.c_int]
    cap = len(data) + 1
    st = np.empty(cap, dtype=np.int64)
    en = np.empty(cap, dtype=np.int64)
    err = ctypes.create_string_buffer(512)
    n = lib.twin_rx_split(pattern.encode("utf-8"), data, len(data), st.ctypes.data, en.ctypes.data, cap, err, 512)
    assert n >= 0, err.value
    return st[:n], en[:n]


def generic_byte_starts(starts, ends, ids, lengths: np.ndarray, n_doc: int) -> np.ndarray:
    """One document of a pattern that may skip text: [starts, ends) = what the pattern matched; the tokens' bytes are the
    pieces' bytes in order, so token k starts at the covered byte its compacted position names."""
    d = np.zeros(n_doc + 1, dtype=np.int64)
    np.add.at(d, np.asarray(starts, dtype=np.int64), 1)
    np.add.at(d, np.asarray(ends, dtype=np.int64), -1)
    covered = np.flatnonzero(np.cumsum(d)[:n_doc] > 0)
    ln = lengths[np.asarray(ids, dtype=np.int64)] if len(ids) else np.zeros(0, np.int64)
    compact = np.concatenate([[0], np.cumsum(ln)])[:-1]
    assert compact.size == 0 or int(compact[-1] + ln[-1]) == covered.size
    return covered[compact]
