"""Truth for overlapping window rows (TD_ROWS_WINDOWS, include/tokendagger_hip.h): straight from the definition.

windows_brute   Python loops over documents and windows: a window starts `step` ids after the one before and the walk ends with
                the window that reaches the document's end (how the Hugging Face description of stride reads).
windows_numpy   the closed form w_d = max(1, ceil((L_d - overlap) / step)), vectorised, for large inputs.
Both return (ids [rows, S], positions [rows, S], row_lengths [rows], row_docs [rows], row_starts [rows], counts[4]) with
counts = rows, real slots, documents with more than one window, the most windows of one document.
"""
from __future__ import annotations

import numpy as np


def windows_brute(ids, tok_offsets, S, overlap=0, bos=-1, eos=-1, pad=0):
    ids = [int(x) for x in ids]
    offs = [int(x) for x in tok_offsets]
    b, e = bos >= 0, eos >= 0
    C = S - b - e
    step = C - overlap
    assert C >= 1 and 0 <= overlap < C
    out, pos, lens, docs, starts = [], [], [], [], []
    multi = most = 0
    for d in range(len(offs) - 1):
        doc = ids[offs[d]:offs[d + 1]]
        at = w = 0
        while True:
            body = doc[at:at + C]
            row = ([bos] if b else []) + body + ([eos] if e else [])
            out += row + [pad] * (S - len(row))
            pos += list(range(len(row))) + [0] * (S - len(row))
            lens.append(len(row))
            docs.append(d)
            starts.append(at)
            w += 1
            if at + C >= len(doc):
                break
            at += step
        multi += w > 1
        most = max(most, w)
    rows = len(lens)
    return (np.array(out, np.int32).reshape(rows, S), np.array(pos, np.int32).reshape(rows, S), np.array(lens, np.int32),
            np.array(docs, np.int64), np.array(starts, np.int64), np.array([rows, sum(lens), multi, most], np.int64))


def window_counts(tok_offsets, S, overlap=0, bos=-1, eos=-1):
    """(w [n_docs], first_row [n_docs + 1]) by the closed form."""
    L = np.diff(np.asarray(tok_offsets, np.int64))
    C = S - int(bos >= 0) - int(eos >= 0)
    step = C - overlap
    w = np.maximum(1, -(-(L - overlap) // step))
    return w, np.concatenate([[0], np.cumsum(w)]).astype(np.int64)


def windows_numpy(ids, tok_offsets, S, overlap=0, bos=-1, eos=-1, pad=0, want_positions=True):
    ids = np.asarray(ids, np.int32)
    offs = np.asarray(tok_offsets, np.int64)
    n_docs = len(offs) - 1
    b, e = int(bos >= 0), int(eos >= 0)
    C = S - b - e
    step = C - overlap
    assert C >= 1 and 0 <= overlap < C
    L = np.diff(offs)
    w, first = window_counts(offs, S, overlap, bos, eos)
    rows = int(first[-1])
    docs = np.repeat(np.arange(n_docs, dtype=np.int64), w)
    starts = (np.arange(rows, dtype=np.int64) - first[:-1][docs]) * step
    body = np.clip(L[docs] - starts, 0, C)
    lens = b + body + e
    out = np.full((rows, S), pad, np.int32)
    pos = np.zeros((rows, S), np.int32) if want_positions else None
    base = offs[:-1][docs] + starts
    blk_rows = max(1, (1 << 22) // S)  # (in blocks of 4 Mi slots: the index arrays are eight times the rows)
    for r0 in range(0, rows, blk_rows):
        r1 = min(rows, r0 + blk_rows)
        o = np.arange(S, dtype=np.int64)[None, :]
        is_body = (o >= b) & (o < b + body[r0:r1, None])
        src = base[r0:r1, None] + o - b
        blk = out[r0:r1]
        if len(ids):
            blk[is_body] = ids[src[is_body]]
        if b:
            blk[:, 0] = bos
        if e:
            blk[np.arange(r1 - r0), b + body[r0:r1]] = eos
        if want_positions:
            pos[r0:r1] = np.where(o < lens[r0:r1, None], o, 0)
    counts = np.array([rows, int(lens.sum()), int((w > 1).sum()), int(w.max()) if n_docs else 0], np.int64)
    return out, pos, lens.astype(np.int32), docs, starts, counts
