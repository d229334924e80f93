"""Truth for training rows (td_make_rows, include/tokendagger_hip.h): straight from the definitions.

rows_brute   Python loops: the flat stream of [BOS] ids [EOS] slots, then rows, positions and cu_seqlens (concat) or one row per
             document (pad).
rows_numpy   the same, vectorised, for large inputs.
Both return (ids [rows, S], positions [rows, S], aux, counts[4]) with aux = cu_seqlens (concat) or lengths (pad).
"""
from __future__ import annotations

import numpy as np

CONCAT, PAD = 0, 1


def rows_brute(ids, tok_offsets, S, layout=CONCAT, bos=-1, eos=-1, pad=0, drop_last=False):
    ids = [int(x) for x in ids]
    offs = [int(x) for x in tok_offsets]
    n_docs = len(offs) - 1
    b, e = bos >= 0, eos >= 0
    if layout == PAD:
        room = S - b - e
        out, pos, lens, trunc = [], [], [], 0
        for d in range(n_docs):
            body = ids[offs[d]:offs[d + 1]]
            trunc += len(body) > room
            row = ([bos] if b else []) + body[:room] + ([eos] if e else [])
            lens.append(len(row))
            pos += list(range(len(row))) + [0] * (S - len(row))
            out += row + [pad] * (S - len(row))
        real = sum(lens)
        return (np.array(out, np.int32).reshape(n_docs, S), np.array(pos, np.int32).reshape(n_docs, S), np.array(lens, np.int32),
                np.array([n_docs, real, sum(x > 0 for x in lens), trunc], np.int64))
    stream, starts = [], []
    for d in range(n_docs):
        starts.append(len(stream))
        stream += ([bos] if b else []) + ids[offs[d]:offs[d + 1]] + ([eos] if e else [])
    T = len(stream)
    rows = T // S if drop_last else -(-T // S)
    R = min(T, rows * S)
    cuts = set(range(0, R, S))
    for d in range(n_docs):
        n_d = b + (offs[d + 1] - offs[d]) + e
        if n_d > 0 and starts[d] < R:
            cuts.add(starts[d])
    cu = sorted(cuts) + [R]
    out = stream[:R] + [pad] * (rows * S - R)
    pos = [0] * (rows * S)
    seg = 0
    for j in range(R):
        if j in cuts:
            seg = j
        pos[j] = j - seg
    return (np.array(out, np.int32).reshape(rows, S), np.array(pos, np.int32).reshape(rows, S), np.array(cu, np.int32),
            np.array([rows, R, len(cu) - 1, 0], np.int64))


def doc_base(tok_offsets, b, e):
    """base_d = tok_offsets[d] + d * (b + e): where document d starts in the stream (closed form; entry n_docs = T)."""
    o = np.asarray(tok_offsets, np.int64)
    return o + np.arange(len(o), dtype=np.int64) * (int(b) + int(e))


def doc_cuts(tok_offsets, S, b, e, R):
    """c_d: the document's start (if it has slots and starts below R) + the row starts strictly inside it, below R."""
    base = doc_base(tok_offsets, b, e)
    n = np.diff(np.asarray(tok_offsets, np.int64)) + int(b) + int(e)
    bs = base[:-1]
    end = np.minimum(bs + n, R)
    live = (n > 0) & (bs < R)
    c = np.where(live, 1 + (end - 1) // S - bs // S, 0)
    return c.astype(np.int64)


def rows_numpy(ids, tok_offsets, S, layout=CONCAT, bos=-1, eos=-1, pad=0, drop_last=False):
    ids = np.asarray(ids, np.int32)
    offs = np.asarray(tok_offsets, np.int64)
    n_docs = len(offs) - 1
    b, e = int(bos >= 0), int(eos >= 0)
    L = np.diff(offs)
    if layout == PAD:
        room = S - b - e
        body = np.minimum(L, room)
        lens = b + body + e
        o = np.arange(S, dtype=np.int64)[None, :]
        src = offs[:-1, None] + o - b
        is_body = (o >= b) & (o < b + body[:, None])
        out = np.where(is_body, ids[np.clip(src, 0, max(len(ids) - 1, 0))] if len(ids) else 0, pad)
        if b:
            out[:, 0] = bos
        if e:
            out[np.arange(n_docs), b + body] = eos
        pos = np.where(o < lens[:, None], o, 0)
        return (out.astype(np.int32).reshape(n_docs, S), pos.astype(np.int32).reshape(n_docs, S), lens.astype(np.int32),
                np.array([n_docs, int(lens.sum()), int((lens > 0).sum()), int((L > room).sum())], np.int64))
    base = doc_base(offs, b, e)
    T = int(base[-1])
    rows = T // S if drop_last else -(-T // S)
    R = min(T, rows * S)
    n = L + b + e
    doc = np.repeat(np.arange(n_docs, dtype=np.int64), n)  # the document of every stream slot
    j = np.arange(T, dtype=np.int64)
    o = j - base[:-1][doc] if T else j
    stream = np.zeros(T, np.int32)
    if T:
        src = j - doc * (b + e) - b
        body = (o >= b) & (o < b + L[doc])
        stream[body] = ids[src[body]]
        if b:
            stream[o == 0] = bos
        if e:
            stream[o == n[doc] - 1] = eos
    out = np.full(rows * S, pad, np.int32)
    out[:R] = stream[:R]
    seg = np.maximum(base[:-1][doc][:R], (j[:R] // S) * S) if T else np.zeros(0, np.int64)
    pos = np.zeros(rows * S, np.int32)
    pos[:R] = (j[:R] - seg).astype(np.int32)
    starts = base[:-1][(n > 0) & (base[:-1] < R)]
    cu = np.union1d(np.arange(0, R, S, dtype=np.int64), starts)
    cu = np.concatenate([cu, [R]]).astype(np.int32)
    return out.reshape(rows, S), pos.reshape(rows, S), cu, np.array([rows, R, len(cu) - 1, 0], np.int64)
