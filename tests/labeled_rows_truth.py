"""Truth for label rows (td_*_rows_labeled, include/tokendagger_hip.h): a second stream `src`, index-aligned with the ids, placed
by the placement of the id rows.

label_rows        through an INDEX STREAM: the layout's existing truth (rows_truth, pack_truth, windows_truth, unmodified) runs on
                  ids' = arange(n) + 3 with bos = 0, eos = 1, pad = 2; its rows say for every slot whether it is the BOS, the EOS,
                  a pad slot or body id k - 3, and those map to bos_value / eos_value / pad_value / src[k - 3].  The overlap mask
                  comes from row_starts and overlap.
label_rows_brute  slot by slot in Python loops, from the contract's words; BESTFIT takes the segments (cu_seqlens, seg_docs) of the
                  id rows and walks every document's [BOS] body [EOS] through its segments.
Both return int32 [rows, S].
"""
from __future__ import annotations

import numpy as np

import pack_truth as pt
import rows_truth as rt
import windows_truth as wt

LAYOUTS = ("concat", "pad", "bestfit", "windows")
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def id_rows(layout, ids, tok_offsets, S, bos=-1, eos=-1, pad=0, overlap=0, drop_last=False, truncate=False):
    """The layout's existing truth, as its own tuple."""
    ids = np.asarray(ids, np.int32)
    offs = np.asarray(tok_offsets, np.int64)
    if layout == "concat":
        return rt.rows_numpy(ids, offs, S, rt.CONCAT, bos, eos, pad, drop_last)
    if layout == "pad":
        return rt.rows_numpy(ids, offs, S, rt.PAD, bos, eos, pad)
    if layout == "bestfit":
        return pt.pack_runs(ids, offs, S, bos, eos, pad, truncate)
    if layout == "windows":
        return wt.windows_numpy(ids, offs, S, overlap, bos, eos, pad)
    raise ValueError(layout)


def label_rows(layout, src, tok_offsets, S, *, bos=False, eos=False, bos_value=-100, eos_value=-100, pad_value=-100, overlap=0,
               mask_overlap=False, drop_last=False, truncate=False):
    src = np.asarray(src, np.int32)
    offs = np.asarray(tok_offsets, np.int64)
    n = int(offs[-1])
    index = np.arange(n, dtype=np.int32) + 3
    r = id_rows(layout, index, offs, S, 0 if bos else -1, 1 if eos else -1, 2, overlap, drop_last, truncate)
    k = r[0].astype(np.int64)
    body = np.concatenate([src[:n], np.zeros(1, np.int32)])  # (one more: the gather of the non-body slots stays inside)
    out = np.where(k == 0, bos_value, np.where(k == 1, eos_value, np.where(k == 2, pad_value, body[np.clip(k - 3, 0, n)])))
    out = out.astype(np.int64)
    if mask_overlap:
        if layout != "windows":
            raise ValueError("mask_overlap is for windows")
        starts = np.asarray(r[4], np.int64)
        b = int(bool(bos))
        cols = np.arange(S)[None, :]
        rep = (starts[:, None] > 0) & (cols >= b) & (cols < b + overlap) & (k >= 3)
        out = np.where(rep, pad_value, out)
    assert out.min(initial=0) >= I32_MIN and out.max(initial=0) <= I32_MAX
    return out.astype(np.int32).reshape(-1, S)


def label_rows_brute(layout, src, tok_offsets, S, *, bos=False, eos=False, bos_value=-100, eos_value=-100, pad_value=-100, overlap=0,
                     mask_overlap=False, drop_last=False, truncate=False):
    src = [int(x) for x in np.asarray(src)]
    offs = [int(x) for x in tok_offsets]
    n_docs = len(offs) - 1
    b, e = int(bool(bos)), int(bool(eos))
    room = S - b - e

    def framed(d, lo=None, hi=None):
        lo = offs[d] if lo is None else lo
        hi = offs[d + 1] if hi is None else hi
        return ([bos_value] if b else []) + src[lo:hi] + ([eos_value] if e else [])

    if layout == "concat":
        stream = []
        for d in range(n_docs):
            stream += framed(d)
        rows = len(stream) // S if drop_last else -(-len(stream) // S)
        flat = (stream + [pad_value] * S)[:rows * S]
    elif layout == "pad":
        flat = []
        for d in range(n_docs):
            row = framed(d, offs[d], min(offs[d + 1], offs[d] + room))
            flat += row + [pad_value] * (S - len(row))
        rows = n_docs
    elif layout == "windows":
        step = room - overlap
        flat, rows = [], 0
        for d in range(n_docs):
            L = offs[d + 1] - offs[d]
            w = 1 if L <= room else -(-(L - overlap) // step)
            for k in range(w):
                lo = offs[d] + k * step
                row = framed(d, lo, min(offs[d + 1], lo + room))
                if mask_overlap and k > 0:
                    for j in range(overlap):
                        row[b + j] = pad_value
                flat += row + [pad_value] * (S - len(row))
                rows += 1
    elif layout == "bestfit":
        index = np.arange(offs[-1], dtype=np.int32)
        r = pt.pack_runs(index, np.asarray(offs, np.int64), S, 0 if b else -1, 0 if e else -1, 0, truncate)
        cu, seg_docs, rows = [int(x) for x in r[2]], [int(x) for x in r[4]], int(r[5][0])
        flat = [pad_value] * (rows * S)
        segs_of = {}
        for k, d in enumerate(seg_docs):
            if d >= 0:
                segs_of.setdefault(d, []).append(k)
        for d in range(n_docs):
            seq = framed(d, offs[d], min(offs[d + 1], offs[d] + room) if truncate else offs[d + 1])
            at = 0
            for k in sorted(segs_of.get(d, []), key=lambda k: cu[k]):  # (full chunks lie in the rows in front of every remainder)
                ln = cu[k + 1] - cu[k]
                flat[cu[k]:cu[k] + ln] = seq[at:at + ln]
                at += ln
            assert at == len(seq), (d, at, len(seq))
    else:
        raise ValueError(layout)
    return np.array(flat, np.int64).astype(np.int32).reshape(rows, S)


def random_case(rng, layout, max_docs=10, max_len=40, max_S=24):
    """A small case for `layout`: (src ids tok_offsets S kwargs-of-label_rows)."""
    n_docs = int(rng.integers(0, max_docs + 1))
    lens = rng.integers(0, max_len + 1, n_docs)
    lens[rng.random(n_docs) < 0.25] = 0
    if rng.random() < 0.1:
        lens[:] = 0
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offs[-1])
    ids = rng.integers(0, 1000, n).astype(np.int32)
    src = rng.integers(I32_MIN, I32_MAX + 1, n).astype(np.int32)
    if n:
        src[rng.integers(0, n, 2)] = [I32_MIN, I32_MAX]
    bos, eos = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    lo = bos + eos + (1 if layout == "windows" else 0)
    S = int(rng.integers(max(lo, 1), max_S + 1))
    kw = dict(bos=bos, eos=eos, bos_value=int(rng.integers(I32_MIN, I32_MAX + 1)), eos_value=int(rng.integers(-5, 5)),
              pad_value=int(rng.choice([-100, I32_MIN, I32_MAX, 0])))
    if layout == "concat":
        kw["drop_last"] = bool(rng.integers(0, 2))
    if layout == "bestfit":
        kw["truncate"] = bool(rng.integers(0, 2))
    if layout == "windows":
        C = S - bos - eos
        kw["overlap"] = int(rng.integers(0, C))
        kw["mask_overlap"] = bool(rng.integers(0, 2))
    return src, ids, offs, S, kw
