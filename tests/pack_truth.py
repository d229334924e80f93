"""Truth for best-fit-decreasing rows (TD_ROWS_BESTFIT, td_pack_rows, include/tokendagger_hip.h): straight from the definitions.

pack_brute   item by item: every chunk in (length desc, document, chunk) order goes into the row with the smallest free count
             that is still >= its length (a linear scan over the rows), else a new row.
pack_runs    the run form: a row that takes one item of a run of equal lengths keeps taking them while it has room, so it takes
             min(k, free // len) at once; rows are found by free count through heaps.  Fast enough for millions of documents.
Both return (ids [rows, S], positions [rows, S], cu_seqlens, row_lengths, seg_docs, counts[4]); with placement=True also
(doc_row, doc_slot): where each document's packed chunk (its only chunk, or its remainder when split) sits, -1 for none.
"""
from __future__ import annotations

import bisect
import heapq

import numpy as np


def _docs(L, S, b, e, truncate):
    """n_d (slots after truncation), full chunks, remainder length and cut flag of every document."""
    L = np.asarray(L, np.int64)
    if truncate:
        body = np.minimum(L, S - b - e)
        n = b + body + e
        full = (n == S).astype(np.int64)
        rem = np.where(n == S, 0, n)
        cut = body < L
    else:
        n = b + L + e
        full = n // S
        rem = n % S
        cut = n > S
    return n, full, rem, cut


def plan_brute(L, S, b, e, truncate):
    """Rows as lists of segments (document, first slot inside the document, length)."""
    n, full, rem, _ = _docs(L, S, b, e, truncate)
    items = []
    for d in range(len(n)):
        chunks = [(S, c * S) for c in range(int(full[d]))]
        if rem[d]:
            chunks.append((int(rem[d]), int(full[d]) * S))
        for c, (ln, src) in enumerate(chunks):
            items.append((-ln, d, c, src))
    items.sort()
    rows = []  # [free, [(doc, src, len)]]
    for negl, d, _, src in items:
        ln = -negl
        best = -1
        for r, row in enumerate(rows):
            if row[0] >= ln and (best < 0 or row[0] < rows[best][0]):
                best = r
        if best < 0:
            rows.append([S, []])
            best = len(rows) - 1
        rows[best][0] -= ln
        rows[best][1].append((d, src, ln))
    return [row[1] for row in rows]


def plan_runs(L, S, b, e, truncate):
    """The same plan in run form: (segments as arrays start, doc, src, len over the flattened rows, rows)."""
    n, full, rem, _ = _docs(L, S, b, e, truncate)
    F = int(full.sum())
    order = np.argsort(-rem, kind="stable")
    order = order[rem[order] > 0]
    lens, starts = np.unique(-rem[order], return_index=True)  # runs, lengths descending
    counts = np.diff(np.append(starts, len(order)))
    frees = []       # sorted distinct free counts of rows that have room left
    heaps = {}       # free count -> heap of row indices
    fill, items = [], []
    pl = []          # (len, row, slot, count)
    for negl, k in zip(lens.tolist(), counts.tolist()):
        ln = -negl
        while k > 0:
            i = bisect.bisect_left(frees, ln)
            if i == len(frees):
                row, f = F + len(fill), S
                fill.append(0)
                items.append(0)
            else:
                f = frees[i]
                row = heapq.heappop(heaps[f])
                if not heaps[f]:
                    del heaps[f]
                    frees.pop(i)
            c = min(k, f // ln)
            m = row - F
            pl.append((ln, row, fill[m], c))
            fill[m] += c * ln
            items[m] += c
            k -= c
            nf = f - c * ln
            if nf > 0:
                if nf not in heaps:
                    heaps[nf] = []
                    bisect.insort(frees, nf)
                heapq.heappush(heaps[nf], row)
    rows = F + len(fill)
    # segments: full rows, then the placed items, then the pad tails; sorted by start afterwards
    fd = np.repeat(np.arange(len(n), dtype=np.int64), full)
    fc = np.arange(F, dtype=np.int64) - np.repeat((np.cumsum(full) - full).astype(np.int64), full)
    st = [np.arange(F, dtype=np.int64) * S]
    dc = [fd]
    sr = [fc * S]
    ln_ = [np.full(F, S, np.int64)]
    if pl:
        P = np.array(pl, np.int64)
        cnt = P[:, 3]
        rep = np.repeat(np.arange(len(P)), cnt)
        j = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        ln = P[rep, 0]
        st.append(P[rep, 1] * S + P[rep, 2] + j * ln)
        dc.append(order.astype(np.int64))
        sr.append(n[order] - ln)
        ln_.append(ln)
    fl = np.array(fill, np.int64)
    tail = np.nonzero(fl < S)[0]
    st.append((F + tail) * S + fl[tail])
    dc.append(np.full(len(tail), -1, np.int64))
    sr.append(np.zeros(len(tail), np.int64))
    ln_.append(S - fl[tail])
    st, dc, sr, ln_ = (np.concatenate(x) for x in (st, dc, sr, ln_))
    o = np.argsort(st, kind="stable")
    return st[o], dc[o], sr[o], ln_[o], rows


def _segments_of_brute(rows, S):
    st, dc, sr, ln_ = [], [], [], []
    for r, segs in enumerate(rows):
        at = r * S
        for d, src, ln in segs:
            st.append(at)
            dc.append(d)
            sr.append(src)
            ln_.append(ln)
            at += ln
        if at < (r + 1) * S:
            st.append(at)
            dc.append(-1)
            sr.append(0)
            ln_.append((r + 1) * S - at)
    a = lambda x: np.array(x, np.int64)  # noqa: E731
    return a(st), a(dc), a(sr), a(ln_), len(rows)


def materialize(ids, tok_offsets, S, bos, eos, pad, truncate, st, dc, sr, ln_, rows, chunk=1 << 24):
    """The five outputs from the segments (vectorised, in chunks of segments)."""
    ids = np.asarray(ids, np.int32)
    offs = np.asarray(tok_offsets, np.int64)
    b, e = int(bos >= 0), int(eos >= 0)
    L = np.diff(offs)
    body = np.minimum(L, S - b - e) if truncate else L
    out = np.full(rows * S, pad, np.int32)
    pos = np.zeros(rows * S, np.int32)
    real = np.nonzero(dc >= 0)[0]
    lo = 0
    while lo < len(real):  # a block of real segments of at most `chunk` slots (at least one segment)
        csum = np.cumsum(ln_[real[lo:]])
        hi = lo + max(1, int(np.searchsorted(csum, chunk, side="right")))
        k = real[lo:hi]
        cnt = ln_[k]
        rep = np.repeat(np.arange(len(k)), cnt)
        o = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        d = dc[k][rep]
        q = sr[k][rep] + o
        j = st[k][rep] + o
        src = offs[:-1][d] + q - b
        v = ids[np.clip(src, 0, max(len(ids) - 1, 0))] if len(ids) else np.zeros(len(q), np.int32)
        if b:
            v = np.where(q == 0, bos, v)
        if e:
            v = np.where(q == b + body[d], eos, v)
        out[j] = v
        pos[j] = o
        lo = hi
    cu = np.append(st, rows * S).astype(np.int32)
    lengths = np.full(rows, S, np.int64)
    pads = dc < 0
    np.subtract.at(lengths, st[pads] // S, ln_[pads])
    return out.reshape(rows, S), pos.reshape(rows, S), cu, lengths.astype(np.int32), dc.copy()


def _placement(n_docs, st, dc, sr, ln_, S, full, rem):
    row = np.full(n_docs, -1, np.int64)
    slot = np.full(n_docs, -1, np.int64)
    one = (full == 1) & (rem == 0)
    packed = (dc >= 0) & (ln_ < S) | ((dc >= 0) & (ln_ == S) & one[np.maximum(dc, 0)])
    d = dc[packed]
    row[d] = st[packed] // S
    slot[d] = st[packed] % S
    return row, slot


def _pack(ids, tok_offsets, S, bos, eos, pad, truncate, placement, planner):
    offs = np.asarray(tok_offsets, np.int64)
    L = np.diff(offs)
    b, e = int(bos >= 0), int(eos >= 0)
    n, full, rem, cut = _docs(L, S, b, e, truncate)
    if planner == "brute":
        st, dc, sr, ln_, rows = _segments_of_brute(plan_brute(L, S, b, e, truncate), S)
    else:
        st, dc, sr, ln_, rows = plan_runs(L, S, b, e, truncate)
    res = materialize(ids, offs, S, bos, eos, pad, truncate, st, dc, sr, ln_, rows)
    counts = np.array([rows, int(n.sum()), len(st), int(cut.sum())], np.int64)
    res = res + (counts,)
    if placement:
        res = res + _placement(len(L), st, dc, sr, ln_, S, full, rem)
    return res


def pack_brute(ids, tok_offsets, S, bos=-1, eos=-1, pad=0, truncate=False, placement=False):
    return _pack(ids, tok_offsets, S, bos, eos, pad, truncate, placement, "brute")


def pack_runs(ids, tok_offsets, S, bos=-1, eos=-1, pad=0, truncate=False, placement=False):
    return _pack(ids, tok_offsets, S, bos, eos, pad, truncate, placement, "runs")


def rows_bound(n_ids, n_docs, S, bos=-1, eos=-1):
    """rows <= floor(2 T / S) + 1, T = n_ids + n_docs * (b + e)."""
    T = n_ids + n_docs * ((bos >= 0) + (eos >= 0))
    return 2 * T // S + 1
