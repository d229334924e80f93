"""The truth for the loss labels from byte ranges (td_range_spec, include/tokendagger_hip.h), twice and independently:

ranges_walk   the contract as written: a boolean per byte of every document, set range by range; m_i by counting the marked
              bytes of id i, in plain Python;
ranges_numpy  a difference array over all documents' bytes (+1 at every begin, -1 at every end), its running sum is "marked",
              the running sum of that the marked bytes in front of every position; m_i is a difference of two entries.  Fast
              enough for millions of ids.

Token lengths come from the vocabulary on the host (lengths[id], offsets_truth.id_lengths), never from the device.  starts None:
the covered rule (an id starts where the one before it in its document ends); else int64 byte starts per id.
Both return (labels int32, mask uint8, trained_offsets int64[n_docs + 1], counts int64[4] = trained ids, partially marked ids,
marked bytes, 0)."""
from __future__ import annotations

import numpy as np

RULES = ("overlap", "inside", "start")


def ranges_walk(ids, tok_offsets, range_offsets, ranges, lengths, rule="overlap", ignore_index=-100, starts=None):
    ids = [int(x) for x in ids]
    offs = [int(x) for x in tok_offsets]
    ro = [int(x) for x in range_offsets]
    rg = [(int(b), int(e)) for b, e in np.asarray(ranges, dtype=np.int64).reshape(-1, 2)]
    total = offs[-1]
    labels = np.full(total, ignore_index, dtype=np.int32)
    mask = np.zeros(total, dtype=np.uint8)
    toff = np.zeros(len(offs), dtype=np.int64)
    trained = partial = marked_bytes = 0
    for d in range(len(offs) - 1):
        toff[d] = trained
        mine = rg[ro[d]:ro[d + 1]]
        pos, where = 0, []
        for q in range(offs[d], offs[d + 1]):
            s = pos if starts is None else int(starts[q])
            where.append((s, s + int(lengths[ids[q]])))
            pos = where[-1][1]
        size = max([e for _, e in where] + [e for _, e in mine] + [0])
        marked = [False] * size
        for b, e in mine:
            assert 0 <= b <= e
            marked_bytes += e - b
            for p in range(b, e):
                marked[p] = True
        for q, (s, e) in zip(range(offs[d], offs[d + 1]), where):
            m = sum(marked[s:e])
            tr = {"overlap": m > 0, "inside": m == e - s, "start": s < size and marked[s]}[rule]
            partial += 0 < m < e - s
            if tr:
                labels[q] = ids[q]
                mask[q] = 1
                trained += 1
    toff[-1] = trained
    return labels, mask, toff, np.asarray([trained, partial, marked_bytes, 0], dtype=np.int64)


def ranges_numpy(ids, tok_offsets, range_offsets, ranges, lengths, rule="overlap", ignore_index=-100, starts=None):
    ids = np.asarray(ids, dtype=np.int64)
    offs = np.asarray(tok_offsets, dtype=np.int64)
    ro = np.asarray(range_offsets, dtype=np.int64)
    rg = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)[:int(ro[-1])]
    total, n_docs = int(offs[-1]), len(offs) - 1
    ids = ids[:total]
    ln = np.asarray(lengths, dtype=np.int64)[ids] if total else np.zeros(0, np.int64)
    doc = np.repeat(np.arange(n_docs), np.diff(offs))
    if starts is None:
        cs = np.concatenate([[0], np.cumsum(ln)])
        s = cs[:-1] - cs[offs[doc]]
    else:
        s = np.asarray(starts, dtype=np.int64)[:total]
    e = s + ln
    # every document gets a stretch of one global byte axis, long enough for its ids and its ranges (+ 1: position `size` exists)
    rdoc = np.repeat(np.arange(n_docs), np.diff(ro))
    size = np.zeros(n_docs, dtype=np.int64)
    np.maximum.at(size, doc, e)
    np.maximum.at(size, rdoc, rg[:, 1])
    base = np.concatenate([[0], np.cumsum(size + 1)])
    diff = np.zeros(int(base[-1]) + 1, dtype=np.int64)
    np.add.at(diff, base[rdoc] + rg[:, 0], 1)
    np.add.at(diff, base[rdoc] + rg[:, 1], -1)
    marked = np.cumsum(diff) > 0                                  # marked[p]: byte p is marked
    before = np.concatenate([[0], np.cumsum(marked)])             # before[p]: marked bytes in front of p
    m = before[base[doc] + e] - before[base[doc] + s]
    trained = {"overlap": m > 0, "inside": m == ln, "start": marked[base[doc] + s]}[rule]
    labels = np.where(trained, ids, ignore_index).astype(np.int32)
    toff = np.concatenate([[0], np.cumsum(trained)]).astype(np.int64)[offs]
    counts = [int(trained.sum()), int(((m > 0) & (m < ln)).sum()), int((rg[:, 1] - rg[:, 0]).sum()), 0]
    return labels, trained.astype(np.uint8), toff, np.asarray(counts, dtype=np.int64)


def random_case(rng, lengths, id_pool, max_docs=12, max_len=40):
    """ids drawn from id_pool (ids of the vocabulary with different byte lengths); per document a sorted, disjoint list of ranges
    inside its bytes.  Makes empty documents, documents without ranges, empty ranges, touching ranges, ranges of one byte (shorter
    than a token) and ranges that end exactly at the document's end.  -> (ids, tok_offsets, range_offsets, ranges[n, 2])"""
    n_docs = int(rng.integers(0, max_docs + 1))
    n_ids = rng.integers(0, max_len + 1, n_docs)
    n_ids[rng.random(n_docs) < 0.2] = 0
    n_ids[rng.random(n_docs) < 0.15] = 1
    offs = np.concatenate([[0], np.cumsum(n_ids)]).astype(np.int64)
    ids = np.asarray(id_pool, dtype=np.int32)[rng.integers(0, len(id_pool), int(offs[-1]))]
    ro, out = [0], []
    for d in range(n_docs):
        size = int(np.asarray(lengths)[ids[offs[d]:offs[d + 1]]].sum())
        mine = []
        if rng.random() >= 0.2:  # (else: a document without ranges)
            k = int(rng.integers(1, 9))
            cuts = np.sort(rng.integers(0, size + 1, 2 * k))
            for b, e in cuts.reshape(-1, 2):
                kind = rng.random()
                if kind < 0.15:
                    e = b                          # an empty range
                elif kind < 0.35:
                    e = min(b + 1, e)              # one byte
                if mine and rng.random() < 0.3:
                    b = mine[-1][1]                # touches the range before it
                    e = max(e, b)
                mine.append((int(b), int(e)))
            if rng.random() < 0.3:                 # the last range ends exactly at the document's end
                last = mine[-1][1]
                mine.append((last if rng.random() < 0.5 else max(last, size - 1), size))
        out += mine
        ro.append(len(out))
    return ids, offs, np.asarray(ro, dtype=np.int64), np.asarray(out, dtype=np.int64).reshape(-1, 2)
