"""The truth for the loss labels (td_labels_spec, include/tokendagger_hip.h), twice and independently:

labels_walk   the contract as written: the sequential two-state walk over every document, in plain Python;
labels_numpy  the vectorised "last event" form: events by shifted compares, inside(i) from the position of the last event in
              front of i by a running maximum.  Fast enough for documents of millions of ids.

Both return (labels int32, mask uint8, trained_offsets int64[n_docs + 1], counts int64[4])."""
from __future__ import annotations

import numpy as np


def labels_walk(ids, tok_offsets, open, close, ignore_index=-100, train_close=True):
    ids = [int(x) for x in ids]
    offs = [int(x) for x in tok_offsets]
    total = offs[-1]
    labels = np.full(total, ignore_index, dtype=np.int32)
    mask = np.zeros(total, dtype=np.uint8)
    toff = np.zeros(len(offs), dtype=np.int64)
    openers = [list(map(int, o)) for o in open]
    closers = set(map(int, close))
    trained = spans = unterminated = 0
    for d in range(len(offs) - 1):
        a, z = offs[d], offs[d + 1]
        toff[d] = trained
        inside = False
        for q in range(a, z):
            is_close = ids[q] in closers
            if inside and (train_close or not is_close):
                labels[q] = ids[q]
                mask[q] = 1
                trained += 1
            is_open = any(q - len(o) + 1 >= a and ids[q - len(o) + 1:q + 1] == o for o in openers)
            assert not (is_open and is_close)
            if is_open:
                spans += not inside
                inside = True
            elif is_close:
                inside = False
        unterminated += inside
    toff[-1] = trained
    return labels, mask, toff, np.asarray([trained, spans, unterminated, 0], dtype=np.int64)


def labels_numpy(ids, tok_offsets, open, close, ignore_index=-100, train_close=True):
    ids = np.asarray(ids, dtype=np.int64)
    offs = np.asarray(tok_offsets, dtype=np.int64)
    total, n_docs = int(offs[-1]), len(offs) - 1
    if total == 0:
        return (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8), np.zeros(n_docs + 1, dtype=np.int64), np.zeros(4, dtype=np.int64))
    ids = ids[:total]
    pos = np.arange(total, dtype=np.int64)
    # the start of every position's document
    L = np.diff(offs)
    doc_start = np.repeat(offs[:-1], L)
    is_close = np.isin(ids, np.asarray(list(close), dtype=np.int64)) if len(close) else np.zeros(total, dtype=bool)
    is_open = np.zeros(total, dtype=bool)
    for o in open:
        k = len(o)
        if k > total:
            continue
        m = np.ones(total - k + 1, dtype=bool)
        for j, v in enumerate(o):
            m &= ids[j:total - k + 1 + j] == int(v)
        hit = np.zeros(total, dtype=bool)
        hit[k - 1:] = m  # (the opener ends at this position)
        is_open |= hit & (pos - (k - 1) >= doc_start)
    assert not (is_open & is_close).any()
    # the last event at a position < i, as position + 1 (0: none), and whether it is an open event
    ev = is_open | is_close
    last = np.maximum.accumulate(np.where(ev, pos + 1, 0))
    last_before = np.concatenate([[0], last[:-1]])
    in_doc = last_before > doc_start  # (the event's position last_before - 1 >= doc_start)
    inside = in_doc & is_open[np.maximum(last_before - 1, 0)]
    trained = inside & (~is_close | bool(train_close))
    labels = np.where(trained, ids, ignore_index).astype(np.int32)
    csum = np.concatenate([[0], np.cumsum(trained)]).astype(np.int64)
    toff = csum[offs]
    spans = int((is_open & ~inside).sum())
    # a document ends inside: its last event is an open event
    ends = offs[1:]
    nonempty = L > 0
    le = last[np.maximum(ends - 1, 0)]
    unterminated = int((nonempty & (le > offs[:-1]) & is_open[np.maximum(le - 1, 0)]).sum())
    return labels, trained.astype(np.uint8), toff, np.asarray([int(trained.sum()), spans, unterminated, 0], dtype=np.int64)


def random_case(rng, alphabet=6, max_docs=12, max_len=40):
    """Small ids over a small alphabet (events are dense); openers that are prefixes / suffixes of each other or overlap
    themselves; closers disjoint from the openers' ids (possibly none)."""
    n_docs = int(rng.integers(0, max_docs + 1))
    lengths = rng.integers(0, max_len + 1, n_docs)
    lengths[rng.random(n_docs) < 0.2] = 0
    lengths[rng.random(n_docs) < 0.15] = 1
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ids = rng.integers(0, alphabet, int(offs[-1])).astype(np.int32)
    n_close = int(rng.integers(0, 3))
    close = sorted(rng.choice(alphabet, n_close, replace=False).tolist())
    free = [x for x in range(alphabet) if x not in close]
    open = []
    base = [int(x) for x in rng.choice(free, int(rng.integers(1, 5)))]
    open.append(base)
    kind = int(rng.integers(0, 5))
    if kind == 0 and len(base) > 1:
        open.append(base[:-1])          # a prefix
    elif kind == 1 and len(base) > 1:
        open.append(base[1:])           # a suffix
    elif kind == 2:
        open.append([free[0], free[0]])  # overlaps itself
    elif kind == 3:
        open.append([int(x) for x in rng.choice(free, int(rng.integers(1, 9)))])
    uniq = []
    for o in open:
        if o not in uniq:
            uniq.append(o)
    return ids, offs, uniq, close, bool(rng.integers(0, 2))
