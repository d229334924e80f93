"""Truth for the document selection (td_select_docs, include/tokendagger_hip.h: td_select_spec): straight from the definition.

select_brute   a Python loop over the entries of sel: the definition.
select_numpy   the same, vectorised (np.repeat / cumsum), for large inputs.
Both take sel=None as the identity and max_len=-1 (or None) as "no limit", and return
(ids int32[T], labels int32[T] | None, offsets int64[K + 1], docs int64[K], counts int64[4] = K, T, dropped short, dropped long).
"""
from __future__ import annotations

import numpy as np


def select_brute(ids, tok_offsets, sel=None, min_len=0, max_len=-1, labels=None):
    offs = [int(x) for x in tok_offsets]
    n_docs = len(offs) - 1
    sel = list(range(n_docs)) if sel is None else [int(x) for x in sel]
    max_len = -1 if max_len is None else max_len
    out, lab, o, docs, n_short, n_long = [], [], [0], [], 0, 0
    for d in sel:
        assert 0 <= d < n_docs
        L = offs[d + 1] - offs[d]
        if L < min_len:
            n_short += 1
            continue
        if max_len >= 0 and L > max_len:
            n_long += 1
            continue
        docs.append(d)
        for q in range(L):
            out.append(int(ids[offs[d] + q]))
            if labels is not None:
                lab.append(int(labels[offs[d] + q]))
        o.append(o[-1] + L)
    counts = np.array([len(docs), o[-1], n_short, n_long], np.int64)
    return (np.array(out, np.int32), np.array(lab, np.int32) if labels is not None else None, np.array(o, np.int64),
            np.array(docs, np.int64), counts)


def select_numpy(ids, tok_offsets, sel=None, min_len=0, max_len=-1, labels=None):
    offs = np.asarray(tok_offsets, np.int64)
    n_docs = len(offs) - 1
    sel = np.arange(n_docs, dtype=np.int64) if sel is None else np.asarray(sel, np.int64)
    max_len = -1 if max_len is None else max_len
    assert ((sel >= 0) & (sel < n_docs)).all()
    L = (offs[1:] - offs[:-1])[sel] if n_docs else np.zeros(0, np.int64)
    short = L < min_len
    long_ = ~short & (L > max_len) if max_len >= 0 else np.zeros(len(L), bool)
    docs = sel[~short & ~long_]
    Lk = L[~short & ~long_]
    o = np.concatenate([[0], np.cumsum(Lk)]).astype(np.int64)
    # slot j of the output: its document's first id + its place in the document
    src = np.repeat(offs[docs] - o[:-1], Lk) + np.arange(int(o[-1]), dtype=np.int64)
    counts = np.array([len(docs), o[-1], short.sum(), long_.sum()], np.int64)
    return (np.asarray(ids, np.int32)[src], np.asarray(labels, np.int32)[src] if labels is not None else None, o, docs.astype(np.int64), counts)


def random_case(rng, max_docs=30, max_len=40):
    """0 .. max_docs documents of 0 .. max_len ids; n_sel 0 .. 3 * n_docs with repeats (sometimes the identity, None); min_len /
    max_len random, with max_len = -1 and min_len == max_len among them."""
    n_docs = int(rng.integers(0, max_docs + 1))
    lengths = rng.integers(0, max_len + 1, n_docs)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ids = rng.integers(0, 200000, int(offs[-1])).astype(np.int32)
    labels = rng.integers(-100, 200000, int(offs[-1])).astype(np.int32)
    kind = int(rng.integers(0, 8))
    if kind == 0 or n_docs == 0:
        sel = None if kind % 2 == 0 else np.zeros(0, np.int64)
    else:
        sel = rng.integers(0, n_docs, int(rng.integers(0, 3 * n_docs + 1))).astype(np.int64)
    min_len = int(rng.integers(0, max_len // 2 + 1)) if rng.integers(0, 3) else 0
    pick = int(rng.integers(0, 4))
    max_len_ = -1 if pick == 0 else min_len if pick == 1 else int(rng.integers(min_len, max_len + 2))
    return ids, labels, offs, sel, min_len, max_len_
