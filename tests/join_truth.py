"""Truth for the field joins (td_join_fields, include/tokendagger_hip.h: td_join_spec): straight from the definition.

A join is described by a plain dict (make_join): K fields, each {"before": [ids], "max_len": -1 | n, "rank": r, "type": v,
"keep_tail", "train", "train_before"}, and "tail", "tail_type", "train_tail", "max_total" (-1: none), "shrink" ("order" |
"longest"), "field_major", "ignore_index".  capi_spec(join) is its td_join_spec.

join_brute     Python loops: the definition, TD_JOIN_SHRINK_LONGEST as the literal one-id-at-a-time loop.
join_numpy     the same, vectorised (sorting for the level of LONGEST; np.repeat / cumsum for the slots), for large inputs.
kept_lengths   one example's c_f and whether it is dropped, by the loop (what join_brute runs).
longest_closed the closed form of LONGEST restated in Python integers, for lengths no loop can walk.
All return (ids int32[T], labels int32[T], types int32[T], offsets int64[E + 1], examples int64[E], field_len int32[E, K],
counts int64[4] = E, T, dropped, truncated).
"""
from __future__ import annotations

import numpy as np


def field(before=(), max_len=-1, rank=0, type=0, keep_tail=False, train=False, train_before=False):
    return {"before": [int(x) for x in before], "max_len": int(max_len), "rank": int(rank), "type": int(type), "keep_tail": bool(keep_tail),
            "train": bool(train), "train_before": bool(train_before)}


def make_join(fields, tail=(), tail_type=0, train_tail=False, max_total=-1, shrink="order", field_major=False, ignore_index=-100):
    return {"fields": list(fields), "tail": [int(x) for x in tail], "tail_type": int(tail_type), "train_tail": bool(train_tail),
            "max_total": int(max_total), "shrink": shrink, "field_major": bool(field_major), "ignore_index": int(ignore_index)}


def capi_spec(join):
    from tokendagger_amd import capi
    fs = [capi.join_field(f["before"], None if f["max_len"] < 0 else f["max_len"], f["rank"], f["type"], f["keep_tail"], f["train"],
                          f["train_before"]) for f in join["fields"]]
    return capi.join_spec(fs, join["tail"], join["tail_type"], join["train_tail"], None if join["max_total"] < 0 else join["max_total"],
                          join["shrink"], join["field_major"], join["ignore_index"])


def doc_of(join, n_ex, x, f):
    return f * n_ex + x if join["field_major"] else x * len(join["fields"]) + f


def kept_lengths(join, L):
    """L[f] -> (c[f], dropped): steps 1 to 4 of the contract, LONGEST one id at a time."""
    fs = join["fields"]
    K = len(fs)
    c = [min(L[f], fs[f]["max_len"]) if fs[f]["max_len"] >= 0 else L[f] for f in range(K)]
    fixed = sum(len(f["before"]) for f in fs) + len(join["tail"])
    need = fixed + sum(c)
    if join["max_total"] < 0 or need <= join["max_total"]:
        return c, False
    over = need - join["max_total"]
    if join["shrink"] == "order":
        for f in sorted((f for f in range(K) if fs[f]["rank"] > 0), key=lambda f: (fs[f]["rank"], f)):
            cut = min(c[f], over)
            c[f] -= cut
            over -= cut
    else:
        while over > 0:
            best = -1
            for f in range(K):
                if fs[f]["rank"] > 0 and c[f] > 0 and (best < 0 or c[f] >= c[best]):  # (>=: a tie goes to the highest index)
                    best = f
            if best < 0:
                break
            c[best] -= 1
            over -= 1
    return c, over > 0


def longest_closed(c, shrinkable, over):
    """LONGEST without the loop: B ids stay in the shrinkable fields; the largest level l with sum min(c_f, l) <= B; every
    shrinkable field above l cut to l; the rest of B, single ids, to the lowest-indexed of them.  -> (c, dropped)."""
    c = list(c)
    sh = [f for f in range(len(c)) if shrinkable[f]]
    S = sum(c[f] for f in sh)
    if over > S:
        return c, True
    if over <= 0:
        return c, False
    B = S - over
    lo, hi = 0, max(c[f] for f in sh)  # the largest l in [0, max] with g(l) <= B, by bisection on integers
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if sum(min(c[f], mid) for f in sh) <= B:
            lo = mid
        else:
            hi = mid - 1
    rest = B - sum(min(c[f], lo) for f in sh)
    for f in sh:
        if c[f] > lo:
            c[f] = lo + (1 if rest > 0 else 0)
            rest -= 1 if rest > 0 else 0
    return c, False


def _i32(x):
    return np.array(x, np.int64).astype(np.int32)


def join_brute(ids, tok_offsets, join):
    offs = [int(x) for x in tok_offsets]
    fs = join["fields"]
    K = len(fs)
    assert (len(offs) - 1) % K == 0
    n_ex = (len(offs) - 1) // K
    ign = join["ignore_index"]
    out, lab, typ, o, exs, flen, n_drop, n_trunc = [], [], [], [0], [], [], 0, 0
    for x in range(n_ex):
        lo = [offs[doc_of(join, n_ex, x, f)] for f in range(K)]
        L = [offs[doc_of(join, n_ex, x, f) + 1] - lo[f] for f in range(K)]
        assert all(v >= 0 for v in L)
        c, dropped = kept_lengths(join, L)
        if dropped:
            n_drop += 1
            continue
        n_trunc += any(c[f] < L[f] for f in range(K))
        exs.append(x)
        flen.append(c)
        for f in range(K):
            for v in fs[f]["before"]:
                out.append(v)
                lab.append(v if fs[f]["train_before"] else ign)
                typ.append(fs[f]["type"])
            first = lo[f] + (L[f] - c[f] if fs[f]["keep_tail"] else 0)
            for q in range(c[f]):
                v = int(ids[first + q])
                out.append(v)
                lab.append(v if fs[f]["train"] else ign)
                typ.append(fs[f]["type"])
        for v in join["tail"]:
            out.append(v)
            lab.append(v if join["train_tail"] else ign)
            typ.append(join["tail_type"])
        o.append(len(out))
    counts = np.array([len(exs), o[-1], n_drop, n_trunc], np.int64)
    return (_i32(out), _i32(lab), _i32(typ), np.array(o, np.int64), np.array(exs, np.int64), np.array(flen, np.int32).reshape(len(exs), K),
            counts)


def lengths_numpy(join, L):
    """L int64[n_ex, K] -> (c int64[n_ex, K], dropped bool[n_ex])."""
    fs = join["fields"]
    K = len(fs)
    L = np.asarray(L, np.int64).reshape(-1, K)
    cap = np.array([f["max_len"] for f in fs], np.int64)
    c = np.where(cap >= 0, np.minimum(L, cap), L)
    fixed = sum(len(f["before"]) for f in fs) + len(join["tail"])
    if join["max_total"] < 0:
        return c, np.zeros(len(L), bool)
    over = np.maximum(fixed + c.sum(1) - join["max_total"], 0)
    sh = [f for f in range(K) if fs[f]["rank"] > 0]
    if join["shrink"] == "order":
        for f in sorted(sh, key=lambda f: (fs[f]["rank"], f)):
            cut = np.minimum(c[:, f], over)
            c[:, f] -= cut
            over = over - cut
        return c, over > 0
    if not sh:
        return c, over > 0
    cs = c[:, sh]
    m = len(sh)
    S = cs.sum(1)
    dropped = over > S
    B = np.where(dropped, S, S - over)  # (a dropped example's lengths are of no interest: left uncut)
    s = np.sort(cs, axis=1)
    prefix = np.concatenate([np.zeros((len(s), 1), np.int64), np.cumsum(s, axis=1)[:, :-1]], axis=1)
    width = m - np.arange(m, dtype=np.int64)
    above = prefix + width * s > B[:, None]          # the level lies below s[:, i]
    cutting = above.any(1)
    i = np.argmax(above, axis=1)
    r = np.arange(len(s))
    room = B - prefix[r, i]
    level = np.where(cutting, room // width[i], s[:, -1])
    rest = np.where(cutting, room % width[i], 0)
    tall = cs > level[:, None]
    nth = np.cumsum(tall, axis=1) - 1                # a tall field's place among the tall ones, by index
    c[:, sh] = np.where(tall, level[:, None] + (nth < rest[:, None]), cs)
    return c, dropped


def join_numpy(ids, tok_offsets, join):
    offs = np.asarray(tok_offsets, np.int64)
    ids = np.asarray(ids, np.int32)
    fs = join["fields"]
    K = len(fs)
    assert (len(offs) - 1) % K == 0
    n_ex = (len(offs) - 1) // K
    x = np.arange(n_ex, dtype=np.int64)
    docs = np.stack([f * n_ex + x if join["field_major"] else x * K + f for f in range(K)], axis=1).reshape(n_ex, K)
    lo, L = offs[docs], offs[docs + 1] - offs[docs]
    assert (L >= 0).all()
    c, dropped = lengths_numpy(join, L)
    keep = ~dropped
    exs, c, lo, L = x[keep], c[keep], lo[keep], L[keep]
    E = len(exs)
    P = 2 * K + 1
    # the parts of every kept example: their lengths, and what a slot of them is
    plen = np.zeros((E, P), np.int64)
    first = np.zeros((E, P), np.int64)       # a body's first kept id
    lit = np.zeros((K + 1, 16), np.int64)    # before_f at f, the tail at K
    for f in range(K):
        plen[:, 2 * f] = len(fs[f]["before"])
        plen[:, 2 * f + 1] = c[:, f]
        first[:, 2 * f + 1] = lo[:, f] + (L[:, f] - c[:, f] if fs[f]["keep_tail"] else 0)
        lit[f, :len(fs[f]["before"])] = fs[f]["before"]
    plen[:, 2 * K] = len(join["tail"])
    lit[K, :len(join["tail"])] = join["tail"]
    p_type = np.array([fs[p // 2]["type"] if p < 2 * K else join["tail_type"] for p in range(P)], np.int64)
    p_train = np.array([(fs[p // 2]["train"] if p % 2 else fs[p // 2]["train_before"]) if p < 2 * K else join["train_tail"] for p in range(P)], bool)
    flat = plen.reshape(-1)
    starts = np.concatenate([[0], np.cumsum(flat)]).astype(np.int64)
    T = int(starts[-1])
    part = np.repeat(np.arange(E * P, dtype=np.int64), flat)  # slot -> its part (example * P + p)
    within = np.arange(T, dtype=np.int64) - starts[part]
    p = part % P
    body = p % 2 == 1
    out = np.empty(T, np.int64)
    out[body] = ids[first.reshape(-1)[part[body]] + within[body]]
    out[~body] = lit[p[~body] // 2, within[~body]]
    lab = np.where(p_train[p], out, join["ignore_index"])
    o = np.concatenate([[0], np.cumsum(plen.sum(1))]).astype(np.int64)
    counts = np.array([E, T, dropped.sum(), (c < L).any(1).sum()], np.int64)
    return (out.astype(np.int32), lab.astype(np.int32), p_type[p].astype(np.int32), o, exs, c.astype(np.int32).reshape(E, K), counts)


def random_join(rng, K=None, lit_pool=None, max_len=12):
    """A random join of K (1 .. 8) fields: literals of 0 .. 3 ids (sometimes 16) from lit_pool, caps, ranks with ties and zeros, both
    shrink modes, max_total from "cuts nothing" to "below the literals"."""
    K = int(rng.integers(1, 9)) if K is None else K
    pool = np.arange(1000) if lit_pool is None else np.asarray(lit_pool)
    lits = lambda: pool[rng.integers(0, len(pool), int(rng.choice([0, 0, 1, 2, 3, 16])))].tolist()
    fs = [field(lits(), -1 if rng.integers(0, 3) else int(rng.integers(0, max_len)), int(rng.integers(0, 4)), int(rng.integers(-3, 4)),
                bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2))) for _ in range(K)]
    tail = lits()
    fixed = sum(len(f["before"]) for f in fs) + len(tail)
    pick = int(rng.integers(0, 5))
    max_total = -1 if pick == 0 else int(rng.integers(0, fixed + 1)) if pick == 1 else fixed + int(rng.integers(0, K * max_len + 1))
    return make_join(fs, tail, int(rng.integers(-3, 4)), bool(rng.integers(0, 2)), max_total, "order" if rng.integers(0, 2) else "longest",
                     bool(rng.integers(0, 2)), int(rng.choice([-100, -1, 0, 7])))


def random_case(rng, max_ex=12, max_len=12, K=None, lit_pool=None):
    """(ids, offs, join): 0 .. max_ex examples of a random_join, field lengths 0 .. max_len with empty fields, equal lengths and
    all-empty examples among them."""
    join = random_join(rng, K, lit_pool, max_len)
    K = len(join["fields"])
    n_ex = int(rng.integers(0, max_ex + 1))
    kind = rng.integers(0, 4, n_ex)  # 0: all empty, 1: all equal, else: free
    L = rng.integers(0, max_len + 1, (n_ex, K))
    L[kind == 0] = 0
    eq = kind == 1
    L[eq] = L[eq][:, :1]
    L[rng.integers(0, 4, (n_ex, K)) == 0] = 0
    lengths = np.zeros(n_ex * K, np.int64)
    for x in range(n_ex):
        for f in range(K):
            lengths[doc_of(join, n_ex, x, f)] = L[x, f]
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ids = rng.integers(0, 200000, int(offs[-1])).astype(np.int32)
    return ids, offs, join
