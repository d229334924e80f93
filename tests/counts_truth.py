"""Two independent statements of the token-counts contract (include/tokendagger_hip.h, td_counts_spec) and a generator of random
cases.  Both return (counts int64[n_groups, n_bins], info int64[4] = counted, negative, too_large, bad_group): every visited
position falls into exactly one of bad_group, negative, too_large, counted, in this order of precedence."""
import numpy as np


def _visited(ids, tok_offsets):
    ids = np.asarray(ids, dtype=np.int32)
    if tok_offsets is None:
        return ids, 0, len(ids)
    o = np.asarray(tok_offsets, dtype=np.int64)
    return ids, int(o[0]), int(o[-1])


def counts_numpy(ids, n_bins, tok_offsets=None, groups=None, n_groups=1):
    """Vectorised: the group of every position by repeat, bincount on the key."""
    ids, lo, hi = _visited(ids, tok_offsets if groups is not None else None)
    v = ids[lo:hi].astype(np.int64)
    if groups is None:
        g = np.zeros(len(v), dtype=np.int64)
    else:
        g = np.repeat(np.asarray(groups, dtype=np.int64), np.diff(np.asarray(tok_offsets, dtype=np.int64)))
    bad = (g < 0) | (g >= n_groups)
    neg = ~bad & (v < 0)
    big = ~bad & ~neg & (v >= n_bins)
    ok = ~bad & ~neg & ~big
    counts = np.bincount(g[ok] * n_bins + v[ok], minlength=n_groups * n_bins).astype(np.int64).reshape(n_groups, n_bins)
    return counts, np.asarray([ok.sum(), neg.sum(), big.sum(), bad.sum()], dtype=np.int64)


def counts_brute(ids, n_bins, tok_offsets=None, groups=None, n_groups=1):
    """A plain loop over documents and positions."""
    ids = [int(x) for x in np.asarray(ids)]
    counts = [[0] * n_bins for _ in range(n_groups)]
    info = [0, 0, 0, 0]
    if groups is None:
        docs = [(0, len(ids), 0)]
    else:
        docs = [(int(tok_offsets[d]), int(tok_offsets[d + 1]), int(groups[d])) for d in range(len(groups))]
    for a, b, g in docs:
        for i in range(a, b):
            if g < 0 or g >= n_groups:
                info[3] += 1
            elif ids[i] < 0:
                info[1] += 1
            elif ids[i] >= n_bins:
                info[2] += 1
            else:
                info[0] += 1
                counts[g][ids[i]] += 1
    return np.asarray(counts, dtype=np.int64).reshape(n_groups, n_bins), np.asarray(info, dtype=np.int64)


def random_case(rng, max_docs=12, max_len=40, bad_groups=True):
    """-> dict(ids, n_tokens, tok_offsets, groups, n_bins, n_groups): empty documents, negative values, values at and above n_bins,
    groups outside [0, n_groups) (bad_groups), tok_offsets[0] > 0 and ids behind the last document; a few values are hot."""
    n_bins = int(rng.choice([1, 2, 7, 64, 300, 5000]))
    n_groups = int(rng.choice([1, 2, 3, 8]))
    n_docs = int(rng.integers(0, max_docs + 1))
    lens = rng.integers(0, max_len + 1, size=n_docs)
    lens[rng.random(n_docs) < 0.25] = 0
    lead = int(rng.integers(0, 6)) if rng.random() < 0.4 else 0
    tail = int(rng.integers(0, 6)) if rng.random() < 0.4 else 0
    offs = (lead + np.concatenate([[0], np.cumsum(lens)])).astype(np.int64)
    n = int(offs[-1]) + tail
    hot = rng.integers(0, n_bins, size=3)
    ids = np.where(rng.random(n) < 0.5, hot[rng.integers(0, 3, size=n)], rng.integers(0, n_bins, size=n)).astype(np.int64)
    r = rng.random(n)
    ids[r < 0.08] = -100
    ids[(r >= 0.08) & (r < 0.11)] = rng.integers(-5, 0, size=int(((r >= 0.08) & (r < 0.11)).sum()))
    ids[(r >= 0.11) & (r < 0.15)] = n_bins + rng.integers(0, 3, size=int(((r >= 0.11) & (r < 0.15)).sum()))
    ids[(r >= 0.15) & (r < 0.16)] = 2**31 - 1
    groups = rng.integers(0, n_groups, size=n_docs).astype(np.int32)
    if bad_groups and n_docs and rng.random() < 0.3:
        k = rng.integers(0, n_docs, size=max(1, n_docs // 4))
        groups[k] = rng.choice([-1, n_groups, n_groups + 5, -2**31], size=len(k))
    return dict(ids=ids.astype(np.int32), n_tokens=n, tok_offsets=offs, groups=groups, n_bins=n_bins, n_groups=n_groups)


def border_documents():
    """Documents of 4095 / 4096 / 4097 / 9000 ids, and documents that start 1 - 3 ids before a tile border; 5 groups."""
    lens = [4095, 4096, 4097, 9000]
    for k in (3, 2, 1):  # a filler up to k ids before the next border, then ten ids across it
        lens += [(-sum(lens) - k) % 4096 or 4096, 10]
    lens.append(100)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert {int(-o % 4096) for o in offs[1:]} >= {1, 2, 3}
    rng = np.random.default_rng(8)
    ids = rng.integers(0, 300, size=int(offs[-1])).astype(np.int32)
    groups = (np.arange(len(lens)) % 5).astype(np.int32)
    return ids, offs, groups, 300, 5


def empty_documents_tile():
    """5000 empty documents inside one tile, between two documents of other groups: more than the tile's table holds."""
    lens = [3000] + [0] * 5000 + [3000, 0, 0, 4096]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.random.default_rng(9).integers(0, 64, size=int(offs[-1])).astype(np.int32)
    groups = (np.arange(len(lens)) % 3).astype(np.int32)
    groups[0], groups[5001] = 1, 2
    return ids, offs, groups, 64, 3
