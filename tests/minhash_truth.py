"""The MinHash contract of include/tokendagger_hip.h restated twice, with its constants typed out here (nothing is read from the C++
headers): minhash_brute in plain Python integers, one shingle and one permutation at a time, and minhash_numpy, vectorised over all
shingles of a batch, for the sizes the GPU tests use.  Also the inputs both the CPU and the GPU tests draw from.

  shingle hash   x = finish(poly(window), len): poly is the polynomial in 0x9E3779B1 modulo 2^32 over the ids as uint32, the first id
                 at the highest power; finish adds len * 0x7FEB352D and runs the murmur3 finaliser
  permutations   a_j = mix64(seed + (2j + 1) G) | 1, b_j = mix64(seed + (2j + 2) G), h_j(x) = (a_j x + b_j mod 2^64) >> 32
  signature      sig[d][j] = min over the document's shingles of h_j(x), 0xFFFFFFFF without one
  band keys      key[d][b] = fold of mix64 over sig[d][b * rows .. (b + 1) * rows), started from mix64(b + 1)
  counts         shingles hashed, documents without an id, documents of 1 .. k - 1 ids, 0
"""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
BASE = 0x9E3779B1
GOLDEN = 0x9E3779B97F4A7C15
TILE = 4096
MAX_K = 64
MAX_PERM = 1024


def mix64(z: int) -> int:
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def params(seed: int, num_perm: int):
    """-> (a uint64[num_perm], b uint64[num_perm])"""
    a = [mix64(seed + (2 * j + 1) * GOLDEN) | 1 for j in range(num_perm)]
    b = [mix64(seed + (2 * j + 2) * GOLDEN) for j in range(num_perm)]
    return np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)


def shingle_hash(window, length: int) -> int:
    h = 0
    for v in window:
        h = (h * BASE + (int(v) & M32)) & M32
    x = (h + length * 0x7FEB352D) & M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def doc_shingles(doc, k: int) -> list[int]:
    L = len(doc)
    if L == 0:
        return []
    if L < k:
        return [shingle_hash(doc, L)]
    return [shingle_hash(doc[q:q + k], k) for q in range(L - k + 1)]


def band_keys_of(sig_row, bands: int, rows: int) -> list[int]:
    out = []
    for b in range(bands):
        h = mix64(b + 1)
        for j in range(b * rows, (b + 1) * rows):
            h = mix64(h ^ int(sig_row[j]))
        out.append(h)
    return out


def minhash_brute(ids, offs, k=5, num_perm=128, seed=1, bands=0, rows=0):
    """-> (sig uint32[n_docs, num_perm], keys uint64[n_docs, bands], counts int64[4]); plain Python, small inputs only."""
    ids = [int(v) for v in ids]
    offs = [int(v) for v in offs]
    n_docs = len(offs) - 1
    a, b = params(seed, num_perm)
    a, b = [int(v) for v in a], [int(v) for v in b]
    sig = np.full((n_docs, num_perm), M32, dtype=np.uint32)
    keys = np.zeros((n_docs, bands), dtype=np.uint64)
    counts = np.zeros(4, dtype=np.int64)
    for d in range(n_docs):
        doc = ids[offs[d]:offs[d + 1]]
        xs = doc_shingles(doc, k)
        counts[0] += len(xs)
        counts[1] += len(doc) == 0
        counts[2] += 0 < len(doc) < k
        for j in range(num_perm):
            for x in xs:
                sig[d, j] = min(int(sig[d, j]), ((a[j] * x + b[j]) & M64) >> 32)
        keys[d] = band_keys_of(sig[d], bands, rows)
    return sig, keys, counts


def _finish(h, length):
    x = (h + np.uint32((length * 0x7FEB352D) & M32)).astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def all_shingles(ids, offs, k):
    """-> (x uint32[n], doc int64[n]) of every shingle of the batch, ordered by document."""
    u = np.ascontiguousarray(np.asarray(ids, dtype=np.int32)).view(np.uint32)
    offs = np.asarray(offs, dtype=np.int64)
    lens = np.diff(offs)
    total = int(offs[-1])
    xs, docs = [], []
    if total >= k:  # the full windows at every start of the stream, then the ones inside a document
        h = np.zeros(total - k + 1, dtype=np.uint32)
        for i in range(k):
            h = h * np.uint32(BASE) + u[i:total - k + 1 + i]
        x = _finish(h, k)
        start_doc = np.searchsorted(offs, np.arange(total - k + 1), side="right") - 1
        ok = np.arange(total - k + 1) + k <= offs[start_doc + 1]
        xs.append(x[ok])
        docs.append(start_doc[ok])
    for d in np.nonzero((lens > 0) & (lens < k))[0]:
        xs.append(np.asarray([shingle_hash(u[offs[d]:offs[d + 1]], int(lens[d]))], dtype=np.uint32))
        docs.append(np.asarray([d], dtype=np.int64))
    if not xs:
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int64)
    x, doc = np.concatenate(xs), np.concatenate(docs).astype(np.int64)
    order = np.argsort(doc, kind="stable")
    return x[order], doc[order]


def minhash_numpy(ids, offs, k=5, num_perm=128, seed=1, bands=0, rows=0):
    """-> (sig, keys, counts) like minhash_brute.  ids behind offs[-1] are not looked at."""
    offs = np.asarray(offs, dtype=np.int64)
    n_docs = len(offs) - 1
    lens = np.diff(offs)
    x, doc = all_shingles(np.asarray(ids)[:int(offs[-1])], offs, k)
    a, b = params(seed, num_perm)
    sig = np.full((n_docs, num_perm), M32, dtype=np.uint32)
    if len(x):
        have, first = np.unique(doc, return_index=True)
        x64 = x.astype(np.uint64)
        with np.errstate(over="ignore"):
            for j0 in range(0, num_perm, 32):
                h = (a[j0:j0 + 32, None] * x64[None, :] + b[j0:j0 + 32, None]) >> np.uint64(32)
                sig[have, j0:j0 + 32] = np.minimum.reduceat(h, first, axis=1).T.astype(np.uint32)
    keys = np.zeros((n_docs, bands), dtype=np.uint64)
    for d in range(n_docs):
        keys[d] = band_keys_of(sig[d], bands, rows)
    counts = np.asarray([len(x), int((lens == 0).sum()), int(((lens > 0) & (lens < k)).sum()), 0], dtype=np.int64)
    return sig, keys, counts


def same(got, want, what=""):
    for name, g, w in zip(("signatures", "band_keys", "counts"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what}: {name} differ at {len(bad)} places, first {bad[0].tolist()}: got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}")


# ---- inputs ------------------------------------------------------------------------------------------------------------------------

def offsets_of(lens):
    o = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=o[1:])
    return o


def edge_lengths(rng, k):
    """Document lengths that put boundaries on lane-run edges (16), on a tile edge, one id either side of it and inside the last k - 1
    starts of a tile, with one document over four tiles and fillers that shift everything behind them."""
    base = [0, 1, max(k - 1, 0), k, k + 1, 15, 16, 17, 4095, 4096, 4097]
    lens = [12300]  # [0, 12300): tiles 0 .. 3, then 4096 - 12300 % 4096 = 4084 ids to the next tile edge
    lens += [4084 - (k - 1) // 2 - 1, k + 3, 3]  # a boundary inside the last k - 1 starts of tile 3, short documents across its edge
    lens += [int(v) for v in rng.permutation(base * 2)]
    lens += [int(v) for v in rng.integers(0, 40, size=24)]  # fillers
    lens += [4096 - sum(lens) % 4096, 0, 16, 4096 - 16, 1]  # a boundary exactly on a tile edge, an empty document on it
    return lens


def edge_case(rng, k, low=0, high=200000):
    lens = edge_lengths(rng, k)
    offs = offsets_of(lens)
    return rng.integers(low, high, size=int(offs[-1])).astype(np.int32), offs


def limit_cases(k=5):
    """name -> (ids, offs): the shapes the host statement and the model are held against the truths on."""
    rng = np.random.default_rng(7)
    out = {}
    out["edges"] = edge_case(rng, k)
    out["no_docs"] = (np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64))
    out["no_tokens"] = (np.zeros(0, dtype=np.int32), np.zeros(4, dtype=np.int64))
    offs = offsets_of(rng.integers(1, 4, size=4096))
    out["all_short"] = (rng.integers(0, 200000, size=int(offs[-1])).astype(np.int32), offs)
    offs = offsets_of([700] + [0] * 5000 + [900])
    out["empty_run"] = (rng.integers(0, 200000, size=1600).astype(np.int32), offs)
    offs = offsets_of([0, 0, 33, 4100, 0])
    out["empty_ends"] = (rng.integers(0, 200000, size=4133).astype(np.int32), offs)
    lab = rng.integers(0, 200000, size=5000).astype(np.int32)
    lab[rng.random(5000) < 0.6] = -100
    out["labels"] = (lab, offsets_of([1000, 7, 3993]))
    ids = rng.integers(0, 200000, size=9000).astype(np.int32)
    ids[8000:8600] = ids[100:700]
    out["twins"] = (ids, offsets_of([100, 600, 7300, 600, 400]))
    return out
