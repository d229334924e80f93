"""N-gram matches: two independent statements of the contract in include/tokendagger_hip.h ("n-gram matches"), and the inputs the
model test and the GPU test share.

matches_brute   the plain loop over documents, positions and a dict of tuples
matches_numpy   sliding_window_view per length, rows viewed as void and np.isin; cover by a difference array

Both return (cover uint8[total], labels int32 | None, doc_stats int64[n_docs, 2], pattern_counts int64[n_pats], counts int64[4])."""
import numpy as np

TILE = 4096
MAX_LEN = 64
VOCAB = 200000


def matches_brute(seqs, ids, offs, labels=None, ignore=-100, pattern_counts=None):
    ids = [int(x) for x in ids]
    first = {}
    for p, q in enumerate(seqs):
        first.setdefault(tuple(int(x) for x in q), p)
    lengths = sorted({len(k) for k in first})
    n_docs, total = len(offs) - 1, int(offs[-1])
    cover = np.zeros(total, dtype=np.uint8)
    stats = np.zeros((n_docs, 2), dtype=np.int64)
    pc = np.zeros(len(seqs), dtype=np.int64) if pattern_counts is None else pattern_counts.copy()
    for d in range(n_docs):
        a, z = int(offs[d]), int(offs[d + 1])
        for q in range(a, z):
            for k in lengths:
                if q + k > z:
                    break
                p = first.get(tuple(ids[q:q + k]))
                if p is not None:
                    stats[d, 0] += 1
                    pc[p] += 1
                    cover[q:q + k] = 1
        stats[d, 1] = int(cover[a:z].sum())
    lab = None
    if labels is not None:
        lab = np.array(labels, dtype=np.int32, copy=True)
        lab[:total][cover == 1] = ignore
    counts = np.asarray([stats[:, 0].sum(), stats[:, 1].sum(), int((stats[:, 0] > 0).sum()), 0], dtype=np.int64)
    return cover, lab, stats, pc, counts


def _rows_as_void(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a.view(np.dtype((np.void, 4 * a.shape[1]))).reshape(-1)


def matches_numpy(seqs, ids, offs, labels=None, ignore=-100, pattern_counts=None):
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    offs = np.asarray(offs, dtype=np.int64)
    n_docs, total = len(offs) - 1, int(offs[-1])
    pc = np.zeros(len(seqs), dtype=np.int64) if pattern_counts is None else pattern_counts.copy()
    diff = np.zeros(total + 1, dtype=np.int64)
    occ = np.zeros(n_docs, dtype=np.int64)
    lens = np.asarray([len(q) for q in seqs])
    pos = np.arange(total, dtype=np.int64)
    end_of = offs[np.searchsorted(offs, pos, side="right")] if total else pos  # the end of every position's document
    doc_of = np.searchsorted(offs, pos, side="right") - 1
    for k in sorted(set(lens.tolist())):
        if total < k:
            continue
        idx = np.flatnonzero(lens == k)  # ascending: the first of equal rows is the lowest index
        pats = _rows_as_void(np.asarray([seqs[i] for i in idx], dtype=np.int32).reshape(len(idx), k))
        uniq, where = np.unique(pats, return_index=True)
        wins = _rows_as_void(np.lib.stride_tricks.sliding_window_view(ids[:total], k))
        starts = np.flatnonzero(np.isin(wins, uniq) & (pos[:len(wins)] + k <= end_of[:len(wins)]))
        np.add.at(diff, starts, 1)
        np.add.at(diff, starts + k, -1)
        np.add.at(occ, doc_of[starts], 1)
        np.add.at(pc, idx[where[np.searchsorted(uniq, wins[starts])]], 1)
    cover = (np.cumsum(diff[:total]) > 0).astype(np.uint8)
    csum = np.concatenate([[0], np.cumsum(cover, dtype=np.int64)])
    stats = np.stack([occ, csum[offs[1:]] - csum[offs[:-1]]], axis=1).astype(np.int64)
    lab = None
    if labels is not None:
        lab = np.array(labels, dtype=np.int32, copy=True)
        lab[:total][cover == 1] = ignore
    counts = np.asarray([occ.sum(), int(cover.sum()), int((occ > 0).sum()), 0], dtype=np.int64)
    return cover, lab, stats, pc, counts


def same(got, want, what=""):
    names = ("cover", "labels", "doc_stats", "pattern_counts", "counts")
    for g, w, n in zip(got, want, names):
        if g is None or w is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, n, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, n, np.flatnonzero((g != w).reshape(-1))[:8])


# ---- inputs -------------------------------------------------------------------------------------------------------------------------

def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def random_offsets(rng, total, n_docs):
    cuts = np.sort(rng.integers(0, total + 1, size=max(n_docs - 1, 0)))
    return np.concatenate([[0], cuts, [total]]).astype(np.int64)


def dense(rng, total=3 * TILE + 12, n_docs=40, lengths=(2, 3, 5, 8), n_pats=40):
    """ids of 4 values: matches everywhere, overlapping and nested; some documents are empty (equal cuts)."""
    ids = rng.integers(0, 4, size=total).astype(np.int32)
    seqs = [rng.integers(0, 4, size=int(rng.choice(lengths))).tolist() for _ in range(n_pats)]
    return dict(seqs=seqs, ids=ids, offs=random_offsets(rng, total, n_docs))


def junk(rng, n):
    return rng.integers(1000, VOCAB, size=n).astype(np.int32)


def planted(rng, total, offs, seqs, places):
    """ids of the vocabulary's range (no pattern occurs by chance: pattern ids are below 1000) with seqs[p] written at q for (p, q) in places."""
    ids = junk(rng, total)
    for p, q in places:
        ids[q:q + len(seqs[p])] = seqs[p]
    return dict(seqs=seqs, ids=ids, offs=np.asarray(offs, dtype=np.int64))


def pattern(rng, k):
    return rng.integers(0, 1000, size=k).tolist()


def sparse(rng, total=3 * TILE + 12, n_docs=30):
    seqs = [pattern(rng, k) for k in (13, 13, 13, 8, 50, 13, 64, 1)]
    places = [(int(rng.integers(0, len(seqs))), int(q)) for q in rng.integers(0, total - 64, size=60)]
    return planted(rng, total, random_offsets(rng, total, n_docs), seqs, places)


def tile_split(rng, split):
    """A 64-id pattern with `split` ids in front of the tile border 4096 (0: it starts at the border, 64: it ends there), one document."""
    seqs = [pattern(rng, 64)]
    total = TILE + 150
    return planted(rng, total, [0, total], seqs, [(0, TILE - split)])


def tile_border(rng):
    """An occurrence that starts at a tile's last id, one that ends exactly at a tile border, one that starts at a border."""
    seqs = [pattern(rng, 2), pattern(rng, 13)]
    total = 2 * TILE + 30
    return planted(rng, total, [0, 10, total], seqs, [(0, TILE - 1), (1, 2 * TILE - 13), (0, 2 * TILE), (1, TILE + 1)])


def document_edges(rng):
    """Patterns at a document's first and last id; a window equal to a pattern across a document border (no occurrence); a document
    shorter than every pattern; documents that begin and end at tile borders."""
    seqs = [pattern(rng, 5), pattern(rng, 13), pattern(rng, 64)]
    lens = [100, 60, 3, 0, TILE - 163, 64, 13, 5, 0, 0, 2 * TILE, 77]
    offs = offsets_of(lens)
    places = [(0, 0), (0, 95),                       # a document's first and last id
              (1, 154),                              # across the border 160: 6 ids in front of it, the 3-id document and 4 more behind
              (1, TILE - 13),                        # ends with its document, at a tile border
              (2, int(offs[5])), (1, int(offs[6])), (0, int(offs[7])),  # whole documents of 64, 13 and 5 ids
              (0, int(offs[10])),                    # a first id behind empty documents
              (2, 2 * TILE - 30),                    # inside one document, across a tile border
              (1, int(offs[11]) - 20),
              (0, int(offs[11]) - 2),                # across the last border
              (0, int(offs[12]) - 5)]                # the last ids of all
    return planted(rng, int(offs[-1]), offs, seqs, places)


def empty_run(rng, n_empty=4400):
    """More empty documents at one position than the locator's LDS table holds (4352), inside a tile and with matches around them."""
    seqs = [pattern(rng, 4), pattern(rng, 13)]
    lens = [700] + [0] * n_empty + [900, 0, 0, TILE + 9]
    offs = offsets_of(lens)
    places = [(0, 10), (0, 696), (1, 694), (0, 700), (1, 1590), (0, 1598), (0, 1600), (1, int(offs[-1]) - 13)]
    return planted(rng, int(offs[-1]), offs, seqs, places)


def nested(rng):
    """[7,7], [7,7,7] and [7] together over runs of 7: overlapping and nested occurrences all count."""
    seqs = [[7, 7], [7, 7, 7], [7]]
    ids = junk(rng, 2 * TILE + 5)
    for q, n in ((3, 4), (100, 1), (TILE - 2, 5), (TILE + 500, 70), (2 * TILE - 1, 2)):
        ids[q:q + n] = 7
    return dict(seqs=seqs, ids=ids, offs=offsets_of([50, 2 * TILE - 50 + 5]))


def eight_lengths(rng):
    ks = (1, 2, 3, 5, 8, 13, 33, 64)
    seqs = [pattern(rng, k) for k in ks for _ in range(3)]
    total = 3 * TILE + 3
    places = [(int(rng.integers(0, len(seqs))), int(q)) for q in rng.integers(0, total - 64, size=80)]
    return planted(rng, total, random_offsets(rng, total, 25), seqs, places)


def repeats(rng):
    """Equal sequences repeat in the list: one pattern, known by the lowest index."""
    a, b, c = pattern(rng, 6), pattern(rng, 6), pattern(rng, 9)
    seqs = [a, b, a, c, b, a, c]
    total = TILE + 300
    return planted(rng, total, random_offsets(rng, total, 6), seqs, [(0, 5), (1, 50), (3, 200), (0, TILE - 3), (1, TILE + 100), (3, TILE + 200)])


def label_stream(rng):
    """A label-like stream is searched: negative values and the ignore_index itself lie in it and match nothing."""
    c = sparse(rng, total=2 * TILE + 77, n_docs=9)
    ids = c["ids"]
    ids[rng.random(len(ids)) < 0.3] = -100
    ids[5], ids[6], ids[TILE] = -1, -2**31, 2**31 - 1
    return c


def limit_cases(seed=21):
    """name -> case, built once per caller."""
    rng = np.random.default_rng(seed)
    out = {"dense": dense(rng), "sparse": sparse(rng), "document_edges": document_edges(rng), "empty_run": empty_run(rng),
           "nested": nested(rng), "eight_lengths": eight_lengths(rng), "repeats": repeats(rng), "label_stream": label_stream(rng), "tile_border": tile_border(rng)}
    for split in (0, 1, 63, 64):
        out[f"tile_split_{split}"] = tile_split(rng, split)
    one = sparse(rng, total=TILE + 40, n_docs=3)
    out["one_pattern"] = dict(one, seqs=one["seqs"][:1])
    out["no_docs"] = dict(seqs=[[1, 2]], ids=np.zeros(0, dtype=np.int32), offs=np.zeros(1, dtype=np.int64))
    out["no_tokens"] = dict(seqs=[[1, 2]], ids=np.zeros(0, dtype=np.int32), offs=np.zeros(6, dtype=np.int64))
    return out


def forced_collisions(rng):
    """Dense ids and many short patterns: with 1 to 4 tag bits most tag matches are of windows whose ids differ."""
    return dense(rng, total=2 * TILE + 100, n_docs=12, lengths=(3, 6, 9), n_pats=120)
