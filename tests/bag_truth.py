"""The bag-model rule (include/tokendagger_hip.h, td_bag_classify*) in plain Python + numpy float64: no tables, no code shared with the
library.  make_model draws weights that are multiples of 2^-6 in [-2, 2]: a sum of up to 2^17 such rows is exact in fp32 in any order,
so stats and hidden are compared for EQUALITY.  The probabilities' tolerance is derived here from the reference's own values (rel_tol)."""
import random

import numpy as np

DELIMS = b" \n\r\t\x0b\x0c\x00"
SOFTMAX, OVA, HS = 0, 1, 2
EOS = b"</s>"
U = 2.0 ** -24      # fp32's unit roundoff
FLOOR = 2.0 ** -125  # below fp32's normal range a probability has no relative precision


def fnv(bs, h=2166136261):
    for c in bs:
        h = ((h ^ (c - 256 if c >= 128 else c)) * 16777619) & 0xFFFFFFFF
    return h


def sext(h):  # the int32 hash as uint64
    return (h - (1 << 32) if h >= 1 << 31 else h) & 0xFFFFFFFFFFFFFFFF


def tokens(doc):
    out, cur = [], bytearray()
    for c in doc:
        if c in DELIMS:
            if cur:
                out.append(bytes(cur))
            cur = bytearray()
        else:
            cur.append(c)
    return out + ([bytes(cur)] if cur else [])


def char_rows(tok, m):
    s, rows = b"<" + tok + b">", []
    for i in range(len(s)):
        if s[i] & 0xC0 == 0x80:
            continue
        j, n = i, 1
        while j < len(s) and n <= m["maxn"]:
            j += 1
            while j < len(s) and s[j] & 0xC0 == 0x80:
                j += 1
            if n >= m["minn"] and not (n == 1 and (i == 0 or j == len(s))):
                rows.append(len(m["words"]) + fnv(s[i:j]) % m["bucket"])
            n += 1
    return rows


def doc_rows(doc, m, eos):
    """-> (rows, [tokens, in_vocab, features, long])"""
    index = m["index"]
    rows, H, in_vocab, n_long = [], [], 0, 0
    for tok in tokens(doc):
        if len(tok) > 1024:
            n_long += 1
            continue
        H.append(fnv(tok))
        if tok in index:
            rows.append(index[tok])
            in_vocab += 1
        if m["maxn"] > 0 and tok != EOS:
            rows += char_rows(tok, m)
    if eos:
        H.append(fnv(EOS))
        if EOS in index:
            rows.append(index[EOS])
            in_vocab += 1
    for i in range(len(H)):
        h = sext(H[i])
        for j in range(i + 1, min(len(H), i + m["word_ngrams"])):
            h = (h * 116049371 + sext(H[j])) & 0xFFFFFFFFFFFFFFFF
            rows.append(len(m["words"]) + h % m["bucket"])
    return rows, [len(H), in_vocab, len(rows), n_long]


def tree(counts):
    """fastText's buildTree -> per label (path, code), leaf to root"""
    L = len(counts)
    parent, binary, count = [-1] * (2 * L - 1), [False] * (2 * L - 1), list(counts) + [10 ** 15] * (L - 1)
    leaf, node = L - 1, L
    for i in range(L, 2 * L - 1):
        mini = []
        for _ in range(2):
            if leaf >= 0 and count[leaf] < count[node]:
                mini.append(leaf)
                leaf -= 1
            else:
                mini.append(node)
                node += 1
        count[i] = count[mini[0]] + count[mini[1]]
        parent[mini[0]] = parent[mini[1]] = i
        binary[mini[1]] = True
    out = []
    for i in range(L):
        path, code, j = [], [], i
        while parent[j] != -1:
            path.append(parent[j] - L)
            code.append(binary[j])
            j = parent[j]
        out.append((path, code))
    return out


def log_sigmoid(x):
    return np.where(x < 0, x - np.log1p(np.exp(np.minimum(x, 0))), -np.log1p(np.exp(-np.maximum(x, 0))))


def classify(m, text, offs, eos=True):
    """-> dict: stats int64 [n, 4], totals, hidden float32 [n, dim], probs float64 [n, L], best, rel [n]: the relative tolerance of a
    document's probabilities (an fp32 evaluation of the output layer against this one), sure [n]: best is decided beyond it."""
    n, dim, L = len(offs) - 1, m["dim"], m["n_labels"]
    wi, wo = m["input"], m["output"].astype(np.float64)
    stats, hidden, probs = np.zeros((n, 4), np.int64), np.zeros((n, dim), np.float32), np.zeros((n, L))
    best, rel, sure = np.full(n, -1, np.int32), np.zeros(n), np.ones(n, bool)
    paths = tree(m["counts"]) if m["loss"] == HS else None
    for d in range(n):
        rows, stats[d] = doc_rows(bytes(text[offs[d]:offs[d + 1]]), m, eos)
        if not rows:
            continue
        assert len(rows) <= 1 << 17, "the sum would not be exact in fp32"
        hidden[d] = wi[rows].astype(np.float64).sum(axis=0).astype(np.float32) / np.float32(len(rows))
        h = hidden[d].astype(np.float64)
        f = wo @ h
        e = (dim + 2) * U * np.abs(wo * h).sum(axis=1).max()  # an fp32 dot product of dim terms, and hidden's own rounding
        if m["loss"] == SOFTMAX:
            p = np.exp(f - f.max())
            p /= p.sum()
            rel[d] = 4 * e + (f.max() - f.min() + L + 16) * U  # numerator and sum each carry 2e; exp's argument, the sum of L terms, a few ulps
        elif m["loss"] == OVA:
            p = 1 / (1 + np.exp(-f))
            rel[d] = e + (np.abs(f).max() + 16) * U
        else:
            lp, depth, tmax = np.zeros(L), 0, 0.0
            for l, (path, code) in enumerate(paths):
                t = log_sigmoid(np.where(code, f[path], -f[path]))
                lp[l], depth, tmax = t.sum(), max(depth, len(path)), max(tmax, np.abs(t).max())
            p = np.exp(lp)
            # a term errs by e and a few ulps of itself, the sum of depth terms by an ulp of its size a step, exp by its argument's ulp
            rel[d] = depth * (e + 8 * U * (1 + tmax)) + (depth + 1) * U * np.abs(lp).max() + 16 * U
        probs[d], best[d] = p, int(np.argmax(p))
        top = np.sort(p)[-2:]
        sure[d] = top[1] - top[0] > 2 * (rel[d] * top[1] + FLOOR)
    return {"stats": stats, "totals": stats.sum(axis=0), "hidden": hidden, "probs": probs, "best": best, "rel": rel, "sure": sure}


def same(got, want, what):
    """got: best, best_prob, probs, hidden, stats, totals of the library (probs, hidden, totals may be None)"""
    assert np.array_equal(got["stats"], want["stats"]), (what, "stats")
    if got["totals"] is not None:
        assert np.array_equal(got["totals"], want["totals"]), (what, "totals")
    if got["hidden"] is not None:
        assert np.array_equal(got["hidden"], want["hidden"]), (what, "hidden")
    tol = want["rel"][:, None] * want["probs"] + FLOOR
    if got["probs"] is not None:
        assert (np.abs(got["probs"] - want["probs"]) <= tol).all(), (what, "probs", float(np.abs(got["probs"] - want["probs"]).max()))
    empty = want["stats"][:, 2] == 0
    assert (got["best"][empty] == -1).all() and (got["best_prob"][empty] == 0).all(), (what, "empty documents")
    s = want["sure"] & ~empty
    assert np.array_equal(got["best"][s], want["best"][s]), (what, "best")
    rows = np.nonzero(~empty)[0]
    assert (got["best"][rows] >= 0).all() and (got["best"][rows] < want["probs"].shape[1]).all(), (what, "best's range")
    pb = want["probs"][rows, got["best"][rows]]
    assert (np.abs(got["best_prob"][rows] - pb) <= want["rel"][rows] * pb + FLOOR).all(), (what, "best_prob")


def make_model(seed, words, dim, n_labels, loss, bucket, minn=0, maxn=0, word_ngrams=1, counts=None):
    rng = np.random.default_rng(seed)
    draw = lambda r, c: (rng.integers(-128, 129, size=(r, c)) / 64).astype(np.float32)  # noqa: E731
    words = [bytes(w) for w in words]
    return {"words": words, "index": {w: i for i, w in enumerate(words)}, "dim": dim, "n_labels": n_labels, "loss": loss, "bucket": bucket,
            "minn": minn, "maxn": maxn, "word_ngrams": word_ngrams, "counts": counts, "input": draw(len(words) + bucket, dim),
            "output": draw(n_labels - (loss == HS), dim)}


VOCAB = [b"the", b"of", b"and", b"caf\xc3\xa9", b"\x80abc", b"x\xbf", b"na\xc3\xafve", b"a", b"b", b"zeta", b"hello", b"wor"]
# words whose hashes have the top bit set: the word n-grams' sign extension
TOP = [w for w in (b"t%d" % i for i in range(64)) if fnv(w) >> 31][:3]
BIG = [b"w%d" % i for i in range(5000)]


def models():
    skew = sorted((int(1e6 / (i + 1) ** 1.5) + (i % 3 == 0) for i in range(176)), reverse=True)
    return {
        "one": make_model(1, VOCAB + [EOS], 1, 2, SOFTMAX, 0),
        "lid": make_model(2, VOCAB + [EOS], 16, 176, HS, 2000003, 2, 4, 1, skew),
        "ova": make_model(3, VOCAB, 100, 3, OVA, 7, 1, 1, 3),
        "wide": make_model(4, VOCAB + TOP, 256, 1000, SOFTMAX, 7, 0, 0, 2),
        "two rows": make_model(5, VOCAB, 300, 5, SOFTMAX, 11, 2, 4, 5),
        "big dictionary": make_model(6, BIG, 8, 4, SOFTMAX, 1000, 0, 0, 2),
    }


def seam_cases():
    """name -> (text, offsets, the model's name, eos)"""
    rnd = random.Random(7)
    fill = b" ".join(rnd.choice(VOCAB) for _ in range(2000))
    # 0xC3 0xA9 lies across a 16-byte window edge at byte 15 | 16 and across the tile edge of a text 15 bytes off the grid (4080 | 4081);
    # 0xE2 0x82 0xAC lies across the tile edge of a text 1 byte off the grid (4094 | 4095) and on it (4095 | 4096); each inside a token
    edge = b"to " + b"x" * 9 + b"caf\xc3\xa9s " + fill[:4077 - 20] + b" tok\xc3\xa9 hello zetas\xe2\x82\xacuro " + fill[:300]
    assert edge[15:17] == edge[4080:4082] == b"\xc3\xa9" and edge[4094:4097] == b"\xe2\x82\xac" and edge[4089:4100] == b"zetas\xe2\x82\xacuro"
    longs = b"aa " + b"x" * 1023 + b" bb " + b"y" * 1024 + b" cc " + b"z" * 1025 + b" dd " + b"q" * 5000 + b" ee"
    gap = b"one" + b" \n" * 2600 + b"two three the of"
    few = b"a" + b"a b" + b"a b the of and zeta"
    blank = b"  \n" + b"\t" + b"the"
    bytes1 = b"ab c" * 1500
    big = b" ".join(rnd.choice(VOCAB + [b"oov", b"q"]) for _ in range(16600))
    high = b"\x80abc caf\xc3\xa9 \xa9\xa9x\xbf \xff\xfe z\xc3 \xc3 x\xbf \xe2\x82\xac\xe2\x82"
    top = b" ".join([TOP[0], TOP[1], b"the", TOP[2], TOP[0], TOP[0]])
    nul = b"a\x00b\x00\x00the\x0bof\x0cand\ra\tb\nzeta"
    lit = b"x </s> hello </s>"
    bigd = b" ".join(rnd.choice(BIG + [b"oov1", b"w5000"]) for _ in range(3000))
    assert len(big) - 5 >= 65536  # (the long document of "a document of many chunks")
    one = lambda t: (t, [0, len(t)])  # noqa: E731
    return {
        "a token and a character across a window and a tile edge": (*one(edge), "lid", True),
        "tokens of 1023 to 5000 bytes, a bigram across the skipped ones": (*one(longs), "wide", True),
        "long tokens' character n-grams": (*one(longs), "lid", False),
        "a delimiter run longer than a tile, bigrams": (*one(gap), "wide", True),
        "a delimiter run longer than a tile, trigrams": (*one(gap), "ova", False),
        "fewer tokens than N": (few, [0, 1, 4, 4, len(few)], "two rows", True),
        "blank documents, </s> a word": (blank, [0, 0, 3, 3, 4, 4, 7, 7], "one", True),
        "blank documents, </s> a word, no EOS": (blank, [0, 0, 3, 3, 4, 4, 7, 7], "one", False),
        "blank documents, </s> no word": (blank, [0, 0, 3, 3, 4, 4, 7, 7], "ova", True),
        "blank documents, </s> no word, no EOS": (blank, [0, 0, 3, 3, 4, 4, 7, 7], "ova", False),
        "one-byte documents": (bytes1, list(range(len(bytes1) + 1)), "one", True),
        "one-byte documents, bigrams, no EOS": (bytes1, list(range(len(bytes1) + 1)), "wide", False),
        "documents that end inside a token": (b"hello world", [0, 3, 8, 11], "lid", True),
        "a document of many chunks": (b"the of " + big + b" a b", [0, 4, 7, 7 + len(big) - 5, len(big) + 11], "ova", True),
        "a document of many chunks, two rows a lane": (big[:20000], [0, 9, 20000], "two rows", True),
        "bytes above 0x7F and stray continuation bytes": (*one(high), "lid", True),
        "hashes with the top bit set": (top, [0, len(top)], "wide", True),
        "0x00 and the other delimiters": (*one(nul), "two rows", True),
        "a literal </s>, a word": (*one(lit), "lid", True),
        "a literal </s>, no word": (*one(lit), "two rows", True),
        "a dictionary of 5000 words": (bigd, [0, 100, len(bigd) // 2, len(bigd)], "big dictionary", True),
    }
