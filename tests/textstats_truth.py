"""Per-document text statistics (include/tokendagger_hip.h, td_text_stats*): the rule in numpy over the per-byte class array of
helpers.Twin.classify (the splitter's classification, the only product code used here), and the cases the CPU model and the GPU tests
share.  Whole documents, whole lines and whole characters are looked at, forwards: nothing here is decomposed the way the kernels are."""
import functools

import numpy as np

import helpers as H

COLS = 21
(BYTES, CHARS, UPPER, LOWER, LETTER_OTHER, MARK, NUMBER, SPACE, NON_ASCII, WORDS, WORDS_ALPHA, WORD_MAX, LINES, LINES_BLANK, LINE_MAX,
 END_TERMINAL, END_ELLIPSIS, START_BULLET, HASHES, ELLIPSES, CURLY) = range(COLS)
LOCAL, RUNS = 1, 2
LOCAL_COLS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 18, 19, 20]
RUNS_COLS = [10, 11, 13, 14, 15, 16, 17]
MAX_COLS = [WORD_MAX, LINE_MAX]
TILE = 4096

C_SP, C_WS, C_CRLF, C_UP, C_LW, C_LB, C_MK, C_NUM = 3, 4, 5, 6, 7, 8, 9, 10
F_CONT = 0x10
TERMINAL = {b".", b"!", b"?", b'"', "”".encode(), "。".encode(), "！".encode(), "？".encode()}
BULLETS = {b"-", b"*", "•".encode(), "‣".encode(), "◦".encode()}
ELLIPSIS = "…".encode()


@functools.lru_cache(maxsize=None)
def twin():
    pat, mr, special = H.llama4()
    return H.Twin(pat, dict(list(mr.items())[:300]), {})


def _runs(mask):
    """-> (starts, ends) of the maximal runs of True in mask"""
    m = np.concatenate([[False], mask, [False]])
    d = np.diff(m.astype(np.int8))
    return np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]


def doc_stats(x: np.ndarray, v: np.ndarray) -> np.ndarray:
    """One document: x its bytes, v their class + F_CONT inside it -> its row."""
    r = np.zeros(COLS, dtype=np.int64)
    n = len(x)
    r[BYTES] = n
    if n == 0:
        return r
    c = v & 0x0F
    start = (v & F_CONT) == 0
    space = np.isin(c, [C_SP, C_WS, C_CRLF])
    letter = np.isin(c, [C_UP, C_LW, C_LB])
    r[CHARS] = start.sum()
    for col, cls in ((UPPER, C_UP), (LOWER, C_LW), (LETTER_OTHER, C_LB), (MARK, C_MK), (NUMBER, C_NUM)):
        r[col] = (start & (c == cls)).sum()
    r[SPACE] = (start & space).sum()
    r[NON_ASCII] = (start & (x >= 0x80)).sum()
    # words: the runs of non-space bytes (a character's bytes share its class)
    ws, we = _runs(~space)
    r[WORDS] = len(ws)
    if len(ws):
        r[WORD_MAX] = (we - ws).max()
        has_letter = np.add.reduceat(letter.astype(np.int64), ws)  # (from a word's start to the next word's: spaces are no letters)
        r[WORDS_ALPHA] = (has_letter > 0).sum()
    # characters
    sp = np.nonzero(start)[0]
    ce = np.concatenate([sp[1:], [n]])
    xb = x.tobytes()
    three = sp[(ce - sp) == 3]
    r[ELLIPSES] = sum(1 for i in three if xb[i:i + 3] == ELLIPSIS)
    ds_, de_ = _runs(x == 0x2E)
    r[ELLIPSES] += ((de_ - ds_) >= 3).sum()
    r[HASHES] = (x == 0x23).sum()
    r[CURLY] = ((x == 0x7B) | (x == 0x7D)).sum()
    # lines
    lf = np.nonzero(x == 0x0A)[0]
    ls = np.concatenate([[0], lf + 1])
    le = np.concatenate([lf, [n]])
    if ls[-1] == n:
        ls, le = ls[:-1], le[:-1]
    r[LINES] = len(ls)
    r[LINE_MAX] = (le - ls).max() if len(ls) else 0
    vp = np.nonzero(~space)[0]
    i0 = np.searchsorted(vp, ls)
    i1 = np.searchsorted(vp, le)
    r[LINES_BLANK] = (i0 == i1).sum()
    for k in np.nonzero(i0 < i1)[0]:
        s = int(ls[k])
        first = int(vp[i0[k]])
        fe = int(ce[np.searchsorted(sp, first, "right") - 1])
        if xb[first:fe] in BULLETS:
            r[START_BULLET] += 1
        q = int(vp[i1[k] - 1])
        j = np.searchsorted(sp, q, "right") - 1
        ch = xb[int(sp[j]):int(ce[j])]
        if ch in TERMINAL:
            r[END_TERMINAL] += 1
        if ch == ELLIPSIS or (ch == b"." and q - 2 >= s and xb[q - 2:q] == b".."):
            r[END_ELLIPSIS] += 1
    return r


def truth(text, offs, groups=LOCAL | RUNS):
    """-> (stats int64[n_docs, 21], totals int64[21])"""
    x = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, dtype=np.uint8)
    offs = np.asarray(offs, dtype=np.int64)
    n_docs = len(offs) - 1
    total = int(offs[-1])
    cls = twin().classify(x[:total].tobytes(), offs)[:total] & 0x1F if total else np.zeros(0, dtype=np.uint8)
    stats = np.zeros((n_docs, COLS), dtype=np.int64)
    for d in range(n_docs):
        a, b = int(offs[d]), int(offs[d + 1])
        if b > a:
            stats[d] = doc_stats(x[a:b], cls[a:b])
    drop = [c for c in range(COLS) if c not in ((LOCAL_COLS if groups & LOCAL else []) + (RUNS_COLS if groups & RUNS else []))]
    stats[:, drop] = 0
    totals = stats.sum(axis=0) if n_docs else np.zeros(COLS, dtype=np.int64)
    for c in MAX_COLS:
        totals[c] = stats[:, c].max() if n_docs else 0
    return stats, totals


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
ALPHABET = [b" ", b"\n", b"\r", b".", b"#", b"{", b"-", "•".encode(), ELLIPSIS, "。".encode(), "”".encode(), b"a", b"A", b"9",
            "é".encode(), "中".encode(), "́".encode(), b"\x80", b"\xe2"]


def dense(rng, n_syms, weights=None):
    """n_syms symbols of the alphabet that makes events dense"""
    idx = rng.choice(len(ALPHABET), size=n_syms, p=weights)
    return b"".join(ALPHABET[i] for i in idx)


def prose(rng, n):
    """about n bytes in which words and lines have the lengths of prose, a tenth of it from the dense alphabet"""
    w = np.ones(len(ALPHABET))
    w[0], w[1], w[11], w[12], w[13] = 40, 3, 160, 10, 8
    out = dense(rng, n, w / w.sum())
    return out[:n]


def cut(rng, n, n_docs):
    """offsets of n_docs documents over n bytes at random positions (empty ones, cuts inside characters)"""
    inner = np.sort(rng.integers(0, n + 1, size=max(n_docs - 1, 0)))
    return np.concatenate([[0], inner, [n]]).astype(np.int64)


def _one(text):
    return text, np.asarray([0, len(text)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def limit_cases(tile=TILE):
    """name -> (text bytes, offsets): the frame's seams at tile size `tile` (a multiple of 16)"""
    rng = np.random.default_rng(23)
    T = tile
    cases = {"no documents": (b"", np.asarray([0], dtype=np.int64))}
    for n in (0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T):
        t = prose(rng, n)
        cases[f"length {n}, one document"] = _one(t)
        cases[f"length {n}, documents"] = (t, cut(rng, n, 1 + n // 40))
    # cross-tile look-back
    cases["a word of three tiles, its letter first"] = _one(b"x" + b"1" * (3 * T) + b" 22\n")
    cases["a word of three tiles without a letter, then a letter"] = _one(b"7" * (3 * T) + b" a")
    line = (b"word " * (T // 2))[:5 * T // 2 - 1] + b"."
    cases["a long line, spaces, LF"] = _one(b"ab\n" + line + b" " * 5000 + b"\nnext line.\n")
    for k in range(3):  # the three dots astride a window seam and a tile seam
        pad = (b"word " * T)[:2 * T - 3 - 1 + k]
        cases[f"three dots astride the seam +{k}"] = _one(b"\n" + pad + b"..." + b" " * 5000 + b"\n" + b"tail")
        padw = (b"word " * T)[:32 - 3 + k]
        cases[f"three dots astride a window seam +{k}"] = _one(b"\n" + padw + b"... \n....\n.. .\n")
    cases["a bullet behind spaces"] = _one(b"x\n" + b" " * 4100 + "• item\n".encode() + b" " * 4100 + b"- item\n" + b"\t* item")
    cases["a final line with no LF"] = _one(b"one.\ntwo!\nthree?")
    cases["only LFs"] = _one(b"\n" * 37)
    cases["only LFs, two tiles"] = _one(b"\n" * (2 * T + 5))
    cases["only spaces, two tiles"] = _one(b" " * (2 * T + 5))
    # clipping at document starts
    t = b"some words end here." + b"123\nnext" + b"x."
    cases["nothing leaks into the next document"] = (t, np.asarray([0, 20, 28, 30], dtype=np.int64))
    t = (b"word " * T)[:T - 2] + b"a." + b"123\n" + b" tail"
    cases["nothing leaks, at a tile seam"] = (t, np.asarray([0, T, T + 4, len(t)], dtype=np.int64))
    t = b"a b\n.c\xe2\x80\xa6#{}-\n\n  " + b"q" * 4
    offs = np.asarray([0] * 8 + list(range(17)) + [16] * 10 + [len(t)] * 8, dtype=np.int64)
    assert len(offs) - 1 >= 40
    cases["forty documents inside one window"] = (t, offs)
    t = "ab…cd中。\n” x".encode()
    for k in range(1, len(t)):
        cases[f"a boundary at byte {k} of characters"] = (t, np.asarray([0, k, len(t)], dtype=np.int64))
    t = prose(rng, 3 * T + 100)
    mid = 2 * T + 7
    cases["runs of empty documents"] = (t, np.asarray([0] * 10000 + [mid] * 10001 + [len(t)] * 10001, dtype=np.int64))
    cases["bytes behind the last document"] = (prose(rng, 300), np.asarray([0, 100, 257], dtype=np.int64))
    return cases


@functools.lru_cache(maxsize=None)
def big_case():
    """about 1.2 MiB: more tiles than one sweep of the prefix kernel's workgroup covers (1024) would need 4 MiB; this has 300 tiles,
    documents of every size, and the same text as ONE document"""
    rng = np.random.default_rng(24)
    n = 1200 * 1024 + 77
    t = prose(rng, n)
    return t, cut(rng, n, 700)


def random_small(seed, count):
    """`count` random small texts from the dense alphabet, with random document boundaries"""
    rng = np.random.default_rng(seed)
    for _ in range(count):
        t = dense(rng, int(rng.integers(0, 60)))
        nd = int(rng.integers(1, 8))
        offs = cut(rng, len(t), nd)
        if rng.integers(0, 4) == 0:  # a run of empty documents
            at = int(rng.integers(0, len(offs)))
            offs = np.concatenate([offs[:at], np.full(int(rng.integers(1, 5)), offs[at]), offs[at:]])
        yield t, offs
