"""Duplicate lines and paragraphs per document (include/tokendagger_hip.h, td_repetition*): the rule in plain Python, with bytes.split,
a set per document and exact bytes, and the small texts the tests share."""
import numpy as np

COLS, LINES, PARAS = 12, 1, 2
TILE = 4096


def units(doc: bytes, kind: int):
    if kind == 0:
        return [u for u in doc.split(b"\n") if u]
    return [u.strip(b"\n") for u in doc.split(b"\n\n") if u.strip(b"\n")]


def truth(text, offs, groups=LINES | PARAS):
    """-> (stats int64[n_docs, 12], totals int64[12])"""
    text = bytes(text)
    stats = np.zeros((len(offs) - 1, COLS), dtype=np.int64)
    for d in range(len(offs) - 1):
        for kind in (0, 1):
            if not groups & (1 << kind):
                continue
            seen = set()
            for u in units(text[offs[d]:offs[d + 1]], kind):
                v = np.asarray([1, len(u), sum(1 for x in u if x & 0xC0 != 0x80)])
                stats[d, 6 * kind:6 * kind + 3] += v
                if u in seen:
                    stats[d, 6 * kind + 3:6 * kind + 6] += v
                seen.add(u)
    return stats, stats.sum(axis=0)


def docs(*parts):
    """documents -> (text, offsets)"""
    return b"".join(parts), np.cumsum([0] + [len(p) for p in parts]).astype(np.int64)


def thue_morse(n, flip=0):
    return bytes(ord("a") + ((bin(i).count("1") + flip) & 1) for i in range(n))


def random_case(seed, n=None, n_cuts=None):
    """a text over {a, b, LF, é} cut into documents at random bytes"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(0, 200)) if n is None else n
    n_cuts = int(rng.integers(0, 6)) if n_cuts is None else n_cuts
    text = b"".join([b"a", b"b", b"\n", "é".encode()][i] for i in rng.choice(4, size=n, p=[0.3, 0.2, 0.35, 0.15]))
    cuts = np.sort(rng.integers(0, len(text) + 1, size=n_cuts))
    return text, np.concatenate([[0], cuts, [len(text)]]).astype(np.int64)


def cases():
    """name -> (text, offsets)"""
    c = {}
    c["the rule's examples"] = docs(b"a\n\nb\n", b"", b"\n\n", b"a\nb\n\n\nc\n", b"\na", b"a\n\n\nb", b"\nx\n", b"\n", b"x", b"a\r\na\na \na")
    for n in (1, 15, 16, 17):
        u = bytes(65 + i for i in range(n))
        c[f"unit length {n}"] = docs(u + b"\n" + u + b"\n\n" + u + b"x\n" + u, u + b"\n\n" + u + b"\n\n\n" + u)
    for edge in (16, 1024, 4096):  # the second copy lies astride byte `edge`
        c[f"a copy astride byte {edge}"] = docs(b"straddle!!\n" + b"f" * (edge - 17) + b"\nstraddle!!\n\nstraddle!!\ng")
    long = bytes(97 + (i * i) % 23 for i in range(9000))
    c["a line of three tiles, twice"] = docs(long + b"\n" + long + b"\n\n" + long[:-1] + b"\n")
    c["the two copies in two documents"] = docs(long + b"\n", long + b"\n")
    c["a document boundary inside a line"] = (b"abcabc\nabc" + b"ab\nab", np.asarray([0, 3, 6, 12, 15], dtype=np.int64))
    c["empty and LF-only documents"] = docs(b"", b"", b"\n", b"q\nq", b"", b"\n\n\n", b"q\n\nq\n", b"")
    c["a paragraph behind different LF runs"] = docs(b"p1\nx\n\np1\nx\n\n\n\np1\nx\n\n\np1\ny")
    c["multi-byte characters"] = docs("é\né\nè\n\nλόγος\n\nλόγος".encode(), "日本\n日本語\n日本".encode())
    c["3000 one-byte documents"] = (bytes(b"a\n"[i % 3 == 2] for i in range(3000)), np.arange(3001, dtype=np.int64))
    tm, inv = thue_morse(2048), thue_morse(2048, 1)
    c["Thue-Morse and its complement"] = docs(tm + b"\n" + inv + b"\n")
    c["Thue-Morse, its complement and a copy"] = docs(tm + b"\n" + inv + b"\n" + tm)
    c["many documents a tile, many tiles"] = random_case(5, 3 * TILE + 77, 400)
    for seed in range(6):
        c[f"random {seed}"] = random_case(100 + seed)
    return c


# ---- the cases at the scan's, the table's and the grid's limits (tests/test_limit_cases_model.py proves what each one reaches) ------------
LDS_DOCS = 4352           # td::RC_LDS_DOCS: a tile's table of documents fits LDS below this many entries
PREFIX_LANES = 256        # lanes of td_rp_prefix: ceil(tiles / 256) consecutive tiles a lane
SHIFTS = (0, 1, 15)       # the text pointer's distance from the 16-byte grid in the device tests
EMPTY_RUNS = tuple(range(4344, 4357)) + (5000,)
BIG_A, BIG_B = 256 * TILE, 513 * TILE - 15  # (B: 513 tiles at every shift of SHIFTS)


def tiles(total, shift):
    """what rp_tiles (td_repetition_scan.h) counts"""
    return (total + shift + TILE - 1) // TILE if total > 0 else 0


def tile_tables(offs, shift):
    """rw_table (td_rewrite_common.h) for every tile of the text at a pointer `shift` bytes off the 16-byte grid ->
    [(t0, s1, kb, nk, lds)]: the tile's first and end byte, the last document that starts in front of t0 (t0 == 0: the first), the
    entries of doc_off from kb on whose value lies below s1 (tile_table's return value: the sentinel behind the last document is an
    entry, and never below s1), and whether they fit: tile_table fills RC_LDS_DOCS entries 256 a step and fits iff a step holds
    fewer than 256 entries below s1, that is iff nk < RC_LDS_DOCS.  The fallback's nk is the same number, found by a search."""
    offs = np.asarray(offs, dtype=np.int64)
    n_docs, total = len(offs) - 1, int(offs[-1])
    out = []
    for t in range(tiles(total, shift)):
        t0, s1 = max(t * TILE - shift, 0), min((t + 1) * TILE - shift, total)
        kb = int(np.searchsorted(offs[:n_docs], t0 - 1, "right")) - 1 if t0 > 0 else 0
        nk = int(np.searchsorted(offs, s1, "left")) - kb
        assert nk == int(np.searchsorted(offs[:n_docs], s1 - 1, "right")) - 1 - kb + 1
        out.append((t0, s1, kb, nk, nk < LDS_DOCS))
    return out


def doc_of_model(offs, table, x):
    """rw_doc_of for byte x of the tile `table` describes: the bisection over the LDS table's clamped entries where it fits, over
    doc_off itself where it does not"""
    t0, s1, kb, nk, lds = table
    assert t0 <= x < s1
    lo, hi, r = 0, nk, x - t0
    while lo < hi:
        mid = (lo + hi) >> 1
        rel = int(offs[kb + mid]) - t0
        if lds:
            rel = min(max(rel, -8), TILE + 8)  # RW_OFF_LO, RW_OFF_HI
        if rel > r:
            hi = mid
        else:
            lo = mid + 1
    return kb + lo - 1


def cut(text, rng, n_cuts, keep=(0, 0), n_empty=6):
    """text cut into documents at n_cuts random bytes outside [keep[0], keep[1]), n_empty of the cuts taken twice (empty documents)"""
    c = rng.integers(0, len(text) + 1, size=n_cuts)
    c = c[(c <= keep[0]) | (c >= keep[1])]
    c = np.sort(np.concatenate([c, c[rng.integers(0, len(c), size=n_empty)]]))
    return text, np.concatenate([[0], c, [len(text)]]).astype(np.int64)


def with_empty_run(text, at, n_empty):
    """text as two documents cut at byte `at` with n_empty empty documents between them"""
    return text, np.asarray([0] + [at] * (n_empty + 1) + [len(text)], dtype=np.int64)


def empty_run_cases(text, inside):
    """The geometry both passes share.  text: a little over two tiles, with one unit across the bytes TILE - 16 .. TILE + 1 (the tile
    edge at every shift of SHIFTS lies inside it); inside: a byte of tile 0 inside a unit of text."""
    c = {}
    total = len(text)
    assert 2 * TILE + 15 < total < 2 * TILE + 1024 and 16 < inside < TILE - 16
    c["10 000 empty documents at byte 0"] = with_empty_run(text, 0, 10000)
    c["10 000 empty documents mid-tile inside a unit"] = with_empty_run(text, inside, 10000)
    for s in SHIFTS:
        c[f"10 000 empty documents on the tile edge of shift {s}"] = with_empty_run(text, TILE - s, 10000)
    c["10 000 empty documents at the text's end"] = with_empty_run(text, total, 10000)
    c["nothing but empty documents, no bytes"] = (b"", np.zeros(5001, dtype=np.int64))
    c["nothing but empty documents, some bytes"] = (text[:100], np.zeros(5001, dtype=np.int64))
    return c


def two_tiles(head, tail, sep):
    """-> (a text of a little over two tiles: head up to its last sep in front of byte TILE - 40, one unit of `a` up to byte TILE + 1,
    tail up to its last sep; a byte of tile 0 that has no sep on either side)"""
    head = head[:head.rindex(sep, 0, TILE - 40) + 1]
    text = head + b"a" * (TILE + 2 - len(head)) + sep + tail
    text = text[:text.rindex(sep, 0, 2 * TILE + 500) + 1]
    inside = 1500
    while text[inside - 1] in b" \n" or text[inside] in b" \n":
        inside += 1
    return text, inside


def _units(rng, n_bytes):
    """about n_bytes of random lines over {a, b, é, 日}, one to six characters, behind one LF (three in four) or two"""
    n = n_bytes // 5 + 8
    sym = np.asarray([b"a", b"b", "é".encode(), "日".encode()], dtype=object)
    k = rng.integers(1, 7, size=n)
    s = sym[rng.choice(4, size=int(k.sum()), p=[0.4, 0.3, 0.2, 0.1])]
    out, at = [], 0
    for kk, two in zip(k.tolist(), (rng.random(n) < 0.25).tolist()):
        out.extend(s[at:at + kk])
        out.append(b"\n\n" if two else b"\n")
        at += kk
    return b"".join(out)


def big_text(total, seed):
    """-> (text of `total` bytes, [begin, end) of the stretch of the three long lines).  In this order: short lines up to the middle of
    tile 0; a line of six tiles and 123 bytes, which is a paragraph too; short lines; the same line; short lines; the line without
    its last byte; short lines to the end."""
    rng = np.random.default_rng(seed)
    long = bytes(97 + (i * i + 3 * i) % 23 for i in range(6 * TILE + 123))
    head, gap = _units(rng, 2000), _units(rng, 3000)
    parts = [head, b"\n", long, b"\n\n", gap, b"\n", long, b"\n\n", gap[:1777], b"\n", long[:-1], b"\n\n"]
    used = sum(map(len, parts))
    fill = _units(rng, total - used + 64)[:total - used]
    text = b"".join(parts + [fill])
    assert len(text) == total and TILE // 4 < len(head) < TILE - 64
    return text, (len(head) + 1, used)


def limit_cases():
    """name -> (text, offsets)"""
    c = {}
    for E in EMPTY_RUNS:  # the line `cd` lies on both sides of the run
        c[f"{E} empty documents inside a line"] = docs(b"ab\nab\n\ncd", *[b""] * E, b"cd\nab\n\nab\ncd")
    rng = np.random.default_rng(11)
    c.update(empty_run_cases(*two_tiles(_units(rng, TILE), _units(rng, TILE + 600), b"\n")))
    five = b"alpha\nbeta\n\ngamma\ndelta\nepsilon\n"
    c["2000 documents of the same five lines"] = docs(*[five] * 2000)
    c["the same five lines 2000 times in one document"] = docs(five * 2000)
    c["100 000 copies of one line"] = docs(b"ab\n" * 100000)
    return c


def big_cases():
    """name -> (text, offsets)"""
    c = {}
    a, keep = big_text(BIG_A, 21)
    c["big A, one document"] = docs(a)
    c["big A, cut"] = cut(a, np.random.default_rng(22), 60, keep)
    b, keep = big_text(BIG_B, 23)
    c["big B, cut"] = cut(b, np.random.default_rng(24), 60, keep)
    return c
