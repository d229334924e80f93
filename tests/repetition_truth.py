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
