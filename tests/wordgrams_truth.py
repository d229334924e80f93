"""Word n-gram repetition per document (include/tokendagger_hip.h, td_word_ngrams*): the rule in plain Python, with bytes.split, tuples
of words and a Counter per document and n; datatrove's greedy walk for the inequality check; and the small texts the tests share."""
from collections import Counter

import numpy as np

from repetition_truth import docs, thue_morse

COLS, TOP, DUP, NO_LDS = 15, 1, 2, 1
LDS_WORDS = 1024  # WG_LDS_WORDS (td_wordgrams_args.h)
TILE = 4096


def chars(b: bytes) -> int:
    return sum(1 for x in b if x & 0xC0 != 0x80)


def truth(text, offs, groups=TOP | DUP):
    """-> (stats int64[n_docs, 15], totals int64[15])"""
    text = bytes(text)
    stats = np.zeros((len(offs) - 1, COLS), dtype=np.int64)
    for d in range(len(offs) - 1):
        doc = text[offs[d]:offs[d + 1]]
        words = doc.split()
        wc = [chars(w) for w in words]
        stats[d, :3] = len(words), sum(wc), chars(doc)
        for n in range(2, 11):
            if not groups & (TOP if n <= 4 else DUP) or len(words) < n:
                continue
            grams = [tuple(words[i:i + n]) for i in range(len(words) - n + 1)]
            count = Counter(grams)
            if n <= 4:
                stats[d, 3 + 2 * (n - 2):5 + 2 * (n - 2)] = max((c, sum(map(chars, g))) for g, c in count.items())
            else:
                inside = {i + j for i, g in enumerate(grams) if count[g] >= 2 for j in range(n)}
                stats[d, 9 + n - 5] = sum(wc[j] for j in inside)
    totals = stats.sum(axis=0)
    totals[3:9] = stats[:, 3:9].max(axis=0, initial=0)
    return stats, totals


def greedy_dup_chars(words, n):
    """datatrove's find_all_duplicate: a serial walk that skips n words after an n-gram it has seen"""
    seen, total, i = set(), 0, 0
    while i < len(words) - n + 1:
        g = tuple(words[i:i + n])
        if g in seen:
            total += sum(map(chars, g))
            i += n
        else:
            seen.add(g)
            i += 1
    return total


def random_case(seed, n=None, n_cuts=None):
    """a text over {a, b, ab, space, LF, é} cut into documents at random bytes"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(0, 200)) if n is None else n
    n_cuts = int(rng.integers(0, 6)) if n_cuts is None else n_cuts
    text = b"".join([b"a", b"b", b"ab", b" ", b"\n", "é".encode()][i] for i in rng.choice(6, size=n, p=[0.2, 0.15, 0.1, 0.35, 0.1, 0.1]))
    cuts = np.sort(rng.integers(0, len(text) + 1, size=n_cuts))
    return text, np.concatenate([[0], cuts, [len(text)]]).astype(np.int64)


def words_doc(n_words, start=0):
    """n_words different words with a stretch of twelve repeated across the middle"""
    w = [b"w%d" % (start + i) for i in range(n_words)]
    mid = n_words // 2
    w[mid:mid + 12] = w[mid - 12:mid]
    return b" ".join(w)


def cases():
    """name -> (text, offsets)"""
    c = {}
    c["the rule's examples"] = docs(b"x y x  y x\ny", b"", b" \t\n\r\x0b\x0c", b"a a a", b"one", b"a\xc2\xa0b a\xe3\x80\x80b", b" lead trail ", b"p, q. p, q.")
    for n in (1, 15, 16, 17):
        u, v = bytes(65 + i for i in range(n)), bytes(66 + i for i in range(n))
        c[f"word length {n}"] = docs(b" ".join([u, v] * 6) + b" " + u + b"x " + v, u + b" " + u)
    for edge in (16, 1024, 4096):  # the second copy of `straddle!!` lies astride byte `edge`
        c[f"a word astride byte {edge}"] = docs(b"straddle!! q r s t u " + b"f" * (edge - 27) + b" straddle!! q r s t u v")
    long = bytes(97 + (i * i) % 23 for i in range(9000))
    c["a word of three tiles"] = docs(long + b" x " + long + b" x " + long[:-1] + b" x")
    c["mixed separators"] = docs(b"a b c d e f\na\tb  c \r\n d\x0be\x0cf g")
    for n in (2, 4, 5, 10):
        c[f"documents of 0 to {n + 1} words"] = docs(b"", b"  \n ", *[b" ".join([b"k"] * m) for m in (1, n - 1, n, n + 1)])
    c["a document boundary inside a word"] = (b"abab ab abab ab", np.asarray([0, 2, 10, 15], dtype=np.int64))
    five = b"r s t u v"
    c["a document boundary inside a duplicate"] = (five + b" " + five, np.asarray([0, 7, 19], dtype=np.int64))
    c["overlapping occurrences"] = docs(b" ".join([b"a"] * 12))
    c["equal counts, different chars"] = docs(b"aa bb x aa bb y cccc d z cccc d", b"cccc d z cccc d aa bb x aa bb")
    c["a 5-gram twice"] = docs(five + b" gap " + five, five + b" " + five, b"r s r s r s r", five + b" gap " + five + b" " + five)
    ten = b"a1 a2 a3 a4 a5 a6 a7 a8 a9 a10"
    c["a 10-gram in two documents and in one"] = docs(ten, ten, ten + b" " + ten)
    c["multi-byte characters"] = docs("é è é è é λόγος 日本 λόγος 日本 語".encode(), "日本 語 日本 語 日本 語".encode())
    c["3000 one-word documents"] = (b"ab " * 3000, np.arange(0, 9001, 3, dtype=np.int64))
    for w in (LDS_WORDS - 1, LDS_WORDS, LDS_WORDS + 1):
        c[f"a document of {w} words"] = docs(words_doc(w), words_doc(40, 5000))
    tm, inv = thue_morse(2048), thue_morse(2048, 1)  # (two words that collide under the word hash)
    c["Thue-Morse and its complement"] = docs(tm + b" x " + inv + b" x")
    c["Thue-Morse, its complement and a copy"] = docs(tm + b" x " + inv + b" x " + tm + b" x")
    c["many documents a tile, many tiles"] = random_case(5, 3 * TILE + 77, 400)
    c["few documents, many tiles"] = random_case(6, 3 * TILE + 77, 3)
    for seed in range(6):
        c[f"random {seed}"] = random_case(100 + seed)
    return c
