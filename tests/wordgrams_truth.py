"""Word n-gram repetition per document (include/tokendagger_hip.h, td_word_ngrams*): the rule in plain Python, with bytes.split, tuples
of words and a Counter per document and n; datatrove's greedy walk for the inequality check; and the small texts the tests share."""
from collections import Counter

import numpy as np

import repetition_truth as rt
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


def truths(text, offs):
    """{groups: truth(text, offs, groups)} for TOP, DUP and both, by two calls of truth(): a column is one group's alone and is
    computed without a look at the other group, the first three belong to both.  (tests/test_limit_cases_model.py holds the merged
    form against truth(TOP | DUP) on all of cases().)"""
    top, dup = truth(text, offs, TOP), truth(text, offs, DUP)
    assert np.array_equal(top[0][:, :3], dup[0][:, :3])
    stats = np.concatenate([top[0][:, :9], dup[0][:, 9:]], axis=1)
    return {TOP: top, DUP: dup, TOP | DUP: (stats, np.concatenate([top[1][:9], dup[1][9:]]))}


# ---- the cases at the scan's, the table's and the grid's limits (tests/test_limit_cases_model.py proves what each one reaches) ------------
GRID_WORDS = 2048 * 256   # WG_MAX_GRID workgroups of 256 lanes: the words one sweep of td_wg_insert, td_wg_count, td_wg_cover takes
DOC_BLOCK = 32            # WG_DOC_BLOCK
STEP_WORDS = (33, 34, 41, 42, 65, 66, 73, 74, 129, 130, 257, 258, 513, 514, 1023, 1024)
PLANT = [b"p%d" % i for i in range(12)]
VOCAB = [b"a", b"b", b"ab", b"ba", "é".encode(), "日本".encode(), b"the", b"of", b"and", b"word", b"gram", b"tile", b"lane", b"x1", b"x2", b"zebra",
         b"quartz", b"a1", b"b2", b"c3", b"delta", b"omega", "λόγος".encode(), b"q", b"r", b"s", b"seven", b"eleven", b"long-ish", b"t,", b"u.", b"(v)"]
SHORT_VOCAB = [bytes([x]) for x in b"abcdefghij"] + [bytes([x, y]) for x in b"kmn" for y in b"opqrstuvwx"]  # 40 words of one and two bytes


def random_words(rng, n, vocab, plant_every=0):
    """n words drawn from vocab; with plant_every, the twelve words of PLANT twice with three words between them, every so many words"""
    w = np.asarray(vocab, dtype=object)[rng.integers(0, len(vocab), size=n)].tolist()
    if plant_every:
        for at in range(plant_every // 2, n - 30, plant_every):
            w[at:at + 12] = PLANT
            w[at + 15:at + 27] = PLANT
    return w


def join_words(rng, words):
    """words with one space between them, now and then an LF or two spaces instead"""
    sep = np.asarray([b" ", b"\n", b"  "], dtype=object)[rng.choice(3, size=len(words), p=[0.9, 0.06, 0.04])].tolist()
    return b"".join(x for pair in zip(words, sep) for x in pair)


def big_text(total, seed):
    """-> (text of `total` bytes, [begin, end) of the stretch of the three long words).  In this order: short words up to the middle of
    tile 0; a word of six tiles and 123 bytes; thirty short words; the same word; the first twelve of the thirty; the word without its
    last byte; the same twelve (a kernel that took it for the whole word would count a third occurrence); short words with the planted
    twelve to the end."""
    rng = np.random.default_rng(seed)
    long = bytes(97 + (i * i + 3 * i) % 23 for i in range(6 * TILE + 123))
    head = join_words(rng, random_words(rng, 400, VOCAB))
    behind = random_words(rng, 30, VOCAB)  # the same twelve words behind all three: the n-grams differ in the long word alone
    near = b" ".join(behind[:12]) + b" "
    parts = [head, long, b" ", join_words(rng, behind), long, b" ", near, long[:-1], b" ", near]
    used = sum(map(len, parts))
    fill = join_words(rng, random_words(rng, (total - used) // 3, VOCAB, plant_every=5000))
    fill = fill[:fill.rindex(b" ", 0, total - used - 8) + 1]
    text = b"".join(parts + [fill, b"z" * (total - used - len(fill))])
    assert len(text) == total and TILE // 4 < len(head) < TILE - 64
    return text, (len(head), used)


def long_list():
    """600 documents; every seventh and the last have 1025 to 1100 words.  -> (text, offsets, the words of each)"""
    rng = np.random.default_rng(41)
    n = np.zeros(600, dtype=np.int64)
    small = rng.integers(0, 4, size=600)
    n[:] = np.where(small == 0, 0, np.where(small == 1, 1, rng.integers(2, 41, size=600)))
    long = [d for d in range(600) if d % 7 == 0] + [599]
    n[long] = rng.integers(1025, 1101, size=len(long))
    k = len(long) // 2  # long[k], long[k + 1]: 1088 words each, behind a multiple of 64 long words; long[k + 2]: 1089
    n[long[k]], n[long[k + 1]], n[long[k + 2]] = 1088, 1088, 1089
    n[long[k - 1]] = 1025 + (-(int(n[long[:k - 1]].sum()) + 1025)) % 64
    parts = [join_words(rng, random_words(rng, int(m), VOCAB, plant_every=300 if m > 1000 else 0)) for m in n]
    return (*docs(*parts), n)


def limit_cases():
    """name -> (text, offsets)"""
    c = {}
    for E in rt.EMPTY_RUNS:  # the word `wx` lies on both sides of the run
        c[f"{E} empty documents inside a word"] = docs(b"r s t u v r s t u v w", *[b""] * E, b"x r s t u v r s t u v")
    rng = np.random.default_rng(12)
    head, tail = (join_words(rng, random_words(rng, 1500, VOCAB, plant_every=200)) for _ in range(2))
    c.update(rt.empty_run_cases(*rt.two_tiles(head, tail, b" ")))
    many = random_words(rng, 440000, SHORT_VOCAB, plant_every=20000)
    c["global stride"] = docs(b"a " * 100000 + join_words(rng, many), join_words(rng, random_words(rng, 2000, VOCAB, plant_every=500)))
    text, offs, _ = long_list()
    c["long list"] = (text, offs)
    step = []
    for i, W in enumerate(STEP_WORDS):  # all words different but the first and the last twelve
        first = [b"f%d.%d" % (i, j) for j in range(12)]
        step.append(b" ".join(first + [b"w%d.%d" % (i, j) for j in range(W - 24)] + first))
    c["LDS table steps"] = docs(*step)
    for n_docs in (31, 32, 33, 65):
        c[f"{n_docs} documents of 2 to 6 words"] = docs(*[join_words(rng, random_words(rng, int(m), VOCAB[:6])) for m in rng.integers(2, 7, size=n_docs)])
    c["64 documents, words in the last alone"] = docs(*[b"", b"one ", b" "] * 21, b"a b a b c a b")
    tie = [b"w%d" % i for i in range(600)]
    for at in (10, 20, 30):
        tie[at:at + 2] = [b"aa", b"bb"]
    for at in (300, 400, 500):
        tie[at:at + 2] = [b"cccc", b"dddd"]
    c["tie-break across lanes"] = docs(b" ".join(tie))
    return c


def big_cases():
    """name -> (text, offsets)"""
    c = {}
    a, keep = big_text(rt.BIG_A, 31)
    c["big A, one document"] = docs(a)
    c["big A, cut"] = rt.cut(a, np.random.default_rng(32), 60, keep)
    b, keep = big_text(rt.BIG_B, 33)
    c["big B, cut"] = rt.cut(b, np.random.default_rng(34), 60, keep)
    return c
