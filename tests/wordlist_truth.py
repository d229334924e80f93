"""The word-list rule (include/tokendagger_hip.h, td_word_matches*) in plain Python: per document the folded bytes, every bytes.find
position of every entry, the two neighbours.  And the cases at the kernel's seams: 16-byte windows, 1024-byte wavefronts, 4096-byte tiles,
the halo behind a tile, the documents' edges."""
import random

FOLD, ANYWHERE = 1, 2
TILE = 4096


def is_word(c: int) -> bool:
    return c >= 0x80 or chr(c).isalnum() or c == 0x5F


def matches(text, offs, entries, groups=None, flags=FOLD):
    """-> (stats rows [hits, groups, first_hit, hit_bytes] with groups as the signed int64 it is stored as, totals, entry_hits)"""
    groups = groups if groups is not None else [0] * len(entries)
    stats, entry_hits, tot = [], [0] * len(entries), [0, 0, 0, 0]
    for ds, de in zip(offs[:-1], offs[1:]):
        doc = bytes(text[ds:de])
        doc = doc.lower() if flags & FOLD else doc  # (bytes.lower: ASCII only)
        hits, gbits, first, nbytes = 0, 0, -1, 0
        for i, e in enumerate(entries):
            p = doc.find(e)
            while p >= 0:
                q = p + len(e)
                if flags & ANYWHERE or ((p == 0 or not is_word(doc[p - 1])) and (q == len(doc) or not is_word(doc[q]))):
                    hits, gbits, nbytes = hits + 1, gbits | 1 << groups[i], nbytes + len(e)
                    first = p if first < 0 else min(first, p)
                    entry_hits[i] += 1
                p = doc.find(e, p + 1)
        stats.append([hits, gbits - (1 << 64) if gbits >> 63 else gbits, first, nbytes])
        tot = [tot[0] + hits, tot[1] | gbits, tot[2] + (hits > 0), tot[3] + nbytes]
    tot[1] = tot[1] - (1 << 64) if tot[1] >> 63 else tot[1]
    return stats, tot, entry_hits


def same(got, want, what):
    stats, totals, entry_hits = got
    assert [list(map(int, r)) for r in stats] == want[0], (what, "stats")
    assert list(map(int, totals)) == want[1], (what, "totals")
    assert list(map(int, entry_hits)) == want[2], (what, "entry_hits")


def plant(n, items, filler=b"zq. "):
    """n bytes of text no entry occurs in, with every word of items = {position: bytes} put at its position between two spaces"""
    t = bytearray((filler * (n // len(filler) + 1))[:n])
    for pos, word in items.items():
        lo = max(pos - 1, 0)
        t[lo:pos + len(word) + 1] = (b" " if pos else b"") + word + b" "
    return bytes(t[:n])


LONG = b"a-sixty-four-byte-entry-that-reaches-as-far-as-an-entry-may-go!!"
STOP = [b"the", b"be", b"to", b"of", b"and", b"that", b"have", b"with"]


def big_list():
    rnd, seen = random.Random(5), set()
    while len(seen) < 3000:
        seen.add(bytes(rnd.choice(b"abcdefghijklmnopqrstuvwxy") for _ in range(rnd.randrange(4, 11))))
    entries = sorted(seen)
    rnd.shuffle(entries)
    return entries


def one(text):
    return text, [0, len(text)]


def seam_cases():
    """name -> (text, offsets, entries, groups or None, flags)"""
    assert len(LONG) == 64
    c = {}
    for name, pos in (("window", 15), ("wavefront", 1023), ("tile", TILE - 1)):
        c[f"astride a {name} seam"] = (plant(pos + 70, {pos - 1: b"The", pos + 20: b"thethe"}), [0, pos + 70], STOP, None, FOLD)
    c["64 bytes from a tile's last byte"] = (plant(TILE + 80, {TILE - 1: LONG}), [0, TILE + 80], [LONG, b"the"], None, FOLD)
    t = bytearray(plant(2 * TILE + 80, {TILE: LONG, 2 * TILE: LONG}))
    t[2 * TILE - 1] = ord("z")  # the second one's left neighbour, in the tile in front, is a word byte
    c["64 bytes at a tile's first byte"] = (bytes(t), [0, 2 * TILE + 80], [LONG], None, FOLD)
    c["the edge is a boundary"] = (b"over the" + b"re it is, the", [0, 8, 21], STOP, None, FOLD)
    c["inside one document it is not"] = (b"over the" + b"re it is, the", [0, 21], STOP, None, FOLD)
    c["empty documents between"] = (b"over the" + b"re it is, the", [0, 0, 8, 8, 8, 21, 21], STOP, None, FOLD)
    c["completed behind the last document"] = (b"say th" + b"e end of and", [0, 4, 6], STOP, None, FOLD)
    c["a last tile shorter than the halo"] = (plant(TILE + 10, {TILE - 2: b"the", TILE + 7: b"of"})[:TILE + 9], [0, TILE + 9], STOP + [LONG], None, FOLD)
    c["shorter than a window"] = (b"to be", [0, 5], STOP, None, FOLD)
    c["overlapping and nested"] = (*one(b"in new york, new yorker, newyork york"), [b"new york", b"york", b"new"], [1, 2, 3], FOLD)
    c["byte for byte"] = (*one(b"a  b a b 2 girls 1 cup, 2 girls  1 cup"), [b"a b", b"2 girls 1 cup"], [0, 5], FOLD)
    for name, flags in (("folded", FOLD), ("as they are", 0)):
        c[f"upper case {name}"] = (*one(b"THE The tHe the"), [b"the"], None, flags)
    c["beside a multi-byte character"] = ("caféthe theé ’the’  the (the)".encode(), [0, 36], [b"the"], None, FOLD)
    c["a non-ASCII entry"] = (*one("naïve NAïVE NAÏVE naïvely".encode()), ["naïve".encode()], [9], FOLD)
    c["punctuation at an entry's ends"] = (*one(b"c++ c++x xc++ (c++) .net a.net .net! x .net"), [b"c++", b".net"], [0, 1], FOLD)
    words = [b"w%02d" % i for i in range(64)]
    t = b" ".join(words[::3] + words[63:]) + b" w64"
    c["64 groups"] = (t, [0, 50, len(t)], words, list(range(64)), FOLD)
    c["first hit with hits in two tiles"] = (plant(3 * TILE, {5000: b"and", 9000: b"and", 9100: b"of"}), [0, 100, 3 * TILE], STOP, list(range(8)), FOLD)
    han = "毒".encode()
    cjk = bytearray("文".encode() * 1500)
    cjk[TILE - 2:TILE + 1] = han  # (astride the tile seam, and not on the text's own character grid: every byte is a start)
    cjk[300:303] = han
    c["anywhere, CJK"] = (bytes(cjk), [0, 4500], [han, b"the"], [3, 4], ANYWHERE)
    c["dense"] = (b"the " * 2000 + b"The", [0, 3001, 8003], STOP, list(range(8)), FOLD)
    c["forty documents in a tile"] = (b"to be " * 40, list(range(0, 241, 6)), STOP, list(range(8)), FOLD)
    c["a run of punctuation"] = (b"!" * 3000 + b"the" + b"?" * 1200 + b"of", [0, 4205], STOP, None, FOLD)
    big = big_list()
    c["a set above the LDS budget"] = (plant(6000, {10: big[0], 2000: big[1500], TILE - 3: big[-1], 5000: big[0] + b"z"}, b"zzz. "),
                                      [0, 2500, 6000], big, [i % 64 for i in range(3000)], FOLD)
    return c
