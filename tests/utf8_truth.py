"""Two plain Python statements of the UTF-8 repair's contract (include/tokendagger_hip.h, td_utf8*) and the limit cases of its kernels:
the interpreter's codec per document, and the unit walker (maximal subparts), which also yields first_bad, n_bad and counts."""
import itertools

import numpy as np

REPLACE, IGNORE = 0, 1
ERRORS = {REPLACE: "replace", IGNORE: "ignore"}
# the bytes at which the rule changes
BOUNDARY = bytes.fromhex("00417F808F909FA0BFC0C1C2DFE0E1ECEDEEEFF0F1F3F4F5FF")
FFFD = b"\xef\xbf\xbd"


def codec(doc: bytes, policy: int) -> bytes:
    return bytes(doc).decode("utf-8", ERRORS[policy]).encode("utf-8")


def unit(doc: bytes, p: int):
    """The unit at doc[p]: (length, well-formed)."""
    b0 = doc[p]
    if b0 < 0x80:
        return 1, True
    if not 0xC2 <= b0 <= 0xF4:
        return 1, False
    need = 2 if b0 < 0xE0 else 3 if b0 < 0xF0 else 4
    lo = {0xE0: 0xA0, 0xF0: 0x90}.get(b0, 0x80)
    hi = {0xED: 0x9F, 0xF4: 0x8F}.get(b0, 0xBF)
    if p + 1 >= len(doc) or not lo <= doc[p + 1] <= hi:
        return 1, False
    n = 2
    while n < need and p + n < len(doc) and 0x80 <= doc[p + n] <= 0xBF:
        n += 1
    return n, n == need


def walk(doc: bytes, policy: int):
    """-> (repaired bytes, first_bad, n_bad, bytes in subparts, begins with a continuation byte, ends in a subpart led by a lead byte)"""
    out, first, bad, sub, p, last = bytearray(), -1, 0, 0, 0, None
    while p < len(doc):
        n, wf = unit(doc, p)
        if wf:
            out += doc[p:p + n]
        else:
            first = p if first < 0 else first
            bad += 1
            sub += n
            if policy == REPLACE:
                out += FFFD
        last = (p, wf)
        p += n
    begins = len(doc) > 0 and 0x80 <= doc[0] <= 0xBF
    ends = last is not None and not last[1] and 0xC2 <= doc[last[0]] <= 0xF4
    return bytes(out), first, bad, sub, int(begins), int(ends)


def starts_by_context(doc: bytes, p: int) -> bool:
    """The fact the kernels rest on: whether p starts a unit, from at most three bytes in front of it."""
    if not 0x80 <= doc[p] <= 0xBF:
        return True
    for j in (1, 2, 3):
        q = p - j
        if q < 0:
            return True
        if 0x80 <= doc[q] <= 0xBF:
            continue
        b0 = doc[q]
        if not 0xC2 <= b0 <= 0xF4:
            return True
        need = 2 if b0 < 0xE0 else 3 if b0 < 0xF0 else 4
        lo = {0xE0: 0xA0, 0xF0: 0x90}.get(b0, 0x80)
        hi = {0xED: 0x9F, 0xF4: 0x8F}.get(b0, 0xBF)
        return not (need > j and lo <= doc[q + 1] <= hi)
    return True


def unit_starts(doc: bytes):
    s, p = [], 0
    while p < len(doc):
        s.append(p)
        p += unit(doc, p)[0]
    return s


def docs_of(text, offs):
    b = bytes(np.asarray(text, dtype=np.uint8))
    return [b[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


def truth(text, offs, policy, by=walk):
    """-> (text, out_offsets, flags, first_bad, n_bad, counts) as td_utf8_host gives them; by=codec_walk: the text from the codec."""
    docs = docs_of(text, offs)
    outs, ooff, flags, first, nbad = [], [0], [], [], []
    c = [0] * 8
    for d in docs:
        o, f, b, sub, begins, ends = by(d, policy)
        outs.append(o)
        ooff.append(ooff[-1] + len(o))
        flags.append(int(b > 0))
        first.append(f)
        nbad.append(b)
        c[1] += b > 0
        c[2] += b
        c[3] += sub
        c[4] += begins
        c[5] += ends
    c[0] = ooff[-1]
    return (np.frombuffer(b"".join(outs), dtype=np.uint8), np.asarray(ooff, dtype=np.int64), np.asarray(flags, dtype=np.uint8),
            np.asarray(first, dtype=np.int64).reshape(-1), np.asarray(nbad, dtype=np.int64).reshape(-1), np.asarray(c, dtype=np.int64))


def codec_walk(doc, policy):
    r = walk(doc, policy)
    return (codec(doc, policy),) + r[1:]


def same(got, want, what):
    for i, part in enumerate(("text", "offsets", "flags", "first_bad", "n_bad", "counts")):
        if got[i] is not None:
            assert np.array_equal(np.asarray(got[i]), np.asarray(want[i])), (what, part, np.asarray(got[i])[:16], np.asarray(want[i])[:16])


def exhaustive(max_len=4):
    for n in range(max_len + 1):
        for t in itertools.product(BOUNDARY, repeat=n):
            yield bytes(t)


def batch(docs):
    offs = np.zeros(len(docs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(d) for d in docs])
    return np.frombuffer(b"".join(docs), dtype=np.uint8).copy(), offs


def filler(n: int, seed: int = 0) -> bytes:
    words = (b"the quick brown fox jumps over the lazy dog. ", b"Pack my box with five dozen liquor jugs!\n", b"0123456789 ")
    base = b"".join(words[(seed + i) % 3] for i in range(3))
    return (base * (n // len(base) + 1))[:n]


def put(buf: bytearray, at: int, piece: bytes):
    buf[at:at + len(piece)] = piece


SEQS = {"two": "é".encode(), "three": "€".encode(), "four": "😀".encode()}
PIECES = dict(SEQS)
PIECES.update({"three cut 1": b"\xe2", "three cut 2": b"\xe2\x82", "four cut 1": b"\xf0", "four cut 2": b"\xf0\x9f", "four cut 3": b"\xf0\x9f\x98",
               "two cut": b"\xc3", "e0 9f": b"\xe0\x9f\x80", "ed a0": b"\xed\xa0\x80", "f0 8f": b"\xf0\x8f\x80\x80", "f4 90": b"\xf4\x90\x80\x80",
               "stray": b"\x80", "strays behind a cut": b"\xe2\x82\x80\x80", "c0": b"\xc0\xaf", "ff": b"\xff", "f5": b"\xf5\x80\x80\x80"})


def limit_cases(tile: int):
    """name -> (text uint8, offsets int64): the smallest shapes at which the windows (16 bytes), the tiles (`tile` bytes), the
    documents' edges and the growth of a tile can go wrong."""
    c = {}
    n = 2 * tile + 200
    seams = (16, 48, tile, 2 * tile)  # a window seam, one more, a tile seam, the next (the check's step seam at these sizes)
    # every piece astride every seam at every split point (0 and len(piece): it touches the seam), one document and three
    for name, piece in PIECES.items():
        for k in range(len(piece) + 1):
            buf = bytearray(filler(n, k))
            for s in seams:
                put(buf, s - k, piece)
            c[f"{name}@{k}"] = (np.frombuffer(bytes(buf), dtype=np.uint8).copy(), np.asarray([0, n], dtype=np.int64))
        buf = bytearray(filler(n))
        for s in seams:
            put(buf, s - 1, piece)
        c[f"{name}, three documents"] = (np.frombuffer(bytes(buf), dtype=np.uint8).copy(), np.asarray([0, 40, tile + 7, n], dtype=np.int64))
    # a document boundary at every position inside a four-byte sequence: alone, at a window seam, at a tile seam; with a run of empty
    # documents at the boundary; with the sequence's last bytes a document of their own
    four = SEQS["four"]
    for j in (1, 2, 3):
        for where, at in (("alone", 100), ("window seam", 32), ("tile seam", tile), ("next tile seam", 2 * tile)):
            buf = bytearray(filler(n, j))
            put(buf, at - j, four)
            text = np.frombuffer(bytes(buf), dtype=np.uint8).copy()
            c[f"boundary in four@{j}, {where}"] = (text, np.asarray([0, at, n], dtype=np.int64))
            c[f"boundary in four@{j}, {where}, empty documents"] = (text, np.asarray([0, at, at, at, at, n], dtype=np.int64))
            c[f"boundary in four@{j}, {where}, one-byte documents"] = (text, np.asarray([0, at, at + 1, at + 2, n], dtype=np.int64))
            c[f"boundary in four@{j}, {where}, cut twice"] = (text, np.asarray([0, at - j + 1, at - j + 3, n], dtype=np.int64))
    # more empty documents at such a boundary than a tile's table of documents holds (4352 entries in LDS: the kernels' other path), in a
    # tile that is walked and in one whose other windows are copies
    for where, at in (("window seam", 32), ("tile seam", tile)):
        buf = bytearray(filler(n, 1))
        put(buf, at - 2, four)
        put(buf, at + 40, SEQS["three"])
        c[f"many empty documents in four@2, {where}"] = (np.frombuffer(bytes(buf), dtype=np.uint8).copy(),
                                                         np.asarray([0] + [at] * 4401 + [at + 41, at + 41, n], dtype=np.int64))
    for name, piece in SEQS.items():  # a boundary inside the shorter ones
        for j in range(1, len(piece)):
            buf = bytearray(filler(n))
            put(buf, tile - j, piece)
            put(buf, 64 - j, piece)
            c[f"boundary in {name}@{j}"] = (np.frombuffer(bytes(buf), dtype=np.uint8).copy(), np.asarray([0, 64, tile, n], dtype=np.int64))
    # documents of 0, 1, 2, 3 bytes of every kind
    small = [b"", b"a", b"\x80", b"\xc3", b"\xc3\xa9", b"\xe2\x82", b"\x80\x80", b"\xe2\x82\xac", b"\xf0\x9f\x98", b"\x9f\x98\x80", b"\xed\xa0\x80",
             b"", b"", b"abc", b"\xf0", b"\x98\x80", b"\xff"]
    c["small documents"] = batch(small * 3)
    c["small documents behind a tile"] = batch([filler(tile - 5)] + small * 2 + [filler(tile + 3)] + small)
    c["begins with continuation bytes, ends in a lead"] = batch([b"\x82\xac" + filler(50), filler(tile), filler(20) + b"\xe2"])
    c["begins with continuation bytes, ends in two"] = batch([b"\x80\x80\x80\x80" + filler(10), filler(7) + b"\xf0\x9f\x98"])
    c["no documents"] = (np.zeros(0, dtype=np.uint8), np.asarray([0], dtype=np.int64))
    c["empty"] = batch([b""])
    c["empty documents"] = batch([b"", b"", b""])
    c["documents at the text's end"] = batch([filler(30) + b"\xe2\x82", b"", b"", b""])
    c["bytes behind the last document"] = (np.frombuffer(filler(40) + b"\xe2\x82" + b"\xac\x80\xff" + filler(20), dtype=np.uint8).copy(),
                                           np.asarray([0, 10, 42], dtype=np.int64))
    for k in range(1, 16):
        c[f"shorter than a window {k}"] = batch([(b"\xe2\x82\xac\x80\xf0\x9f\x98\x80\xc3\xa9\xed\xa0\x80\xe2\x82")[:k]])
    # growth: a tile of stray continuation bytes between clean tiles; with documents inside it
    strays = filler(tile) + b"\x80" * tile + filler(tile + 17)
    c["a tile of strays"] = batch([strays])
    c["a tile of strays, documents"] = (np.frombuffer(strays, dtype=np.uint8).copy(),
                                        np.asarray([0, 5, tile, tile + 1, tile + 1, tile + tile // 2, 2 * tile + 3, len(strays)], dtype=np.int64))
    c["strays alone"] = batch([b"\x80" * (tile + 33)])
    # whole clean tiles (the cooperative copy) next to one bad byte
    buf = bytearray(filler(4 * tile))
    buf[2 * tile + 77] = 0xFF
    c["clean tiles next to one bad byte"] = batch([bytes(buf)])
    c["clean tiles next to one bad byte, documents"] = (np.frombuffer(bytes(buf), dtype=np.uint8).copy(),
                                                        np.asarray([0, tile // 2, tile + 5, 3 * tile, 4 * tile], dtype=np.int64))
    # tiles of one kind of sequence
    c["all ascii"] = batch([filler(3 * tile)])
    for name, piece in SEQS.items():
        reps = 3 * tile // len(piece) + 5
        c[f"all {name}"] = batch([piece * reps])
        c[f"all {name}, documents"] = (np.frombuffer(piece * reps, dtype=np.uint8).copy(),
                                       np.asarray([0, len(piece) * 7, tile, tile + 1, 2 * tile + 2, len(piece) * reps], dtype=np.int64))
        c[f"all {name}, one cut"] = batch([piece * (tile // len(piece)) + piece[:-1] + piece * reps])
    mixed = ("naïve café — Привет, мир! 日本語のテキスト 😀 हिन्दी " * (2 * tile // 60 + 2)).encode()
    c["mixed scripts"] = batch([mixed])
    c["mixed scripts, cut every 1000"] = (np.frombuffer(mixed, dtype=np.uint8).copy(),
                                          np.asarray(list(range(0, len(mixed), 1000)) + [len(mixed)], dtype=np.int64))
    c["mixed scripts, cut every 7"] = (np.frombuffer(mixed[:tile + 100], dtype=np.uint8).copy(),
                                       np.asarray(list(range(0, tile + 100, 7)) + [tile + 100], dtype=np.int64))
    rng = np.random.default_rng(8)
    pool = np.frombuffer(BOUNDARY, dtype=np.uint8)
    noise = pool[rng.integers(0, len(pool), size=2 * tile + 31)]
    c["noise"] = (noise.copy(), np.asarray([0, len(noise)], dtype=np.int64))
    cuts = np.unique(rng.integers(0, len(noise), size=300))
    c["noise, documents"] = (noise.copy(), np.asarray([0] + cuts.tolist() + [len(noise)], dtype=np.int64))
    return c


# ---- the check's multi-load loop ------------------------------------------------------------------------------------------------------------
CHECK_MAX_GRID, CHECK_LOADS, THREADS = 2048, 4, 256


def check_loop_geometry(n: int, shift: int):
    """td_utf8_check as launch_utf8_check launches it on n bytes whose base lies `shift` bytes off the 16-byte grid -> (step in windows,
    the full rounds of four loads lane 256 makes)."""
    grid = min(max((n + 16 + CHECK_LOADS * 16 * THREADS - 1) // (CHECK_LOADS * 16 * THREADS), 1), CHECK_MAX_GRID)
    step = grid * THREADS
    g, rounds = THREADS, 0
    while g * 16 - shift >= 4 and (g + 3 * step) * 16 - shift + 20 <= n:
        rounds += 1
        g += 4 * step
    return step, rounds


def dense(n: int) -> bytes:
    """n bytes of text in which every window holds two-, three- and four-byte sequences (cut where n falls)."""
    base = "naïve café — Привет, мир! 日本語のテキスト 😀😁 हिन्दी ελληνικά 한국어 ".encode()
    return (base * (n // len(base) + 1))[:n]


# every piece at every split point: (piece, the bytes of it in front of the seam)
COMBOS = [(piece, k) for piece in PIECES.values() for k in range(len(piece) + 1)]


def check_loop_case(n: int, shift: int, fill=filler):
    """`fill` (ASCII filler, or dense: no window without a byte >= 0x80) with EVERY piece at EVERY split point astride a window seam behind
    every load of the check's loop: behind window q * step + 256 (lane 256's q-th load; lane 0's first window has no four bytes of the
    text in front of it, so it never enters the four-load loop) combination j lies astride the seam of window q * step + 264 + 8 j, so all
    of them are loaded by lanes that are in the four-load loop, as their first, second, third and fourth load and in every round.  The
    combinations are rotated by `shift`.  Document boundaries: at every region's start, ON the seam of every other combination (it cuts
    the piece there), and around a stretch of fill alone -> (text, offsets, the regions' starts)."""
    step, rounds = check_loop_geometry(n, shift)
    buf = bytearray(fill(n))
    span = 16 * 8 * (len(COMBOS) + 1)
    regions = [s for s in ((q * step + THREADS) * 16 - shift for q in range(4 * max(rounds, 1) + 1)) if 100 < s and s + span + 2400 < n]
    bounds = [0]
    for s in regions:
        bounds += [s]
        for j in range(len(COMBOS)):
            piece, k = COMBOS[(j + shift) % len(COMBOS)]
            seam = s + 16 * 8 * (j + 1)
            put(buf, seam - k, piece)
            if j % 2:
                bounds += [seam]
        bounds += [s + span + 2000, s + span + 2300]  # (of filler: a document that is well-formed)
    bounds += [n]
    return np.frombuffer(bytes(buf), dtype=np.uint8).copy(), np.asarray(sorted(set(bounds)), dtype=np.int64), regions
