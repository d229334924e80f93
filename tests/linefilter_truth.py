"""The line filter's rule in plain Python (include/tokendagger_hip.h, td_line_filter*), and the seam cases both tests share."""
SPACE = b" \t\n\r\x0b\x0c"
TERMINAL = (b".", b"!", b"?", b'"', "”".encode(), "。".encode(), "！".encode(), "？".encode())
TILE = 4096


def occurrences(line: bytes, p: bytes) -> int:
    n, i = 0, line.find(p)
    while i >= 0:
        n, i = n + 1, line.find(p, i + 1)
    return n


def filter_lines(text: bytes, offsets, min_words=0, max_word_bytes=0, need_terminal=False, drop=(), count=()):
    """-> (output bytes, output offsets, stats rows, totals), all plain lists"""
    out, ooff, stats = bytearray(), [0], []
    for d in range(len(offsets) - 1):
        pieces = bytes(text[offsets[d]:offsets[d + 1]]).split(b"\n")
        row = [0] * 8
        for i, line in enumerate(pieces):
            last = i == len(pieces) - 1
            if last and not line:  # a final empty piece is no line
                break
            words, low = line.split(), line.lower()
            fails = [len(words) < min_words,
                     need_terminal and not line.rstrip(SPACE).endswith(TERMINAL),
                     max_word_bytes > 0 and max((len(w) for w in words), default=0) > max_word_bytes,
                     any(low.find(p) >= 0 for p in drop)]
            own = line + (b"" if last else b"\n")
            row[0] += 1
            for k in range(4):
                row[3 + k] += bool(fails[k])
            row[7] += sum(occurrences(low, p) for p in count)
            if not any(fails):
                row[1] += 1
                row[2] += len(own)
                out += own
        stats.append(row)
        ooff.append(len(out))
    return bytes(out), ooff, stats, [sum(r[c] for r in stats) for c in range(8)]


C4ISH = dict(min_words=2, max_word_bytes=0, need_terminal=True, drop=(b"javascript",), count=(b"aa",))
PROSE = b"Hello there, world. \nno\nA line with JavaScript in it.\naaaa x.\n\nSecond sentence here!\r\nlast words\xe2\x80\x9d \n"


def prose(n: int) -> bytes:
    return (PROSE * (n // len(PROSE) + 1))[:n]


def long_line(where) -> bytes:
    """a line of 9001 bytes over three tiles behind a line of 9, "javascript" at `where` of it (None: nowhere)"""
    line = bytearray(b"ab " * 3000)
    line[-1:] = b"."
    if where is not None:
        line[where:where + 10] = b"javascript"
    return b"Ok fine.\n" + bytes(line)


def astride(seam: int) -> bytes:
    """"JavaScript" (a word of ten bytes, a phrase in mixed case) from five bytes in front of `seam`"""
    return b"Good line.\n" + b"x " * ((seam - 16) // 2) + b"JavaScript end.\nLast line.\n"


def seam_cases():
    """name -> (text, offsets, rules)"""
    c = {}
    lengths = [0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1]
    for n in lengths:
        c[f"one document of {n}"] = (prose(n), [0, n], C4ISH)
    offs = [0]
    for n in lengths:
        offs += [offs[-1], offs[-1] + n, offs[-1] + n]
    c["the lengths between empty documents"] = (prose(offs[-1]), offs, C4ISH)
    for name, where in (("nowhere", None), ("first", 20), ("middle", 4500), ("last", 8900)):
        t = long_line(where)
        c[f"three tiles, decided {name}"] = (t + b"\nThe end.\n", [0, len(t) + 10], C4ISH)
        c[f"three tiles, no LF, decided {name}"] = (t + b"Next doc.\n", [0, len(t), len(t) + 10], C4ISH)
    word = b"Start.\n" + b"w" * 9000 + b" x\nEnd.\n"
    c["a word of 9000 against 8999"] = (word, [0, len(word)], dict(max_word_bytes=8999))
    c["a word of 9000 against 9000"] = (word, [0, len(word)], dict(max_word_bytes=9000))
    for seam in (16, 1024, TILE):
        c[f"a phrase astride {seam}"] = (astride(seam), [0, len(astride(seam))], C4ISH)
        c[f"a word astride {seam}"] = (astride(seam), [0, len(astride(seam))], dict(max_word_bytes=9))
    c["a phrase astride a document start"] = (b"a java" + b"script is. ok.\n", [0, 6, 21], C4ISH)
    c["overlapping occurrences"] = (b"aaaa b.\nAaA\n", [0, 12], dict(count=(b"aa",)))
    mark = b"ab " * 1365 + "”".encode() + b" \r\nnext one.\n"
    c["a terminal mark astride a tile seam"] = (mark, [0, len(mark)], C4ISH)
    c["a terminal mark cut by a document start"] = (b"word word \xe2\x80\x9d\n", [0, 11, 14], dict(need_terminal=True))
    behind = b"Fine words. \t\r\nFine words\xef\xbc\x9f\x0b\x0c\nno mark \n"
    c["spaces behind the mark"] = (behind, [0, len(behind)], dict(need_terminal=True))
    big = prose(1100 * 1024)
    c["more than 256 tiles"] = (big, list(range(0, len(big), 997)) + [len(big)], C4ISH)
    c["ten thousand empty documents"] = (prose(100), [0, 50] + [50] * 10000 + [100], C4ISH)
    c["nothing but empty documents"] = (b"", [0] * 10001, C4ISH)
    c["everything dropped"] = (prose(9000), [0, 3000, 9000], dict(min_words=100))
    c["empty rules"] = (prose(9000), [0, 0, 4097, 9000, 9000], {})
    return c


def make_rules(kw):
    """the rules of a case as the C ABI takes them"""
    from tokendagger_amd import capi
    phrases = [(capi.TD_LF_PHRASE_DROP_LINE, p) for p in kw.get("drop", ())] + [(capi.TD_LF_PHRASE_COUNT_DOC, p) for p in kw.get("count", ())]
    return capi.LineRules.make(kw.get("min_words", 0), kw.get("max_word_bytes", 0),
                               capi.TD_LF_NEED_TERMINAL if kw.get("need_terminal") else 0, phrases)


def same(got, want, what):
    """(text, offsets, stats, totals) as numpy arrays against filter_lines' answer"""
    assert bytes(got[0]) == want[0], (what, "text", len(got[0]), len(want[0]))
    assert got[1].tolist() == want[1], (what, "offsets")
    assert got[2].tolist() == want[2], (what, "stats")
    assert got[3].tolist() == want[3], (what, "totals", got[3], want[3])
