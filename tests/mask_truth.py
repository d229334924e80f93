"""The address mask's rule in plain Python (include/tokendagger_hip.h, td_mask_addresses*), and the seam cases both tests share."""
ALNUM = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
L, D, TILE = ALNUM + b"._%+-", ALNUM + b".-", 4096
PRIVATE = ((0, 8), (10 << 24, 8), (127 << 24, 8), (169 << 24 | 254 << 16, 16), (172 << 24 | 16 << 16, 12), (192 << 24 | 168 << 16, 16), (224 << 24, 3))


def fnv(b: bytes) -> int:
    h = 2166136261
    for c in b:
        h = ((h ^ c) * 16777619) & 0xFFFFFFFF
    return h


def email_at(doc: bytes, a: int):
    """the '@' at a -> (start, end) of the match, or None"""
    i, j = a, a + 1
    while i > 0 and doc[i - 1] in L:
        i -= 1
    while j < len(doc) and doc[j] in D:
        j += 1
    local, run = doc[i:a], doc[a + 1:j]
    dom = run[:-1] if run.endswith(b".") else run
    labels = dom.split(b".")
    ok = (1 <= len(local) <= 64 and local[:1] != b"." and local[-1:] != b"." and doc[max(i - 1, 0):i] != b"@" and 1 <= len(run) <= 254
          and doc[j:j + 1] != b"@" and len(labels) >= 2 and all(1 <= len(x) <= 63 and x[:1] != b"-" and x[-1:] != b"-" for x in labels)
          and 2 <= len(labels[-1]) <= 24 and labels[-1].isalpha() and len(local) + 1 + len(dom) <= 254)
    return (i, a + 1 + len(dom)) if ok else None


def ip_at(doc: bytes, p: int):
    """the digit at p -> (start, end, private) of the match, or None"""
    j = p
    while j < len(doc) and doc[j] in b"0123456789.":
        j += 1
    parts, behind = doc[p:j].split(b"."), doc[j:j + 1]
    if len(parts) == 5 and parts[4] == b"":  # one dot behind the quad stays in the text
        parts, j = parts[:4], j - 1
    if (p > 0 and doc[p - 1] in L) or len(parts) != 4 or (behind and (behind in L or behind == b"@")):
        return None
    if any(not 1 <= len(o) <= 3 or int(o) > 255 or (len(o) > 1 and o[:1] == b"0") for o in parts):
        return None
    v = int(parts[0]) << 24 | int(parts[1]) << 16 | int(parts[2]) << 8 | int(parts[3])
    return p, j, any(v >> (32 - bits) == net >> (32 - bits) for net, bits in PRIVATE)


def mask(text: bytes, offsets, emails=(), ips=(), keep=False):
    """-> (output bytes, output offsets, stats rows, totals), all plain lists; a kind with no literal is off"""
    out, ooff, stats = bytearray(), [0], []
    for d in range(len(offsets) - 1):
        doc = bytes(text[offsets[d]:offsets[d + 1]])
        row, done = [0] * 6, 0
        for p, c in enumerate(doc):
            m = None
            if c == 0x40 and emails and email_at(doc, p):
                m = email_at(doc, p) + (emails,)
            elif 0x30 <= c <= 0x39 and ips and ip_at(doc, p):
                s, e, private = ip_at(doc, p)
                row[2] += private and keep
                m = None if private and keep else (s, e, ips)
            if m:
                s, e, lits = m
                assert s >= done, "matches do not overlap"
                lit = lits[fnv(doc[s:e]) % len(lits)]
                out += doc[done:s] + lit
                done = e
                row[0 if lits is emails else 1] += 1
                row[3] += e - s
                row[4] += len(lit)
        out += doc[done:]
        row[5] = len(doc) - row[3] + row[4]
        stats.append(row)
        ooff.append(len(out))
    return bytes(out), ooff, stats, [sum(r[c] for r in stats) for c in range(6)]


BOTH = dict(emails=(b"email@example.com",), ips=(b"0.0.0.0",), keep=True)
EIGHT = dict(emails=tuple(b"<mail %d>" % i for i in range(8)), ips=tuple(b"<ip " + b"x" * i + b">" for i in range(8)), keep=False)
PROSE = b"The quick brown fox, in 2019, paid 3.50 for v1.2 of it; 40% + 2 is more_or-less 12.5.\n"
SAMPLE = b"Mail bob@example.com or 8.8.8.8, not 10.0.0.1 nor a@b.co@d.org; see x@1.2.3.4 and 1.2.3.4@x.org.\n"
ODD = [b"a@b.co@d.org", b"x@1.2.3.4", b"1.2.3.4@x.org", b"bob@x.com.", b".bob@x.com", b"bob.@x.com", b"a@-b.com", b"a@b-.com", b"a@b-c.com", b"a@b.c",
       b"a@b." + b"c" * 24, b"a@b." + b"c" * 25, b"a@b.c0m", b"a@b..com", b"a@.com", b"a@b.com..", b"@b.com", b"a@", b"255.255.255.255", b"256.1.1.1",
       b"01.2.3.4", b"0.0.0.0", b"1.2.3.4.", b"1.2.3.4.5", b"1.2.3.4..", b"v1.2.3.4", b"1.2.3.4.x", b"1.2.3.4@", b"1.2.3.4.@", b"1.2.3", b"1234.1.1.1",
       b"1.2.3.4-", b"_1.2.3.4", b"(1.2.3.4)", b"a%b+c_d-e.f@sub.dom-ain.example.museum", b"a@b.cd1.2.3.4"]
RANGES = [b"0.0.0.0", b"0.255.255.255", b"1.0.0.0", b"9.255.255.255", b"10.0.0.0", b"10.255.255.255", b"11.0.0.0", b"126.255.255.255", b"127.0.0.0",
          b"127.255.255.255", b"128.0.0.0", b"169.253.255.255", b"169.254.0.0", b"169.254.255.255", b"169.255.0.0", b"172.15.255.255", b"172.16.0.0",
          b"172.31.255.255", b"172.32.0.0", b"192.167.255.255", b"192.168.0.0", b"192.168.255.255", b"192.169.0.0", b"223.255.255.255", b"224.0.0.0",
          b"255.255.255.255"]
LONG = b"x" * 64 + b"@" + b"a" * 63 + b"." + b"b" * 63 + b"." + b"c" * 57 + b".com"  # 254 bytes


def prose(n: int, sample: bytes = PROSE) -> bytes:
    return (sample * (n // len(sample) + 1))[:n]


def put(text: bytearray, s: int, addr: bytes):
    text[s - 1:s + len(addr) + 1] = b" " + addr + b" "


def placed(addr: bytes, idx: int, seams, span: int = 3 * TILE) -> tuple:
    """a document of three tiles a seam, byte idx of addr on that seam of its second tile -> (text, offsets)"""
    text = bytearray(prose(span * len(seams)))
    for i, seam in enumerate(seams):
        put(text, i * span + TILE + seam - idx, addr)
    return bytes(text), list(range(0, len(text) + 1, span))


def seam_cases():
    """name -> (text, offsets, rules)"""
    c = {}
    lengths = [0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1]
    for n in lengths:
        c[f"one document of {n}"] = (prose(n, SAMPLE), [0, n], BOTH)
    offs = [0]
    for n in lengths:
        offs += [offs[-1], offs[-1] + n, offs[-1] + n]
    c["the lengths between empty documents"] = (prose(offs[-1], SAMPLE), offs, EIGHT)
    seams = [15, 16, 17, 1023, 1024, TILE - 1, TILE, TILE + 1]
    mail, quad = b"john.doe+tag@mail.example.org", b"123.45.67.89"
    for name, addr, idx in (("@", mail, 12), ("first byte", mail, 0), ("last byte", mail, len(mail) - 1), ("quad's first byte", quad, 0),
                            ("quad's last byte", quad, len(quad) - 1), ("254 bytes' @", LONG, 64)):
        c[f"the {name} on every seam"] = placed(addr, idx, seams[3:] if addr is LONG else seams) + (BOTH,)
    limits = [LONG, b"y" + LONG, LONG + b"c", LONG[63:], LONG[:64] + b"@" + b"d" * 61 + b"." + LONG[65:],
              b"a@" + b"a" * 63 + b"." + b"b" * 63 + b"." + b"c" * 63 + b"." + b"d" * 56 + b".com.", b"a@" + b"a.a." * 62 + b"aa.com", b"a@" + b"a.a." * 62 + b"aaa.com"]
    for name, items in (("LOCAL, RUN and the address at their limits", limits), ("odd forms", ODD), ("private ranges kept", RANGES), ("private ranges", RANGES)):
        text, offs = b" ".join(items) + b"\n", [0]
        for x in items:
            text, offs = text + x, offs + [len(text), len(text) + len(x)]
        c[name] = (text, offs, dict(BOTH, keep=name != "private ranges"))
    far = bytearray(prose(3 * TILE))
    put(far, TILE + 10 - 64, LONG)  # LOCAL begins in the tile in front of the '@'
    put(far, 2 * TILE - 96, LONG)   # DOMAIN ends in the tile behind it
    c["both of the reach's ends in the neighbouring tiles"] = (bytes(far), [0, 3 * TILE], BOTH)
    cut = b"bob@example.com bob@ex.com.org 11.2.3.4 1.2.3.4"
    c["document starts that cut LOCAL, DOMAIN and a quad"] = (cut, [0, 2, 15, 26, 30, 32, 39, 42, len(cut)], BOTH)
    c["empty literals"] = (prose(5000, SAMPLE), [0, 2500, 5000], dict(emails=(b"",), ips=(b"", b""), keep=False))
    c["literals of 32 bytes"] = (prose(5000, SAMPLE), [0, 2500, 5000], dict(emails=(b"E" * 32,) * 8, ips=(b"I" * 32, b"i" * 32), keep=False))
    many = b"".join(b"u%d@h%d.example.com 8.%d.%d.9 " % (i, i * 7, i, i * 13 % 251) for i in range(200))
    c["eight literals"] = (many, [0, len(many) // 2, len(many)], EIGHT)
    c["e-mail alone"] = (prose(5000, SAMPLE), [0, 5000], dict(emails=(b"<m>",)))
    c["IPv4 alone"] = (prose(5000, SAMPLE), [0, 5000], dict(ips=(b"<i>",), keep=True))
    c["back-to-back minimal matches"] = (b"a@b.cd " * 1200, [0, 4200, 8400], EIGHT)
    c["back-to-back minimal quads"] = (b"1.1.1.1 " * 1100, [0, 8800], EIGHT)
    big = bytearray(prose(1100 * 1024))
    for i, at in enumerate((5, 4090, 70000, 70100, 500000, 1000001, len(big) - 40)):
        big[at:at + 30] = b" me%d@site.example.org 9.9.9.%d " % (i, i)
    c["more than 256 tiles"] = (bytes(big), list(range(0, len(big), 997)) + [len(big)], BOTH)
    c["ten thousand empty documents"] = (prose(200, SAMPLE), [0, 100] + [100] * 10000 + [200], BOTH)
    c["nothing but empty documents"] = (b"", [0] * 10001, BOTH)
    c["the identity"] = (prose(9000, SAMPLE), [0, 0, 4097, 9000, 9000], {})
    return c


def make_rules(kw):
    """the rules of a case as the C ABI takes them"""
    from tokendagger_amd import capi
    flags = (capi.TD_MA_EMAILS if kw.get("emails") else 0) | (capi.TD_MA_IPS if kw.get("ips") else 0) | (capi.TD_MA_KEEP_PRIVATE_IPS if kw.get("keep") else 0)
    return capi.MaskRules.make(flags, kw.get("emails", ()), kw.get("ips", ()))


def same(got, want, what):
    """(text, offsets, stats, totals) as numpy arrays against mask's answer"""
    assert bytes(got[0]) == want[0], (what, "text", len(got[0]), len(want[0]))
    assert got[1].tolist() == want[1], (what, "offsets")
    assert got[2].tolist() == want[2], (what, "stats")
    assert got[3].tolist() == want[3], (what, "totals", got[3], want[3])
