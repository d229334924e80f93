"""The NFC contract of include/tokendagger_hip.h restated twice in plain Python (nothing is read from the C++ headers or the generated
tables): nfc_by_runs splits a document at its opaque units with a bytes regex for well-formed UTF-8 and hands the runs to
unicodedata.normalize; nfc_uax15 is UAX #15 from scratch over unicodedata.combining / unicodedata.decomposition (decompose, order,
compose; Hangul by arithmetic).  Both depend on the Unicode version of the interpreter: UNICODE_VERSION says which.  Also the quick
check (flags), and limit_cases(tile_bytes): the inputs at which a decomposition into windows and tiles can go wrong."""
import re
import unicodedata as ud

import numpy as np

UNICODE_VERSION = sum(int(x) * m for x, m in zip(ud.unidata_version.split("."), (10000, 100, 1)))

# Unicode Table 3-7
WELL_FORMED = re.compile(rb"[\x00-\x7F]|[\xC2-\xDF][\x80-\xBF]|\xE0[\xA0-\xBF][\x80-\xBF]|[\xE1-\xEC\xEE\xEF][\x80-\xBF]{2}|\xED[\x80-\x9F][\x80-\xBF]"
                         rb"|\xF0[\x90-\xBF][\x80-\xBF]{2}|[\xF1-\xF3][\x80-\xBF]{3}|\xF4[\x80-\x8F][\x80-\xBF]{2}")


def units(doc: bytes):
    """-> [(code point | None, its bytes)]: at every position the well-formed sequence that starts there, or the byte alone."""
    out, p = [], 0
    while p < len(doc):
        m = WELL_FORMED.match(doc, p)
        if m:
            out.append((ord(m.group().decode("utf-8")), m.group()))
            p = m.end()
        else:
            out.append((None, doc[p:p + 1]))
            p += 1
    return out


def nfc_by_runs(doc: bytes) -> bytes:
    out, run = [], []
    for cp, raw in units(doc):
        if cp is None:
            out.append(ud.normalize("NFC", "".join(run)).encode("utf-8"))
            out.append(raw)
            run = []
        else:
            run.append(chr(cp))
    out.append(ud.normalize("NFC", "".join(run)).encode("utf-8"))
    return b"".join(out)


# ---- UAX #15 from scratch ------------------------------------------------------------------------------------------------------------
S_BASE, L_BASE, V_BASE, T_BASE, L_COUNT, V_COUNT, T_COUNT = 0xAC00, 0x1100, 0x1161, 0x11A7, 19, 21, 28
N_COUNT, S_COUNT = V_COUNT * T_COUNT, L_COUNT * V_COUNT * T_COUNT
_dec_cache = {}
_pairs = None


def decompose(cp):
    if S_BASE <= cp < S_BASE + S_COUNT:
        si = cp - S_BASE
        d = [L_BASE + si // N_COUNT, V_BASE + (si % N_COUNT) // T_COUNT]
        return d + ([T_BASE + si % T_COUNT] if si % T_COUNT else [])
    if cp not in _dec_cache:
        raw = ud.decomposition(chr(cp))
        _dec_cache[cp] = [cp] if not raw or raw.startswith("<") else [x for part in raw.split() for x in decompose(int(part, 16))]
    return _dec_cache[cp]


def pairs():
    """(a, b) -> the primary composite.  A canonical two-code-point decomposition that does not come back from its own decomposition
    is a composition exclusion (the one place where normalize is asked: unicodedata does not carry the exclusion list)."""
    global _pairs
    if _pairs is None:
        _pairs = {}
        for cp in range(0x110000):
            if 0xD800 <= cp <= 0xDFFF or S_BASE <= cp < S_BASE + S_COUNT:
                continue
            raw = ud.decomposition(chr(cp))
            if raw and not raw.startswith("<") and len(raw.split()) == 2:
                a, b = (int(x, 16) for x in raw.split())
                if ud.normalize("NFC", chr(a) + chr(b)) == chr(cp):
                    _pairs[(a, b)] = cp
    return _pairs


def compose_pair(a, b):
    if L_BASE <= a < L_BASE + L_COUNT and V_BASE <= b < V_BASE + V_COUNT:
        return S_BASE + ((a - L_BASE) * V_COUNT + (b - V_BASE)) * T_COUNT
    if S_BASE <= a < S_BASE + S_COUNT and (a - S_BASE) % T_COUNT == 0 and T_BASE < b < T_BASE + T_COUNT:
        return a + (b - T_BASE)
    return pairs().get((a, b))


def nfc_cps(cps):
    d = [x for cp in cps for x in decompose(cp)]
    # canonical ordering: a stable sort of every run of non-starters
    i = 0
    while i < len(d):
        if ud.combining(chr(d[i])) == 0:
            i += 1
            continue
        j = i
        while j < len(d) and ud.combining(chr(d[j])) != 0:
            j += 1
        d[i:j] = sorted(d[i:j], key=lambda x: ud.combining(chr(x)))
        i = j
    # composition
    out, starter, last = [], -1, 0  # starter: its index in out; last: the ccc of the last unit kept behind it
    for c in d:
        cc = ud.combining(chr(c))
        if starter >= 0:
            adjacent = len(out) == starter + 1
            if adjacent or last < cc:  # (not blocked: what was kept in between are non-starters of a lower ccc)
                comp = compose_pair(out[starter], c)
                if comp is not None:
                    out[starter] = comp
                    continue
        if cc == 0:
            starter, last = len(out), 0
        else:
            last = cc
        out.append(c)
    return out


def nfc_uax15(doc: bytes) -> bytes:
    out, run = [], []
    for cp, raw in units(doc) + [(None, b"")]:
        if cp is None:
            out.append("".join(map(chr, nfc_cps(run))).encode("utf-8"))
            out.append(raw)
            run = []
        else:
            run.append(cp)
    return b"".join(out)


# ---- the quick check -------------------------------------------------------------------------------------------------------------------
_qc = {}
_maybe = None


def quick_check(cp) -> int:
    """0 Yes, 1 Maybe, 2 No."""
    global _maybe
    if _maybe is None:
        _maybe = {b for (_, b) in pairs()} | set(range(0x1161, 0x1176)) | set(range(0x11A8, 0x11C3))
    if cp not in _qc:
        _qc[cp] = 2 if ud.normalize("NFC", chr(cp)) != chr(cp) else 1 if cp in _maybe else 0
    return _qc[cp]


def is_boundary_cp(cp) -> bool:
    return ud.combining(chr(cp)) == 0 and quick_check(cp) == 0


def doc_flag(doc: bytes) -> int:
    prev = 0
    for cp, _ in units(doc):
        if cp is None:
            prev = 0
            continue
        cc = ud.combining(chr(cp))
        if quick_check(cp) or (cc and prev > cc):
            return 1
        prev = cc
    return 0


# ---- batches ---------------------------------------------------------------------------------------------------------------------------
def offsets_of(lengths):
    offs = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lengths, dtype=np.int64), out=offs[1:])
    return offs


def batch(docs):
    """[bytes] -> (text uint8, offsets int64)"""
    return np.frombuffer(b"".join(docs), dtype=np.uint8).copy(), offsets_of([len(d) for d in docs])


def docs_of(text, offs):
    raw = bytes(np.asarray(text, dtype=np.uint8))
    return [raw[int(offs[d]):int(offs[d + 1])] for d in range(len(offs) - 1)]


def truth(text, offs, fn=nfc_by_runs):
    """-> (out uint8, out_offsets, flags, changed): what td_nfc_host must give but for the counts."""
    docs = docs_of(text, offs)
    outs = [fn(d) for d in docs]
    out, ooff = batch(outs)
    return (out, ooff, np.asarray([doc_flag(d) for d in docs], dtype=np.uint8).reshape(-1),
            np.asarray([a != b for a, b in zip(docs, outs)], dtype=np.uint8).reshape(-1))


def same(got, want, what=""):
    """got: (text, out_doc_offsets, flags, changed[, counts]) of an entry point; want: truth(...)"""
    assert np.array_equal(got[1], want[1]), (what, "offsets", got[1][:8], want[1][:8])
    assert bytes(got[0]) == bytes(want[0]), (what, "text")
    assert np.array_equal(got[2], want[2]), (what, "flags")
    assert np.array_equal(got[3], want[3]), (what, "changed")
    if len(got) > 4:
        assert got[4][0] == len(want[0]) and got[4][1] == int(want[2].sum()) and got[4][2] == int(want[3].sum()), (what, "counts", got[4])


# ---- limit cases -----------------------------------------------------------------------------------------------------------------------
def E(s):
    return s.encode("utf-8")


def U(*cps):
    """the UTF-8 of the code points"""
    return "".join(map(chr, cps)).encode("utf-8")


DIRTY = [U(0x61, 0x301, 0x323), U(0x65, 0x301)]  # rewritten: U+1EA1 U+0301, U+00E9
OUT_OF_ORDER = U(0x301, 0x323)  # ccc 230, 220: flagged
IN_ORDER = U(0x323, 0x301)      # ccc 220, 230: proven
FILL = b"The quick brown fox jumps over the lazy dog. "


def filler(n):
    return (FILL * (n // len(FILL) + 1))[:n]


def placed(piece: bytes, at: int, total: int) -> bytes:
    """`piece` at byte `at` of at least `total` bytes of ASCII."""
    return filler(at) + piece + filler(max(total - at - len(piece), 0))


def seam_cases(seam: int, total: int):
    """name -> (text, offsets): the dirty segments, an out-of-order pair and an in-order pair (each behind a letter) at every byte offset
    from 16 in front of `seam` to 16 behind it, in one document ("/"); and the same with a document boundary at `seam` ("|"): where it
    cuts the piece, marks lose their base and sequences are cut."""
    out = {}
    for name, piece in (("dirty0", DIRTY[0]), ("dirty1", DIRTY[1]), ("ooo", b"a" + OUT_OF_ORDER), ("ino", b"a" + IN_ORDER)):
        for at in range(max(seam - 16, 0), seam + 17):
            raw = placed(piece, at, total)
            out[f"{name}@{at}/{seam}"] = (np.frombuffer(raw, dtype=np.uint8).copy(), np.asarray([0, len(raw)], dtype=np.int64))
            out[f"{name}@{at}|{seam}"] = (np.frombuffer(raw, dtype=np.uint8).copy(), np.asarray([0, seam, len(raw)], dtype=np.int64))
    return out


def mark_run(n):
    """n marks of three interleaved ccc values (230, 220, 202) behind a base."""
    return b"o" + b"".join(U((0x301, 0x323, 0x327)[i % 3]) for i in range(n))


MIXED = ("Ångström café naïve Việt Nam tiếng Việt हिन्दी क़िला ज़रा "
         "한국어 조선말 ἀρχή Ελληνικά русский язык й ё "
         "日本語 がぎぐ パピプ עִבְרִית العربية أإآ ô̧ q̣̇ Å Ω "
         "̈́ ཱི \U0001d15e \U0002f800 ẛ̣ ")


def mixed(n_bytes: int, form: str) -> bytes:
    """n_bytes of the mixed-script text in the given form (the cut may fall inside a sequence)."""
    s = ud.normalize(form, MIXED).encode("utf-8")
    return (s * (n_bytes // len(s) + 1))[:n_bytes]


def limit_cases(tile_bytes: int):
    """name -> (text uint8, offsets int64): what a decomposition into 16-byte windows and tiles of tile_bytes can get wrong."""
    T = tile_bytes
    c = {}
    c["empty"] = batch([])
    c["empty documents"] = batch([b"", b"", b""])
    c["one byte"] = batch([b"a", b"", b"\xcc", b"\x81", b"b"])
    c["begins with a mark"] = batch([U(0x301, 0x61), U(0x323, 0x301), U(0x301, 0x323), U(0x1161, 0x11A8), b"a", U(0x301)])
    c["truncated then continuation"] = batch([b"e\xcc", b"\x81x", b"a\xe1\xba", b"\xa1\xcc\x81", b"\xf0\x9d\x85", b"\x9e"])
    c["ill-formed"] = batch([b"\xff", b"a\xff\xcc\x81", b"\xc0\xaf\xcc\x81", b"\xe0\x80\xaf", b"\xed\xa0\x80\xcc\x81", b"\xed\xbf\xbf", b"\xf4\x90\x80\x80",
                             b"\xf8\x88\x80\x80\x80", b"a\x80\xcc\x81", b"\xcc", b"a\xcc", b"\xe1\xba\xcc\x81", b"e\xcc\x81\xff\xcc\x81e\xcc\x81"])
    c["nothing to do"] = batch([filler(T + 7), U(0x64, 0xE9, 0x6A, 0xE0, 0x20, 0x76, 0x75, 0x20) * (T // 8), filler(3), U(0x65E5, 0x672C, 0x8A9E) * 40])
    c["nfd of mixed"] = batch([mixed(3 * T + 11, "NFD")])
    raw = mixed(3 * T, "NFD")
    c["nfd of mixed, documents"] = (np.frombuffer(raw, dtype=np.uint8).copy(),
                                    np.asarray(sorted({0, 1, 2, 17, T - 1, T, T + 1, 2 * T + 5, len(raw)}), dtype=np.int64))
    c["nfc of mixed"] = batch([mixed(2 * T + 3, "NFC")])
    c["triples"] = batch([U(0x1D1C0) * (T // 2 + 3), U(0x390) * 5, U(0x1D1C0)])
    for n in (1, 2, 31, 32, 33, 300, 5000):
        c[f"marks {n}"] = batch([b"x" * 5 + mark_run(n) + b"y", mark_run(n)[1:]])
    c["hangul across a seam"] = batch([filler(T - 4) + U(0x1100, 0x1161, 0x11A8, 0xD7A3, 0xAC01, 0xAC00, 0x11A8, 0x1100, 0xAC00, 0x1161) * 3])
    c["maybe with nothing to compose"] = batch([U(0x301), U(0x78, 0x11A8), U(0x1161), U(0x7A, 0xCD5), U(0x6B, 0x9BE)])
    c["many empty documents"] = (np.frombuffer(U(0x65, 0x301) * 3, dtype=np.uint8).copy(), np.asarray([0] * 5 + [3] * 4400 + [6, 9, 9, 9], dtype=np.int64))
    c["bytes behind the last document"] = (np.frombuffer(U(0x65, 0x301, 0x65, 0x301) + b"tail\xcc", dtype=np.uint8).copy(), np.asarray([0, 3, 6], dtype=np.int64))
    # windows that are proven by their bytes alone (all below 0xCC) and still hold opaque bytes; ASCII in whole windows: counts[5], counts[6]
    c["ascii, whole windows"] = batch([filler(64)])
    c["ascii, whole tiles"] = batch([filler(2 * T)])
    c["stray continuation bytes in whole windows"] = batch([b"a" + b"\x80" * 15 + b"b" * 16])
    low = (b"abc\x80\xbf" + b"\xc0\xaf" + b"\xc1\x81" + b"\xc3" + b"x\xc3\xa9y" + b"\xc2" + b"z") * 40
    c["ill-formed below 0xCC"] = batch([filler(T - 32) + low + filler(T + 16 - len(low) % 16)])
    raw = filler(32) + (b"\xc3\xa9" * 8) * 6 + filler(32)  # Latin-1 letters, and document boundaries that cut some of them in two
    c["documents cut two-byte letters below 0xCC"] = (np.frombuffer(raw, dtype=np.uint8).copy(),
                                                      np.asarray([0, 33, 35, 48, 49, 63, 64, 65, 80, 97, len(raw)], dtype=np.int64))
    for seam in sorted({16, T, 2 * T}):
        c.update(seam_cases(seam, 2 * T + 40))
    return c


def check_loop_geometry(n_bytes: int, shift: int = 0):
    """How td_nfc_check walks a text of n_bytes whose base lies `shift` bytes behind a 16-byte address: (step, first, rounds).  A lane is
    a window g of 16 bytes at 16 g - shift; the workgroups are one to 16 KiB of n_bytes + 16, 2048 at most, and `step` is their lanes.
    Lane g loads the windows g, g + step, g + 2 step, g + 3 step at once, then the four from g + 4 step on, ... while all four lie
    inside the text, and takes what is left one window at a time.  `rounds` is the most rounds of four a lane makes, and `first` the
    lowest lane that makes one fewer (the hand-over; at or above `step`: none does)."""
    groups = min(max((n_bytes + 16 + 16383) // 16384, 1), 2048)
    step = 256 * groups
    m = (n_bytes + shift - 16) // 16 + 1 - 3 * step  # lane g makes round k iff g + 4 k step < m
    if m <= 1:
        return step, 1, 0
    k_last = (m - 1) // (4 * step)
    return step, m - 4 * k_last * step, k_last + 1


def check_loop_case(n_bytes: int, shift: int = 0, reach: int = 17):
    """-> (text, offsets, the byte positions of the seams): n_bytes of ASCII in a few documents with the dirty segments, out-of-order pairs and
    in-order pairs laid from `reach` bytes in front of to `reach` behind every seam of the check's unrolled loop for this size and shift:
    the windows g + q step of lane 0 (the workgroups' wrap, where the four loads of a round and the rounds meet) and of the lane
    at the hand-over to the one-window loop.  A document boundary lies at or right behind most seams; some documents between them are plain."""
    step, first, rounds = check_loop_geometry(n_bytes, shift)
    seams = []
    for at in sorted({16 * (g + q * step) - shift for g in (0, first) for q in range(4 * rounds + 5)}):
        if 32 <= at <= n_bytes - 32 and (not seams or at - seams[-1] > 2 * reach + 8):
            seams.append(at)
    raw = bytearray(filler(n_bytes))
    pieces = (DIRTY[0], b"a" + OUT_OF_ORDER, b"a" + IN_ORDER, DIRTY[1])
    k = 0
    for seam in seams:
        for at in range(seam - reach, seam + reach, 7):  # (pieces of at most 5 bytes, 7 apart: windows with one and without)
            raw[at:at + len(pieces[k % 4])] = pieces[k % 4]
            k += 1
    offs = sorted({0, n_bytes} | set(seams[::2]) | {s + 3 for s in seams[1::4]} | {s + d for s in seams[::3] for d in (1000, 2000) if s + d < n_bytes})
    return np.frombuffer(bytes(raw), dtype=np.uint8).copy(), np.asarray(offs, dtype=np.int64), seams
