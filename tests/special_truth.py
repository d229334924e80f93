"""Allowed special tokens: two plain truths of tiktoken's rule, the literal sets and the placements at which a search can go wrong.

The rule (tiktoken's encode with allowed_special; CoreBPE::encode in the reference, src/tiktoken/tiktoken.cpp:169-234, minus its
iterator bug), per document: scanning forward, the LONGEST allowed literal that starts at the current position is cut out and gives
its id; the search goes on behind it; the text between two cuts is encoded as a subject of its own.  A literal that a document's end
cuts short is no literal.

  cuts_brute   position by position, every literal tried
  cuts_re      Python's re: an alternation of the escaped literals, longest first, finditer per document
  cuts         both, which must agree before anything is compared with them
  expected_ids cuts -> ids and document offsets, the segments through a plain encoder (the C port of oracle/)

Shared by tests/test_special_model.py (the CPU model of td_special.hip) and tests/test_gpu_special_sets.py (the kernels).  Built once,
left unchanged."""
from __future__ import annotations

import functools
import random
import re

import numpy as np

# ---- the truths ---------------------------------------------------------------------------------------------------------------------


def cuts_brute(text: bytes, offs, lits: dict[bytes, int]):
    """-> [(position, length, id)] ascending, positions in the whole text"""
    out = []
    items = sorted(lits.items(), key=lambda kv: -len(kv[0]))  # longest first: the first that fits is the longest
    for d in range(len(offs) - 1):
        p, hi = int(offs[d]), int(offs[d + 1])
        while p < hi:
            for s, i in items:
                if p + len(s) <= hi and text.startswith(s, p):
                    out.append((p, len(s), i))
                    p += len(s)
                    break
            else:
                p += 1
    return out


def cuts_re(text: bytes, offs, lits: dict[bytes, int]):
    if not lits:
        return []
    rx = re.compile(b"|".join(re.escape(s) for s in sorted(lits, key=lambda s: -len(s))), re.DOTALL)
    out = []
    for d in range(len(offs) - 1):
        lo, hi = int(offs[d]), int(offs[d + 1])
        doc = text[lo:hi]
        out += [(lo + m.start(), m.end() - m.start(), lits[m.group()]) for m in rx.finditer(doc)]
    return out


def cuts(text: bytes, offs, lits: dict[bytes, int]):
    a = cuts_brute(text, offs, lits)
    b = cuts_re(text, offs, lits)
    assert a == b, "the two truths of the rule disagree"
    return a


def expected_ids(text: bytes, offs, lits: dict[bytes, int], encode):
    """encode(bytes) -> ids of ordinary text.  -> (ids int32, document offsets int64)"""
    cs = cuts(text, offs, lits)
    ids, toffs, k = [], [0], 0
    cache = {}

    def enc(seg: bytes):
        if not seg:
            return []
        if len(seg) > 64:
            return encode(seg).tolist()
        if seg not in cache:
            cache[seg] = encode(seg).tolist()
        return cache[seg]

    for d in range(len(offs) - 1):
        p, hi = int(offs[d]), int(offs[d + 1])
        while k < len(cs) and cs[k][0] < hi:
            ids += enc(text[p:cs[k][0]])
            ids.append(cs[k][2])
            p = cs[k][0] + cs[k][1]
            k += 1
        ids += enc(text[p:hi])
        toffs.append(len(ids))
    return np.asarray(ids, dtype=np.int32), np.asarray(toffs, dtype=np.int64)


# ---- the literal sets ---------------------------------------------------------------------------------------------------------------
# Every string below is a special token of ONE vocabulary (ids from 200000 up, the Llama-4 ranks below them); a set is allowed by the
# ids of its strings.  name -> (strings, why)

CHAIN_FULL = "<s>" + "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRS"  # 48 bytes
CHAIN = [CHAIN_FULL[:k] for k in range(1, 49)]
CHAIN_SIBLINGS = ["<s>a!", "<s>a!!", "<s>a!!!", "<s>a!!!!"]
LENS_PREFIX = "<len:" + "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"[:42]  # 47 bytes
LENS = [LENS_PREFIX[:k - 1] + "|" for k in range(1, 49)]  # one literal per length, none a prefix of another
LETTERS48 = "qzxjkvwpfhgbmydculthrsnoiaeQZXJKVWPFHGBMYDCULTHRS"[:48]
MULTI_ID = "zxqjvkwpfh"        # random lower-case letters: more than one id as ordinary text (asserted by the GPU test)
TWO_PIECES = "zxqjvkwpfh wkkjqxzv"  # its second piece " wkkjqxzv" stands many times in the ordinary text too: dedupe candidates
TOO_LONG = "<" + "x" * 47 + ">"  # 49 bytes
SOUP_STRETCH = "abcd" * 12       # stretched soup literals: 48 bytes, the first 42 to 47 of them from here (40 shared by all)
assert len(CHAIN_FULL) == 48 and len(LENS[47]) == 48 and len(LETTERS48) == 48 and len(TOO_LONG) == 49

SETS = {
    "chain": (CHAIN + CHAIN_SIBLINGS,
              "every prefix of a 48-byte literal is a literal: parent is i - 1 along the chain, the match climbs it; the siblings under "
              "'<s>a' sort behind the text '<s>a\"', so the greatest literal <= the text is no prefix of it and the climb takes four steps"),
    "chain_noroot": (["<s>", "<s>a", "<s>ab", "<s>abc"], "no 1-byte root: on the text '<sz' the climb ends at parent -1"),
    "lens": (LENS, "lengths 1 to 48 behind a common prefix of up to 47 bytes: the comparison goes a dword at a time, 4k-1, 4k, 4k+1 end inside, "
                   "at the end of and just behind a dword; the 1-byte '|' sets all 256 second bytes in first2"),
    "nonascii": (["<｜begin▁of▁sentence｜>", "<｜User｜>", "§", "\U0010FFFF"],
                 "bytes above 0x7F in the key and in the compared dwords (a signed compare would misorder them); F4 8F lands in the top word of first2"),
    "words": (["ENDOFTEXT", "[INST]", "[/INST]", " \n\n", "2024", MULTI_ID, TWO_PIECES, LETTERS48],
              "literals of letters, digits and whitespace: cut out of the middle of a word, a digit run, a whitespace run; pieces that are no "
              "whole tokens (had > 1) and pieces that also stand in the ordinary text (dedupe)"),
    "alias": (["<|alias1|>", "<|alias2|>"], "two strings carry one id: allowed by the id, both are cut"),
    "one_byte": (["|", "~"], "maxlen 1: back = 0, every hit is a head, clusters have one member"),
    "one_and_48": (["|", LETTERS48], "maxlen 48 with a literal at every byte of a run of '|': the longest clusters"),
    "too_long": ([TOO_LONG, "[INST]"], "49 bytes: refused by the device search, cut by the host search"),
    "graph_a": (["[INST]", LETTERS48], "two literals, maxlen 48"),
    "graph_b": (["[/INST]", CHAIN_FULL], "two literals, maxlen 48: the table of graph_a with other contents"),
}

SOUP_ALPHABET = "abcd"


def _soup_set(rng: random.Random, stretched: bool):
    out = []
    for _ in range(rng.randint(1, 8)):
        s = "".join(rng.choice(SOUP_ALPHABET) for _ in range(rng.randint(1, 6)))
        if stretched and rng.random() < 0.75:
            s = SOUP_STRETCH[:48 - len(s)] + s
        if s not in out:
            out.append(s)
    return out


for _k in range(6):
    SETS[f"soup{_k}"] = (_soup_set(random.Random(100 + _k), _k >= 3),
                         "strings of 1 to 6 letters over {a,b,c,d}" + (", most stretched to 48 bytes by a shared 40-byte prefix" if _k >= 3 else "") +
                         ": nested, overlapping and self-overlapping literals")


@functools.lru_cache(maxsize=None)
def vocabulary():
    """-> {special string: id}: every string of every set; the two aliases share an id"""
    out, nxt = {}, 200000
    for name, (strings, _) in SETS.items():
        for s in strings:
            if s in out:
                continue
            if s == "<|alias2|>":
                out[s] = out["<|alias1|>"]
                continue
            out[s] = nxt
            nxt += 1
    return out


def literals(set_name: str) -> dict[bytes, int]:
    """the set as the truths take it: {literal bytes: id}"""
    v = vocabulary()
    return {s.encode("utf-8"): v[s] for s in SETS[set_name][0]}


def allowed_ids(set_name: str) -> list[int]:
    return sorted(set(literals(set_name).values()))


# ---- texts --------------------------------------------------------------------------------------------------------------------------

WORDS = ("the of and to in is that for it as was with be by on not he this are or his from at which but have an had they you were their "
         "one all we can her has there been if more when will would who so no out up into wkkjqxzv than them only some could time these two "
         "may then do first any my now such like our over man me even most made after also did many before must through years where much").split()


def filler(n: int, seed: int = 0) -> bytes:
    """exactly n bytes of ordinary words; the unknown word ' wkkjqxzv' is among them many times"""
    rng = random.Random(seed)
    out, size = [], 0
    while size < n:
        w = rng.choice(WORDS) + rng.choice([" ", " ", " ", ", ", ".\n", " 12 "])
        out.append(w)
        size += len(w)
    return "".join(out).encode()[:n]


class Call:
    """One device call: documents that share an allowed set."""

    def __init__(self, name: str, set_name: str, docs: list[bytes], ptr_shift: int = 0):
        self.name, self.set_name, self.docs, self.ptr_shift = name, set_name, docs, ptr_shift
        self.text = b"".join(docs)
        self.offs = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)

    def __repr__(self):
        return f"Call({self.name}, {self.set_name}, {len(self.docs)} documents, {len(self.text)} bytes)"


def _enc(strings):
    return [s.encode("utf-8") for s in strings]


def _chain_docs():
    docs = [b"<s>a\"x", b"<s>a\"", b"x<s>a!!!!\"<s>a!!!\"<s>a!\"", b"<t<", b"<", b"<<<s<s><s>a<s>ab"]
    for k in (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 47, 48):  # a chain member followed by a byte that sorts behind every continuation
        docs.append(CHAIN_FULL[:k].encode() + b"~~ " + CHAIN_FULL[:k].encode() + b"!")
    docs.append((CHAIN_FULL * 3).encode())            # back to back
    docs.append((CHAIN_FULL[:-1] * 3).encode())       # the 47-byte member, then the next starts
    docs.append(b"word " + CHAIN_FULL.encode()[:20] + b" more words")
    return docs


def _lens_docs():
    """every literal whole, then cut short at every length inside it by a document end (the last by the end of the text)"""
    docs = []
    for s in _enc(LENS):
        docs.append(b"ab " + s + b" cd" + s + s)
    for s in _enc(LENS):
        for cut in range(1, len(s)):
            docs.append(s[:cut])
            docs.append(s[cut:] + b" x")
    for cut in (47, 46, 45, 44, 43, 5, 4, 3, 2, 1):
        docs.append(b"x" + _enc(LENS)[47][:cut])
    return docs


def _nonascii_docs():
    a, b, c, d = _enc(SETS["nonascii"][0])
    return [("中文".encode() + a + "ñandú 😀".encode() + b + "\n\nمرحبا".encode() + c + "§§".encode() + d + "日本語".encode() + d + d),
            a[:-1] + b + a[1:], c[:1] + c + c[1:], d[:3] + d + d[1:] + d[:2], "<｜".encode() + a + "｜>".encode(),
            "\U0010FFFE".encode() + d + "\U000FFFFF".encode() + "\U0010FFFF\U0010FFFF".encode(), c * 40 + d * 20 + "é".encode() + c]


def _words_docs():
    L = _enc(SETS["words"][0])
    docs = []
    for s in L:
        docs.append(b"pre" + s + b"post " + s + b" 1999" + s + b"1234 \n\n\n" + s + b"\n\n  x")
    docs.append(b"un[INST]do[/INST]ne [/INST [INST][INST]] ENDOFTEXTENDOFTEXT ENDOFTEX")
    docs.append(b"20242024 12024 2 0 2 4 202 \n\n \n\n\n \n \n\n")
    docs.append(b"x zxqjvkwpfh wkkjqxzv wkkjqxzv zxqjvkwpfh wkkjqxz zxqjvkwpfhzxqjvkwpfh wkkjqxzv")
    for s in (L[5], L[7], L[1]):  # inside a piece above 64 bytes and one above 1 KiB
        docs.append(b"b" * 100 + s + b"b" * 100)
        docs.append(b"a" * 3000 + s + b"a" * 3000)
    docs.append(filler(6000, seed=4) + L[6] + filler(3000, seed=5))
    return docs


def _scan_word_docs(set_name, lit: bytes):
    """the literal's start at byte 29 .. 33 of a 32-byte scan word: its two-byte key straddles two lanes (each call starts its own text)"""
    return [Call(f"{set_name}: key at byte {at} of a scan word", set_name, [filler(64 + at, seed=at) + lit + filler(40, seed=1)]) for at in range(29, 34)]


def _border_call(set_name, lit: bytes, name):
    """documents of 16 KiB: the literal at every offset from -48 to +1 around byte 4096 (a token tile border: its pieces settle in two
    tiles) and around byte 8192 (the end of a workgroup's pass of the scan) of its document"""
    docs = []
    for k, d in enumerate(range(-48, 2)):
        a, b = 4096 + d, 8192 + d
        doc = filler(a, seed=k) + lit + filler(b - a - len(lit), seed=k + 100) + lit
        docs.append(doc + filler(16384 - len(doc), seed=k + 200))
    return Call(name, set_name, docs)


def _tiny_calls():
    """texts of 1 to 40 bytes: every word of the scan takes its tail path"""
    out = []
    src = (b"|" + LENS[5].encode() + b"|x" + LENS[20].encode() + b"||" + LENS[9].encode())
    for n in range(1, 41):
        out.append(Call(f"lens: a text of {n} bytes", "lens", [src[:n]]))
    return out


def soup_text(rng: random.Random, lits: list[bytes], max_parts: int = 60) -> bytes:
    parts = []
    for _ in range(rng.randrange(max_parts)):
        s = rng.choice(lits)
        r = rng.random()
        parts.append(s if r < 0.35 else s[:rng.randrange(len(s) + 1)] if r < 0.6 else rng.choice(b"abcde").to_bytes(1, "little") if r < 0.85
                     else bytes([rng.randrange(256)]))
    return b"".join(parts)


SOUP_CALL_BYTES = 4000  # nearly every byte of a soup is a candidate, and a call's list holds n / 32 + 4096 of them


def _soup_calls(calls_per_set: int = 2):
    out = []
    for k in range(6):
        name = f"soup{k}"
        rng = random.Random(500 + k)
        lits = _enc(SETS[name][0])
        for c in range(calls_per_set):
            docs, size, soups = [], 0, 0
            while True:
                s = soup_text(rng, lits, max_parts=16)
                if size + len(s) > SOUP_CALL_BYTES:
                    break
                cut = sorted(rng.randrange(len(s) + 1) for _ in range(rng.randrange(3)))  # documents cut anywhere
                docs += [s[a:b] for a, b in zip([0] + cut, cut + [len(s)])]
                size += len(s)
                soups += 1
            out.append(Call(f"{name}: {soups} soups, call {c}", name, docs))
    return out


@functools.lru_cache(maxsize=None)
def calls() -> tuple:
    """Every small call of the GPU file and of the model test, in a fixed order."""
    out = [Call("chain", "chain", _chain_docs()),
           Call("chain_noroot", "chain_noroot", [b"<sz", b"<s", b"<s>", b"x<s>abz<s>abc<s>abcd<sz<s", b"<s?"]),
           Call("lens", "lens", _lens_docs()),
           Call("nonascii", "nonascii", _nonascii_docs()),
           Call("words", "words", _words_docs()),
           Call("alias", "alias", [b"x<|alias1|>y<|alias2|>z", b"<|alias2|><|alias1|>", b"<|alias1|", b"|alias2|>"]),
           Call("one_byte", "one_byte", [b"|", b"a|b~c", b"||||~~~~" * 30, b"", b"~", b"no bar here", filler(300, seed=9) + b"|"]),
           Call("one_and_48", "one_and_48", [b"|" * 100 + LETTERS48.encode() + b"|" * 3 + LETTERS48.encode()[:47] + b"|", LETTERS48.encode() * 2,
                                             b"|", b"", (b"|" + LETTERS48.encode()) * 5]),
           Call("empty and 1-byte documents between cuts", "words",
                [b"[INST]", b"", b"x", b"", b"", b"[/INST]", b"2", b"0", b"2", b"4", b"2024", b"", b" ", b"\n", b"\n", b" \n\n", b"E", b"ENDOFTEXT"])]
    for c in out:
        c.group = "sets"
    groups = {
        "scan_words": _scan_word_docs("words", LETTERS48.encode()) + _scan_word_docs("nonascii", "\U0010FFFF".encode()) + _scan_word_docs("one_byte", b"|"),
        "borders": [_border_call("words", LETTERS48.encode(), "words: the 48-letter literal around bytes 4096 and 8192"),
                    _border_call("words", MULTI_ID.encode(), "words: the multi-id literal around bytes 4096 and 8192"),
                    _border_call("words", TWO_PIECES.encode(), "words: the two-piece literal around bytes 4096 and 8192")],
        "tiny": _tiny_calls(),
        # the text pointer off a 16-byte boundary: every word of the scan is loaded byte by byte
        "pointer": [Call(f"words: text pointer shifted by {shift}", "words",
                         _words_docs()[:9] + [filler(9000, seed=shift) + b"[INST]" + LETTERS48.encode()], ptr_shift=shift) for shift in (1, 4, 15)],
        "soups": _soup_calls(),
    }
    for g, cs in groups.items():
        for c in cs:
            c.group = g
        out += cs
    return tuple(out)


def config_call() -> Call:
    """About a dozen mixed documents for the launch configurations: the tile-border and long-piece cases, dedupe candidates, and 2100
    pieces above 64 bytes so that a warmed handle forks its long pieces onto the second stream."""
    rng = random.Random(77)
    L = _enc(SETS["words"][0])
    longs = b" ".join(bytes([97 + rng.randrange(26)]) * rng.randint(65, 90) for _ in range(2100))
    docs = _words_docs() + _border_call("words", LETTERS48.encode(), "").docs[44:50] + _border_call("words", TWO_PIECES.encode(), "").docs[46:50]
    docs += [longs[:70000] + L[5] + longs[70000:] + L[7] + b" " + L[6]]
    return Call("configurations", "words", docs)
