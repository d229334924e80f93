"""The inputs of the small-call tests (test_gpu_small_encode.py, test_gpu_decode_limits.py), built once and deterministically.
tests/test_small_inputs_model.py checks, without a GPU, every count and size the GPU tests rely on: from the compiled reference and
the vocabulary alone.  A host call of at most SMALL_MAX_BYTES and SMALL_MAX_DOCS documents is answered by ONE kernel
(td_small_encode); a piece above LONG_MAX bytes makes that kernel hand the call back."""
from __future__ import annotations

import functools
import random

import numpy as np

import cases
import helpers as H
import td_corpus
from tokendagger_amd import vocab_io

SMALL_MAX_BYTES, SMALL_MAX_DOCS = 4096, 1024
SHORT_MAX, LONG_MAX = 64, 1024  # pieces above SHORT_MAX: a wavefront each inside the kernel; above LONG_MAX: handed back
MISS_SHORT_MAX = 16             # missed pieces of 2..16 bytes merge 256 at a time, those of 17..64 bytes 64 at a time

# every spelling the table builder takes for a family scanner (GPT-2 has the two spellings below and no third)
SPELLINGS = {
    "llama4": vocab_io.LLAMA4_PAT_STR, "tekken": vocab_io.TEKKEN_PAT_STR, "cl100k": vocab_io.CL100K_PAT_STR,
    "cl100k_possessive": vocab_io.CL100K_PAT_STR_POSSESSIVE, "cl100k_current": vocab_io.CL100K_PAT_STR_CURRENT,
    "qwen2": vocab_io.QWEN2_PAT_STR, "gpt2": vocab_io.GPT2_PAT_STR, "gpt2_possessive": vocab_io.GPT2_PAT_STR_POSSESSIVE,
}
EOS_SPELLINGS = ("cl100k_current", "gpt2_possessive")  # `\s++$`: the end of the subject is part of the language
TWINS = {"llama4": H.twin_llama4, "tekken": H.twin_tekken, "cl100k": H.twin_cl100k, "gpt2": H.twin_gpt2}  # the families the CPU twin knows

TAILS = ["\r\t", "\n ", " \n\t ", "\r\n\r\n  ", "\t", "  ", "\n", " \r", "x\n\t", " \n "]  # (tests/test_cl100k_pattern.py)


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """The compiled reference running SPELLINGS[name] itself through PCRE2, over the Llama-4 vocabulary."""
    from oracle import ref
    _, mr, special = H.llama4()
    return ref.RefTokenizer(SPELLINGS[name], mr, special)


PORT_VARIANT = {"llama4": 0, "tekken": 1, "cl100k": 2, "cl100k_possessive": 2, "cl100k_current": 4, "qwen2": 5, "gpt2": 3, "gpt2_possessive": 3}


@functools.lru_cache(maxsize=None)
def restatement(name: str):
    """This package's C restatement of the spelling's language (oracle/td_oracle.c), which also DEFINES ill-formed UTF-8."""
    from oracle import port
    _, mr, _ = H.llama4()
    return port.OracleTokenizer(mr, PORT_VARIANT[name])


def well_formed(doc: bytes) -> bool:
    try:
        doc.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def truth_ids(name: str, doc: bytes, mode: int = 0) -> np.ndarray:
    """The ids of one document (mode 1: encode_ordinary).  Well-formed UTF-8: the compiled reference (CoreBPE::encode).  Ill-formed UTF-8 (a document cut inside a
    character, a stray continuation byte): the reference runs PCRE2 with NO_UTF_CHECK and leaves it undefined; what this package
    defines for it is its restatement (tests/test_gpu_parity.py::test_malformed_utf8_is_handled_like_the_oracle)."""
    T = reference(name) if well_formed(doc) else restatement(name)
    return T.encode_ordinary(doc) if mode else T.encode(doc)


def piece_lengths(name: str, doc: bytes) -> list[int]:
    """The lengths of the document's pieces: the reference's split_text, or the restatement's where the document is ill-formed."""
    if well_formed(doc):
        return [len(p) for p in reference(name).split_pieces(doc)]
    from oracle import port
    return np.diff(np.concatenate([[0], port.split(doc, PORT_VARIANT[name])])).tolist()


def hands_back(name: str, doc: bytes) -> bool:
    """A piece above LONG_MAX bytes: td_small_encode hands the call back to the general path."""
    return max(piece_lengths(name, doc), default=0) > LONG_MAX


def truth_batch(name: str, text: bytes, offs) -> tuple[np.ndarray, np.ndarray]:
    """-> (ids, offsets): truth_ids of every document (the reference's encode_batch encodes each document by itself as well)"""
    parts = [truth_ids(name, text[offs[d]:offs[d + 1]]) for d in range(len(offs) - 1)]
    out = np.zeros(len(offs), dtype=np.int64)
    np.cumsum([len(q) for q in parts], out=out[1:])
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)).astype(np.int32), out


def _corpus(kind: str, n: int, seed: int = 41) -> bytes:
    return {"english": td_corpus.english, "mixed": td_corpus.mixed, "code": td_corpus.code}[kind](max(n, 1 << 14), seed=seed)[0].tobytes()[:n]


def whole(docs) -> tuple[bytes, np.ndarray]:
    return H.pack_docs(list(docs))


def max_piece(R, doc: bytes) -> int:
    return max((len(p) for p in R.split_pieces(doc)), default=0)


# ---- 1: documents alone -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def documents() -> tuple[bytes, ...]:
    """Every string of tests/cases.py, about 1500 joins of fuzz_string, and strings that end in one to three of TAILS; none empty.
    A few hold a piece above LONG_MAX bytes (those calls are handed back); only strings of tests/cases.py exceed SMALL_MAX_BYTES (the
    kernel is not asked)."""
    rng = random.Random(1)
    out = [s.encode("utf-8") for _, s in cases.all_strings()]
    for i in range(1500):
        parts = [H.fuzz_string(rng) for _ in range(rng.choice([1, 2, 5, 12, 40, 120, 300]))]
        d = "".join(parts).encode("utf-8")
        while len(d) > SMALL_MAX_BYTES:
            parts.pop()
            d = "".join(parts).encode("utf-8")
        out.append(d)
    bases = ["ab", "", "x ", "don't", "12", "中", "a.", " ", "The end", "'s"] + [H.fuzz_string(rng) for _ in range(20)]
    for b in bases:
        for t in TAILS:
            out.append((b + t * rng.randint(1, 3)).encode("utf-8"))
    out += [b"a" * 1500, b"x" + b" " * 1100 + b"y", b"=" * 1025 + b"\n", ("的" * 400).encode("utf-8"), b"a" * SMALL_MAX_BYTES]
    n_cases = len(cases.all_strings())
    assert all(len(d) <= SMALL_MAX_BYTES for d in out[n_cases:])
    out = [d for d in out if d]
    return tuple(out)


# ---- 2: every lane border -----------------------------------------------------------------------------------------------------------
PROBES = [b"'s", b"'S", b"'ll", b"'LL", "a'ſt".encode(), b" \n", b"\r\n", b"  x", b" \n\n y", "é".encode(), "中".encode(),
          "\U0001F600".encode(), b"12345", b"a1b", "١٢٣".encode(), "\u2028".encode(), "\u00a0".encode(), b"!/\n/", b"...",
          b" The", b"McDonald", "ǅe".encode(), b"\x00", b"\x80", b"\xe4\xb8", b"'re'RE", b"'t ", b"x's", b" 's", b"''ll", b"\t\t", b" \r",
          b"\n\n", b"a/\n", b"A\r\n", "\u0301\u0301".encode(), b"1 2", b"$%", b" 9", b"Ab"]
FILLERS = {"letters": b"x" * 48, "digits": b"7" * 48, "english": b"It is a truth, they said; nobody's sure of 1813."}
BORDER_K = range(0, 49)


@functools.lru_cache(maxsize=None)
def border_inputs() -> tuple[bytes, ...]:
    """Each probe behind the first k bytes of each filler, k = 0..48, with " tail" behind it: the probe at every place of a lane's 16
    bytes, behind a run with no sync point ("x" * k), behind pieces at stride 3 from the run's start ("7" * k) and behind text."""
    assert all(len(f) == 48 for f in FILLERS.values())
    return tuple(f[:k] + p + b" tail" for f in FILLERS.values() for k in BORDER_K for p in PROBES)


# ---- 3: document cuts inside a small batch ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cut_batches() -> dict:
    """name -> (text, offsets, answered by the kernel)"""
    mixed = _corpus("mixed", SMALL_MAX_BYTES)
    eng = _corpus("english", 100)
    every4 = np.arange(0, SMALL_MAX_BYTES + 1, 4, dtype=np.int64)
    return {
        "every_4_bytes": (mixed, every4, True),
        "1025_documents": (mixed, np.sort(np.concatenate([every4, [2]])).astype(np.int64), False),
        "one_byte_documents": (mixed[:SMALL_MAX_DOCS], np.arange(SMALL_MAX_DOCS + 1, dtype=np.int64), True),
        "empty_documents": (eng, np.asarray([0, 0, 0, 5, 5, 16, 16, 16, 33, 48, 48, 64, 100, 100, 100], dtype=np.int64), True),
    }


@functools.lru_cache(maxsize=None)
def random_cuts() -> tuple:
    """200 draws: a piece of English, mixed or code text with a random set of cuts (doubles: empty documents)."""
    rng = random.Random(3)
    out = []
    for i in range(200):
        n = rng.choice([rng.randint(1, 64), rng.randint(1, 600), rng.randint(1, SMALL_MAX_BYTES), SMALL_MAX_BYTES])
        text = _corpus(("english", "mixed", "code")[i % 3], n, seed=50 + i % 7)
        k = min(rng.choice([0, 1, 3, 17, 100, 600, SMALL_MAX_DOCS - 1]), SMALL_MAX_DOCS - 1)
        cuts = sorted(rng.randint(0, n) for _ in range(k))
        out.append((text, np.asarray([0] + cuts + [n], dtype=np.int64)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def eos_batches() -> tuple:
    """Documents that END in each whitespace tail, each followed by a document that starts with a letter, a blank, a newline or
    nothing: the end of a document that is not the end of the text."""
    out = []
    for base in ("ab", "", "a.", "12"):
        docs = []
        for t in TAILS:
            for rep in (1, 3):
                for nxt in ("x", " y", "\nz", ""):
                    docs += [(base + t * rep).encode(), nxt.encode()]
        out.append(tuple(docs))
    assert all(sum(map(len, d)) <= SMALL_MAX_BYTES and len(d) <= SMALL_MAX_DOCS for d in out)
    return tuple(out)


# ---- 4: sizes -------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 15, 16, 17, 4095, 4096, 4097)


@functools.lru_cache(maxsize=None)
def size_texts() -> tuple:
    """(text, answered by the kernel): n bytes of English, mixed and code text for every n of SIZES, and texts whose last character has
    3 and 4 bytes and ends exactly at byte 4096."""
    out = []
    for kind in ("english", "mixed", "code"):
        t = _corpus(kind, SMALL_MAX_BYTES + 1)
        out += [(t[:n], n <= SMALL_MAX_BYTES) for n in SIZES]
    eng = _corpus("english", SMALL_MAX_BYTES)
    out += [(eng[:SMALL_MAX_BYTES - 3] + "中".encode(), True), (eng[:SMALL_MAX_BYTES - 4] + "\U0001F600".encode(), True)]
    assert all(len(t) == SMALL_MAX_BYTES for t, _ in out[-2:])
    return tuple(out)


# ---- 5: the miss merge's batches -------------------------------------------------------------------------------------------------
RARE = "qxzjvk"
CONSONANTS = "bcdfghjklmnpqrstvwxz"
FILLER_WORDS = (b" the", b" of", b" and")


def _miss_word(rng, n_letters: int, mr, seen) -> bytes:
    for _ in range(1000):
        w = (" " + "".join(rng.choice(RARE if n_letters <= 15 else CONSONANTS) for _ in range(n_letters))).encode()
        if w not in mr and w not in seen:
            seen.add(w)
            return w
    raise AssertionError("no word of that length outside the vocabulary")


@functools.lru_cache(maxsize=None)
def miss_text(n_short: int, n_long: int, seed: int = 5) -> bytes:
    """Exactly n_short pieces of 2..16 bytes and n_long pieces of 17..64 bytes that are no token (words of rare letters, each checked
    against the vocabulary), in random order among filler words that are tokens."""
    _, mr, _ = H.llama4()
    rng = random.Random(seed)
    seen = set()
    short_letters = (3, 3, 3, 4, 3, 3, 15, 3, 5, 3) if n_short <= 300 else (3, 4, 4)  # (piece = a blank + the letters)
    long_letters = (16, 16, 19, 16, 63, 16, 32, 16) if n_long <= 100 else (16, 16, 16, 17, 16, 16, 16, 30)
    words = [_miss_word(rng, short_letters[i % len(short_letters)], mr, seen) for i in range(n_short)]
    words += [_miss_word(rng, long_letters[i % len(long_letters)], mr, seen) for i in range(n_long)]
    rng.shuffle(words)
    out = []
    for i, w in enumerate(words):
        out.append(w)
        if i % 11 == 10:
            out.append(FILLER_WORDS[(i // 11) % len(FILLER_WORDS)])
    text = b"".join(out)
    assert len(text) <= SMALL_MAX_BYTES, len(text)
    return text


MISS_COUNTS = [(256, 0), (257, 0), (512, 0), (513, 0), (0, 64), (0, 65), (0, 128), (0, 129), (310, 72)]


def count_misses(R, mr, text: bytes) -> tuple[int, int]:
    """-> (pieces of 2..16 bytes, pieces of 17..64 bytes) of `text` that are no token"""
    pieces = [p for p in R.split_pieces(text) if p not in mr]
    return sum(2 <= len(p) <= MISS_SHORT_MAX for p in pieces), sum(MISS_SHORT_MAX < len(p) <= SHORT_MAX for p in pieces)


# ---- 6: a vocabulary that is not merge-closed -----------------------------------------------------------------------------------
TOY_LONG_TOKEN = b"abcd" * 20


def toy_open_vocab() -> dict[bytes, int]:
    """All 256 bytes plus " a", "ab", "abcd" and "abcd" * 20: no merge makes "abcd" ("cd" is no token) or the 80-byte token, so encode
    (whole-piece table first, tiktoken.cpp:209-215) and encode_ordinary differ on them — the Llama-4 vocabulary is merge-closed and
    cannot tell whether the whole-piece lookup of a piece above 64 bytes ran."""
    v = {bytes([i]): i for i in range(256)}
    v.update({b" a": 256, b"ab": 257, b"abcd": 258, TOY_LONG_TOKEN: 259})
    return v


@functools.lru_cache(maxsize=None)
def toy_open_inputs() -> tuple[bytes, ...]:
    rng = random.Random(6)
    return (b" a" * 2048, b"abcd " * 800, bytes(rng.choice(b"abcd") for _ in range(300)), b"abcd", TOY_LONG_TOKEN,
            b"ab\n" + TOY_LONG_TOKEN + b"\n" + TOY_LONG_TOKEN)


# ---- 7: pieces of 65..1024 bytes inside the kernel ---------------------------------------------------------------------------------
LONG_LENGTHS = (64, 65, 66, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025)


@functools.lru_cache(maxsize=None)
def long_single_pieces() -> tuple:
    """(text, length of its one long piece): one letter, random letters, dashes, blanks up to the end of the text, a CJK character, an
    emoji; lengths of multi-byte characters rounded down to whole characters."""
    rng = random.Random(7)
    out = []
    for n in LONG_LENGTHS:
        out.append((b"a" * n, n))
        out.append((bytes(rng.choice(b"etaoinshrdlu") for _ in range(n)), n))
        out.append((b"-" * n, n))
        out.append((b"x" + b" " * n, n))
        out.append(("的".encode() * (n // 3), n // 3 * 3))
        out.append(("\U0001F600".encode() * (n // 4), n // 4 * 4))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def long_tokens() -> tuple[bytes, ...]:
    """The vocabulary's tokens above 64 bytes (74 of them, 65..113 bytes)."""
    _, mr, _ = H.llama4()
    return tuple(sorted((b for b in mr if len(b) > SHORT_MAX), key=lambda b: (len(b), b)))


@functools.lru_cache(maxsize=None)
def long_token_texts() -> tuple:
    """(text, token): every long token between "x " and the end of the text, and between two words."""
    return tuple((pre + t + post, t) for t in long_tokens() for pre, post in ((b"x ", b""), (b"word ", b" word")))


@functools.lru_cache(maxsize=None)
def long_many() -> dict:
    """name -> (text, pieces above 64 bytes): six pieces of 600 bytes (more than one per wavefront of the four), and 63 pieces of 65
    bytes (4095 bytes: the long list nearly full)."""
    rng = random.Random(8)
    word = lambda n: b" " + bytes(rng.choice(b"etaoinshrdlu") for _ in range(n - 1))  # noqa: E731
    return {"six_of_600": (b"".join(word(600) for _ in range(6)), 6), "63_of_65": (b"".join(word(65) for _ in range(63)), 63)}


# ---- 8: errors -------------------------------------------------------------------------------------------------------------------------
def toy_holes_vocab() -> dict[bytes, int]:
    """Every byte but "c" and "Z" (ids stay the byte values)."""
    return {bytes([i]): i for i in range(256) if bytes([i]) not in (b"c", b"Z")}


def full_byte_vocab() -> dict[bytes, int]:
    return {bytes([i]): i for i in range(256)}


ERROR_INPUTS = {
    "one_byte_piece": b"c ab de",
    "missed_piece_of_5": b"ab abcd ef gh",
    "missed_piece_of_40": b"ab " + b"a" * 20 + b"c" + b"a" * 18 + b" ef",
    "piece_of_200": b"ab " + b"a" * 120 + b"c" + b"a" * 78 + b" ef",
    "piece_of_200_first_byte": b"ab Z" + b"a" * 198 + b" ef",
    "two_unknown_bytes": b"ab abcd ef " + b"Z" + b"a" * 99 + b" gh",
}
ERROR_PIECE_LEN = {"one_byte_piece": 1, "missed_piece_of_5": 5, "missed_piece_of_40": 40, "piece_of_200": 200, "piece_of_200_first_byte": 200}


def pieces_with_unknown_bytes(R_full, text: bytes, known) -> list[tuple[int, int]]:
    """[start, end) of every piece of `text` (the reference's split, full byte vocabulary) that holds a byte outside `known`"""
    out, pos = [], 0
    for p in R_full.split_pieces(text):
        if any(bytes([b]) not in known for b in p):
            out.append((pos, pos + len(p)))
        pos += len(p)
    assert pos == len(text)
    return out
