"""The fused tile loop inside its smaller LDS budget (seven workgroups per CU): nine class masks are stored and MK_N, MK_A,
MK_SP and MK_D are derived where a view is loaded (td_common.h: cm_expand, CompactMaskP), and the lists are shorter
(FZ_NPC, FZ_CCAP, KS_HCAP in td_kernels.hip).  Every case goes through the C ABI against the compiled reference, in the
three forms of the loop (staged, TD_OPT_FUSED = 0, TD_OPT_DIRECT = 1), which must agree id for id.

  derived masks     a probe string of the bytes whose classes are derived (digit runs of 1..7, apostrophes with and without
                    a contraction, blanks, tabs, CR/LF runs, both cases, a multi-byte letter and a multi-byte digit)
                      - as inputs of three tiles at every offset 0..63 relative to a 64-byte mask word (Llama-4), and
                      - at every byte of the string across the tile border, the edge of the left halo (128 bytes in front of
                        a tile) and the edge of the right halo (192 bytes behind it), for every pattern family the kernel is
                        instantiated for: one buffer per family whose tile borders each carry the string at another position
                        (a border inside a long buffer takes the same code as the border of a two-tile input, and a call
                        per position would be 500 calls per family)
  document starts   a start at every byte of a 70-byte stretch around a tile border, behind an apostrophe and inside blank
                    runs included (same construction: border b carries the start at offset b - 36)
  at the caps       one tile with a swept number of pieces / pieces of 14 bytes / unresolved heads: TD_INFO_DEFERRED_TILES
                    flips from zero exactly once over the sweep where a cap defers the tile, and the ids are the reference's
                    below, at and above it

Reference behaviour: CoreBPE::encode, src/tiktoken/tiktoken.cpp:169-234 of the reference (through oracle/_ref, the checker).
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

import helpers as H
import td_corpus
from oracle import ref
from tokendagger_amd import capi, vocab_io

pytestmark = pytest.mark.gpu

TILE = 8192  # bytes per pre-tokenizer tile (KS_TILE); K_HL = 128 in front, K_HR = 192 behind
FAMILIES = {
    "llama4": vocab_io.LLAMA4_PAT_STR, "tekken": vocab_io.TEKKEN_PAT_STR, "cl100k": vocab_io.CL100K_PAT_STR,
    "cl100k_current": vocab_io.CL100K_PAT_STR_CURRENT, "qwen2": vocab_io.QWEN2_PAT_STR, "gpt2": vocab_io.GPT2_PAT_STR,
}
# the bytes whose masks are derived: MK_N (digit runs of 1..7), MK_A (apostrophes with and without a contraction), MK_SP / MK_TR
# (blanks, tabs, CR/LF runs), letters of both cases, a two-byte letter, a two-byte digit (U+0663)
PROBE = "7 42 123 1234 12345 123456 1234567 don't I'LL 'q' x' ''a  b\t\tc \r\n\r\nd\n\n  Ee FF gH é٣ ٣٣ z.".encode("utf-8")
STRETCH = b"so don't  \n\n it's 'x  \t y'all   can't \r\n  'tis o'clock   'em we've  ok yes "


@functools.lru_cache(maxsize=None)
def _filler() -> bytes:
    return td_corpus.english(1 << 16, seed=17)[0].tobytes()


_PAIRS: dict = {}


def _pair(family: str):
    """-> (the family's handle on the GPU, the compiled reference with the same pattern), made once per module"""
    if family not in _PAIRS:
        assert ref.available(), "oracle/_ref/libtdref.so is missing: build it where a checkout of the reference can be read (oracle/build_ref.sh)"
        _, mr, special = H.llama4()
        t = capi.HipTokenizer(FAMILIES[family], mr, special, device=0)
        t.set_option(capi.TD_OPT_SMALL_PATH, 0)  # (the one-launch path for tiny inputs is not what is tested here)
        _PAIRS[family] = (t, ref.RefTokenizer(FAMILIES[family], mr, special))
    return _PAIRS[family]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for t, _ in _PAIRS.values():
        t.close()
    _PAIRS.clear()


def _forms(tok, text: bytes, offs):
    """the staged form's (ids, offsets, deferred token tiles) after checking that the two other forms give the same"""
    offs = np.asarray(offs, dtype=np.int64)
    st, so = tok.encode_batch(text, offs)
    deferred = tok.info(capi.TD_INFO_DEFERRED_TILES)
    tok.set_option(capi.TD_OPT_FUSED, 0)
    ut, uo = tok.encode_batch(text, offs)
    tok.set_option(capi.TD_OPT_FUSED, 1)
    tok.set_option(capi.TD_OPT_DIRECT, 1)
    dt, do = tok.encode_batch(text, offs)
    tok.set_option(capi.TD_OPT_DIRECT, 0)
    assert np.array_equal(so, uo) and np.array_equal(st, ut), "the fused and the two-kernel form differ"
    assert np.array_equal(so, do) and np.array_equal(st, dt), "the staged form and direct placement differ"
    return st, so, deferred


def _check(family: str, text: bytes, offs, what: str) -> int:
    tok, R = _pair(family)
    st, so, deferred = _forms(tok, text, offs)
    _, et, eo = R.encode_batch(np.frombuffer(text, dtype=np.uint8), np.asarray(offs, dtype=np.int64), n_threads=min(os.cpu_count() or 1, 16))
    assert np.array_equal(so, eo), f"{family}, {what}: document offsets differ from the reference"
    bad = np.flatnonzero(st != et)
    assert bad.size == 0, f"{family}, {what}: ids differ from the reference, first at token {bad[:1]}"
    return deferred


def _borders_buffer(piece: bytes, edges, positions):
    """English filler of len(edges) * len(positions) + 1 tiles; border b = 1, 2, ... carries `piece` so that its byte
    positions[..] lies on the border (or on the halo edge `edge` bytes from it).  Documents are cut in the middle of every tile."""
    f = _filler()
    nb = len(edges) * len(positions)
    buf = bytearray((f * ((nb + 2) * TILE // len(f) + 1))[:(nb + 1) * TILE + TILE // 2])
    b = 1
    for e in edges:
        for d in positions:
            at = b * TILE + e - d
            buf[at:at + len(piece)] = piece
            b += 1
    offs = [0] + [k * TILE + TILE // 2 for k in range(1, nb + 1)] + [len(buf)]
    return bytes(buf), offs


def test_derived_masks_at_every_offset_of_a_mask_word():
    unit = PROBE + b" "
    for s in range(64):
        text = b"x" * s + unit * ((3 * TILE - s) // len(unit))
        assert 2 * TILE < len(text) <= 3 * TILE
        _check("llama4", text, [0, len(text)], f"probe string shifted by {s}")


@pytest.mark.parametrize("family", list(FAMILIES))
def test_derived_masks_across_tile_borders_and_halos(family):
    text, offs = _borders_buffer(b" " + PROBE + b" ", (-128, 0, 192), range(len(PROBE) + 2))
    _check(family, text, offs, "probe string across tile borders and halo edges")


@pytest.mark.parametrize("family", list(FAMILIES))
def test_document_starts_around_a_tile_border(family):
    assert len(STRETCH) >= 72
    half = len(STRETCH) // 2
    text, offs = _borders_buffer(STRETCH, (0,), [half] * 71)
    starts = [b * TILE + (b - 36) for b in range(1, 72)]  # -35 .. +35 around the border
    for b, p in zip(range(1, 72), starts):
        assert b * TILE - half <= p < b * TILE - half + len(STRETCH)
    behind_apostrophe = [p for p in starts if text[p - 1:p] == b"'"]
    in_blanks = [p for p in starts if text[p - 1:p + 1] in (b"  ", b" \n", b"\n\n", b" \t", b"\r\n")]
    assert behind_apostrophe and in_blanks
    offs = sorted(set(offs) | set(starts))
    _check(family, text, offs, "document starts around tile borders")


def _deferred(text: bytes) -> int:
    tok, _ = _pair("llama4")
    tok.encode_batch(text, np.asarray([0, len(text)], dtype=np.int64))
    return tok.info(capi.TD_INFO_DEFERRED_TILES)


def _flip_of(build, lo: int, hi: int, coarse: int = 16) -> int:
    """Sweeps one-tile inputs build(c), c = lo .. hi (every coarse-th, then every one around the change): the deferred token
    tiles must be zero up to some count and two (both token tiles of the tile) from there on, changing exactly once.  -> the
    first deferred count; it and its two neighbours are compared with the reference in the three forms."""
    res = {c: _deferred(build(c)) for c in list(range(lo, hi + 1, coarse)) + [hi]}
    assert res[lo] == 0 and res[hi] == 2, (res[lo], res[hi])
    first = min(c for c, d in res.items() if d)
    res.update({c: _deferred(build(c)) for c in range(max(lo, first - coarse), first + 1)})
    seq = [res[c] for c in sorted(res)]
    assert sum(1 for x, y in zip(seq, seq[1:]) if (x != 0) != (y != 0)) == 1 and set(seq) == {0, 2}, sorted(res.items())
    first = min(c for c, d in res.items() if d)
    for c in (first - 2, first - 1, first, first + 1):
        assert len(build(c)) <= TILE
        assert _check("llama4", build(c), [0, len(build(c))], f"{c} at the cap") == (2 if c >= first else 0)
    return first


def test_piece_list_cap():
    """'1 1 1' is a piece per byte; c pieces in all, the last one a word to the end of the text.  More pieces than the list holds:
    the tile's two token tiles are deferred.  The measured corpora have at most 4612 pieces in a tile: the list
    must hold those, and it is shorter than the 5120 of the layout before."""
    def build(c):
        m = c - 1
        return (b"" if m & 1 else b" ") + b" ".join([b"1"] * ((m + 1) // 2)) + b".wwwwwwwwwwwwwwwwwwww"

    _, R = _pair("llama4")
    for c in (4611, 4612):
        assert len(R.split(build(c))) == c
    first = _flip_of(build, 4612, 5136)
    assert len(R.split(build(first))) == first


def test_cold_list_cap():
    """' abcdefghijklm' is a piece of 14 bytes: above the 12 of the exact-key table, so it is put aside for the long route.  More
    of them than that list holds: deferred.  The corpora have at most 205 such pieces in a tile."""
    def build(c):
        return b"go" + b" abcdefghijklm" * c + b" on" * ((TILE - 2 - 14 * c) // 3)

    _flip_of(build, 205, 584)


def test_heads_list_cap():
    """' aBc' is the pieces ' a' and 'Bc' behind one head that the whole-word rules leave open (the twin counts them).  Heads that
    find no room on the list are matched by the lane that found them, and the ids stay the reference's.  The corpora have at
    most 448 open heads in a tile; the sweep goes from there to above the 768 of the layout before, and takes every count where
    the list ends now.  (Whether the token phases then defer the tile is not this list's business: the START bits that
    td_probe_tiles reads for a deferred tile are the ones these heads were walked for.)"""
    def build(c):
        words = b"".join(b" " + bytes([97 + i % 26, 65 + (i // 26) % 26, 97 + (i * 7) % 26]) for i in range(c))
        return b"go" + words + b" on" * ((TILE - 2 - 4 * c) // 3)

    hs = np.zeros(TILE, dtype=np.uint8)
    H.twin_llama4().word_rules_check(build(600), None, head_state=hs)
    assert int((hs == 2).sum()) >= 600, "the builder's words are no open heads any more"
    for c in list(range(448, 780, 12)) + list(range(568, 586)):
        _check("llama4", build(c), [0, len(build(c))], f"{c} open heads")
