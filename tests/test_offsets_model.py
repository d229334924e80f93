"""CPU restatement of the per-token starts kernels (td_offsets.hip) against the brute-force truth of tests/offsets_truth.py.

The restatement follows the device: a segmented scan in chunks (chunk totals, carries into the chunks, starts), the
covered-byte bitmap derived from piece-start / skipped-stretch bitmaps as the generic engine leaves them (a stretch runs from
its bit to the next piece start; the kind in force is carried across words and 4 KiB tiles), select on it through tile and
word prefixes, and the character rank through the same two levels.  The truth places each piece's ids (whole-piece lookup,
else the merge) inside the text the piece covers by cumulative byte length."""
import numpy as np
import pytest

import helpers as H
import offsets_truth as OT

AUTOGEN = r"[a-zA-Z]+|\s+|[0-9]+|[^\w\s]"
TILE = 4096


@pytest.fixture(scope="module")
def vocab():
    pat, mr, special = H.llama4()
    table = OT.id_bytes(mr, special)
    return pat, mr, special, table, OT.id_lengths(table)


@pytest.fixture(scope="module")
def oracle(vocab):
    from oracle import port
    return port.OracleTokenizer(vocab[1])


def piece_ids(mr, O, piece: bytes):
    return [mr[piece]] if piece in mr else [int(i) for i in O.merge_piece(piece)]


# ---- the device algorithm, restated ---------------------------------------------------------------------------------------
def seg_op(x, y):
    return (x[0] | y[0], y[1] if y[0] else x[1] + y[1])


def chunked_scan(values, heads, chunk):
    """td_off_scan<0> / td_off_carry / td_off_scan<1>: exclusive segmented scan, chunk by chunk."""
    n = len(values)
    nch = (n + chunk - 1) // chunk
    agg = []
    for c in range(nch):
        r = (0, 0)
        for i in range(c * chunk, min(n, (c + 1) * chunk)):
            r = seg_op(r, (int(heads[i]), int(values[i])))
        agg.append(r)
    carry, run = [], (0, 0)
    for a in agg:
        carry.append(run[1])
        run = seg_op(run, a)
    out = np.zeros(n, dtype=np.int64)
    for c in range(nch):
        r = (0, carry[c])
        for i in range(c * chunk, min(n, (c + 1) * chunk)):
            out[i] = 0 if heads[i] else r[1]
            r = seg_op(r, (int(heads[i]), int(values[i])))
    return out


def head_bits(tok_offsets, n):
    h = np.zeros(n, dtype=bool)
    to = np.asarray(tok_offsets)
    for d in range(len(to) - 1):
        if to[d] < to[d + 1]:
            h[to[d]] = True
    return h


def engine_bitmaps(docs):
    """startbits / gapbits as the generic engine writes them: a bit at every piece start and at the start of every stretch the
    pattern skipped (gap bit set there)."""
    text, offs = H.pack_docs(docs)
    n = len(text)
    sb = np.zeros(n + 1, dtype=bool)
    gb = np.zeros(n + 1, dtype=bool)
    for d, doc in enumerate(docs):
        o0, pos = int(offs[d]), 0
        st, en = OT.split_arrays(AUTOGEN, doc)
        for s, e in zip(st.tolist(), en.tolist()):
            if s > pos:
                sb[o0 + pos] = gb[o0 + pos] = True
            sb[o0 + s] = True
            pos = e
        if pos < len(doc):
            sb[o0 + pos] = gb[o0 + pos] = True
        sb[o0 + len(doc)] = True  # (the engine marks where the last piece ended: the next document's start)
    return text, offs, sb[:n], gb[:n]


def covered_model(sb, gb):
    """td_off_rank_words / td_off_rank_tiles / td_off_cov_words: per word the kind of its last start, carried across words
    inside a tile and across tiles; a byte is covered unless the start in force is a skipped stretch."""
    n = len(sb)
    nw = (n + 31) // 32
    kinds = np.zeros(nw, dtype=np.int64)
    for w in range(nw):
        idx = np.flatnonzero(sb[w * 32:(w + 1) * 32])
        if idx.size:
            kinds[w] = 2 if gb[w * 32 + idx[-1]] else 1
    ntiles = (n + TILE - 1) // TILE
    per = TILE // 32
    tile_last = [next((int(k) for k in kinds[t * per:(t + 1) * per][::-1] if k), 0) for t in range(ntiles)]
    tile_in, cur = [], 0
    for k in tile_last:
        tile_in.append(cur)
        cur = k or cur
    cov = np.zeros(n, dtype=bool)
    for t in range(ntiles):
        state = tile_in[t]
        for w in range(t * per, min(nw, (t + 1) * per)):
            for p in range(w * 32, min(n, w * 32 + 32)):
                if sb[p]:
                    state = 2 if gb[p] else 1
                cov[p] = state != 2
    return cov


class Rank:
    """Two-level rank / select over a bitmap: prefixes per 4 KiB tile, then per word inside the tile."""

    def __init__(self, bits):
        self.bits = bits
        n = len(bits)
        nw = (n + 31) // 32
        wc = np.asarray([int(bits[w * 32:(w + 1) * 32].sum()) for w in range(nw)], dtype=np.int64)
        per = TILE // 32
        self.wpref = np.zeros(nw, dtype=np.int64)
        ntiles = (n + TILE - 1) // TILE
        self.tpref = np.zeros(ntiles + 1, dtype=np.int64)
        for t in range(ntiles):
            seg = wc[t * per:(t + 1) * per]
            self.wpref[t * per:t * per + len(seg)] = np.concatenate([[0], np.cumsum(seg)])[:-1]
            self.tpref[t + 1] = self.tpref[t] + seg.sum()

    def rank(self, p):
        w = p // 32
        return int(self.tpref[p // TILE] + self.wpref[w] + self.bits[w * 32:p].sum())

    def select(self, k):
        t = int(np.searchsorted(self.tpref, k, side="right")) - 1
        r = k - int(self.tpref[t])
        per = TILE // 32
        ws = self.wpref[t * per:(t + 1) * per]
        w = t * per + int(np.searchsorted(ws, r, side="right")) - 1
        r -= int(self.wpref[w])
        return w * 32 + int(np.flatnonzero(self.bits[w * 32:w * 32 + 32])[r])


# ---- tests ------------------------------------------------------------------------------------------------------------------
def _autogen_docs():
    rng = np.random.default_rng(5)
    words = ["snake_case", "é", "_", "__x__", "naïve", "x", "42", "!", " ", "\n", "_é_", "中文", "\U0001F600"]
    docs = ["_leading", "mid_dle", "trailing_", "____", "", "é", "", "plain 1 2"]
    docs.append("".join(words[i] + " " for i in rng.integers(0, len(words), 1500)))  # several 4 KiB tiles
    return [d.encode("utf-8") for d in docs]


def _autogen_truth(docs, mr, O, lengths):
    ids, toffs, truth = [], [0], []
    for doc in docs:
        st, en = OT.split_arrays(AUTOGEN, doc)
        dids = []
        for s, e in zip(st.tolist(), en.tolist()):
            piece_start, acc = s, 0
            for i in piece_ids(mr, O, doc[s:e]):
                truth.append(piece_start + acc)  # the token inside its piece, by cumulative byte length
                acc += int(lengths[i])
                dids.append(i)
        ids += dids
        toffs.append(len(ids))
    return np.asarray(ids, dtype=np.int64), np.asarray(toffs, dtype=np.int64), np.asarray(truth, dtype=np.int64)


def test_autogen_gaps_through_the_covered_bitmap(vocab, oracle):
    _, mr, _, _, lengths = vocab
    docs = _autogen_docs()
    ids, toffs, truth = _autogen_truth(docs, mr, oracle, lengths)
    text, offs, sb, gb = engine_bitmaps(docs)
    cov = covered_model(sb, gb)
    mask = np.zeros(len(text), dtype=bool)
    for d, doc in enumerate(docs):
        st, en = OT.split_arrays(AUTOGEN, doc)
        for s, e in zip(st.tolist(), en.tolist()):
            mask[int(offs[d]) + s:int(offs[d]) + e] = True
    assert np.array_equal(cov, mask)
    compact = chunked_scan(lengths[ids], head_bits(toffs, len(ids)), chunk=64)  # (small chunks: many chunk boundaries)
    covered_starts = OT.covered_byte_starts(ids, toffs, lengths)
    assert np.array_equal(compact, covered_starts)
    assert not np.array_equal(compact, truth), "a plain prefix sum of lengths is wrong where the pattern skips text"
    R = Rank(cov)
    got = np.empty(len(ids), dtype=np.int64)
    for d in range(len(docs)):
        o0 = int(offs[d])
        for i in range(toffs[d], toffs[d + 1]):
            got[i] = R.select(R.rank(o0) + int(compact[i])) - o0
    assert np.array_equal(got, truth)
    # characters by rank over the source text
    t = np.frombuffer(text, dtype=np.uint8)
    NC = Rank(~OT.is_cont(t))
    chars = np.empty(len(ids), dtype=np.int64)
    for d in range(len(docs)):
        o0 = int(offs[d])
        for i in range(toffs[d], toffs[d + 1]):
            p = o0 + int(got[i])
            chars[i] = max(0, NC.rank(p) - NC.rank(o0) - int(OT.is_cont(t[p:p + 1])[0]))
    assert np.array_equal(chars, OT.char_starts(text, offs, toffs, truth))


def test_chunk_boundaries_and_empty_documents(vocab):
    lengths = vocab[4]
    rng = np.random.default_rng(2)
    sizes = [0, 4095, 4096, 4097, 0, 1, 9000, 0]
    ids = rng.integers(0, 1000, sum(sizes))
    toffs = np.concatenate([[0], np.cumsum(sizes)])
    got = chunked_scan(lengths[ids], head_bits(toffs, len(ids)), chunk=4096)
    assert np.array_equal(got, OT.covered_byte_starts(ids, toffs, lengths))


def test_char_rule_and_byte_fallback(vocab):
    _, mr, special, table, lengths = vocab
    s = "héllo 中文 \U0001F600 x"
    data = s.encode("utf-8")
    # a 3-byte and a 4-byte character split into single-byte tokens
    parts = []
    for ch in s:
        b = ch.encode("utf-8")
        if len(b) > 2 and all(bytes([c]) in mr for c in b):
            parts += [bytes([c]) for c in b]
        else:
            parts.append(b)
    assert b"".join(parts) == data
    offs = OT.decode_offsets_rule(parts)
    b = np.concatenate([[0], np.cumsum([len(p) for p in parts])])[:-1]
    for p, k in zip(parts, range(len(parts))):
        if (p[0] & 0xC0) != 0x80:
            assert offs[k] == len(data[:b[k]].decode("utf-8"))
        else:  # inside a character: the character it belongs to
            assert offs[k] == len(data[:b[k]].decode("utf-8", "ignore"))
    ct = np.asarray([sum(1 for c in x if not 0x80 <= c < 0xC0) * 2 + (0x80 <= x[0] < 0xC0) if x else 0 for x in table])
    ids = [mr[p] for p in parts]
    vals = ct[ids] >> 1
    got = chunked_scan(vals, head_bits([0, len(ids)], len(ids)), chunk=3)
    got = np.maximum(got - (ct[ids] & 1), 0)
    assert list(got) == offs
    assert list(got) == list(OT.char_starts(data, [0, len(data)], [0, len(ids)], b))


def test_allowed_specials_stitching(vocab, oracle):
    _, mr, special, table, lengths = vocab
    name = sorted(special)[0]
    doc = f"ab{name}c é{name}".encode("utf-8")
    lit = name.encode("utf-8")
    # segments between the specials, their ids and where they stand
    segs, pos = [], 0
    while True:
        q = doc.find(lit, pos)
        segs.append((pos, q if q >= 0 else len(doc)))
        if q < 0:
            break
        pos = q + len(lit)
    ids, starts = [], []
    for k, (s, e) in enumerate(segs):
        seg_ids = [int(i) for i in oracle.encode(doc[s:e])] if e > s else []
        rel = OT.covered_byte_starts(seg_ids, [0, len(seg_ids)], lengths)
        ids += seg_ids
        starts += [int(r) + s for r in rel]  # shifted by where the segment stands
        if k + 1 < len(segs):
            ids.append(special[name])
            starts.append(e)
    truth = OT.covered_byte_starts(ids, [0, len(ids)], lengths)  # the special's bytes are its literal: covered rule
    assert starts == list(truth)
    for i, st in zip(ids, starts):
        assert doc[st:st + len(table[i])] == table[i]


def test_the_surface_exists_without_a_gpu():
    """The C ABI exports the starts entry points and the Python layers carry the methods (no device needed to check)."""
    from tokendagger_amd import capi, wrapper
    from tokendagger_amd import _tokendagger_core as core
    lib = capi.load_library()
    for name in ("td_token_starts", "td_token_starts_device", "td_encode_batch_with_starts", "td_encode_device_with_starts"):
        assert hasattr(lib, name)
    for name in ("encode_with_offsets", "encode_batch_to_numpy_with_offsets", "decode_with_offsets"):
        assert callable(getattr(wrapper.Tokenizer, name))
    for name in ("encode_with_starts", "encode_batch_numpy_with_starts", "token_starts"):
        assert hasattr(core.CoreBPE, name)
    for name in ("token_starts", "token_starts_device", "encode_batch_with_starts", "encode_device_with_starts"):
        assert callable(getattr(capi.HipTokenizer, name))
