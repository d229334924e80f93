"""Decode at its seams: td_decode_len / td_decode_chunks / td_decode_copy / td_decode_doc_offsets (chunks of 4096 ids, an LDS window of
32 752 bytes per pass, 1024 chunk totals per trip of the chunk scan) and td_small_decode (1024 ids, 16 384 bytes), both forms.

Truth: decode_rows_truth.decode_numpy over the vocabulary's bytes (a vectorised numpy gather of the same bytes for the 4 M id case,
checked against it here); for the error cases the compiled reference's decode_bytes (the reference's src/tiktoken/tiktoken.cpp:236-255),
which must raise where the product does.  Device outputs lie inside larger tensors filled with 0xFF, 64 guard bytes on both sides that
must stay untouched.  "Answered by the kernel" / "handed back" are assertions on TD_INFO_SMALL_DECODES / TD_INFO_SMALL_DECODE_HANDBACKS."""
from __future__ import annotations

import ctypes
import re

import numpy as np
import pytest

import decode_rows_truth as dt
import helpers as H
from oracle import ref
from tokendagger_amd import capi

pytestmark = pytest.mark.gpu

GUARD = 64
CHUNK, WINDOW = 4096, 32768 - 16  # ids per workgroup of td_decode_copy; bytes per pass of its LDS window
INT32_MIN = -(2 ** 31)
E_CAPACITY, E_BAD_TOKEN = capi.TD_E_CAPACITY, capi.TD_E_BAD_TOKEN


@pytest.fixture(scope="module")
def tok():
    pat, mr, special = H.llama4()
    t = capi.HipTokenizer(pat, mr, special, device=0)
    yield t
    t.close()


@pytest.fixture(scope="module")
def V():
    """The vocabulary's bytes by id, specials included (decode_rows_truth.Vocab: lens, begin, blob)."""
    _, mr, special = H.llama4()
    by_id = {r: b for b, r in mr.items()}
    by_id.update({i: s.encode() for s, i in special.items()})
    v = dt.Vocab(by_id)
    assert (v.lens > 0).all(), "the Llama-4 ids have no holes"
    return v


def _gather(V, ids) -> bytes:
    """The bytes of valid ids, vectorised (the large case)."""
    ids = np.asarray(ids, dtype=np.int64)
    ln = V.lens[ids]
    start = np.cumsum(ln) - ln
    src = np.repeat(V.begin[ids] - start, ln) + np.arange(int(ln.sum()), dtype=np.int64)
    return V.blob[src].tobytes()


def _truth(V, ids, offs=None):
    offs = np.asarray([0, len(ids)], dtype=np.int64) if offs is None else offs
    out, bo, _, _ = dt.decode_numpy(ids, V, tok_offsets=offs)
    return out, bo


def _stream() -> int:
    import torch
    return torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream


def _device(tok, ids, tok_shift: int = 0, out_shift: int = 0, capacity: int | None = None, room: int | None = None):
    """td_decode_device with d_tokens `tok_shift` bytes and d_out `out_shift` bytes behind a 16-byte boundary, the output inside a
    tensor of 0xFF.  -> (status code, err_pos, n_bytes, the `room` bytes from d_out on); the guards are checked here."""
    import torch
    dev = torch.device("cuda", 0)
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    assert tok_shift % 4 == 0 and 0 <= tok_shift < 16 and 0 <= out_shift < 16
    d_ids = torch.full((len(ids) + 8,), -7, dtype=torch.int32, device=dev)
    d_ids[tok_shift // 4: tok_shift // 4 + len(ids)] = torch.from_numpy(ids).to(dev)
    room = capacity if room is None else room
    out = torch.full((GUARD + 16 + room + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    nb = torch.full((3,), -1, dtype=torch.int64, device=dev)
    assert d_ids.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    at = GUARD + out_shift
    s = _stream()
    tok.decode_device(d_ids.data_ptr() + tok_shift, len(ids), out.data_ptr() + at, capacity, nb.data_ptr() + 8, s)
    rc, pos = tok.device_status_pos(s)
    o, n = out.cpu().numpy(), nb.cpu().numpy()
    assert (o[:at] == 0xFF).all() and (o[at + room:] == 0xFF).all() and n[0] == -1 and n[2] == -1, "a guard was written"
    return rc, pos, int(n[1]), o[at:at + room]


def _dcounters(tok):
    return tok.info(capi.TD_INFO_SMALL_DECODES), tok.info(capi.TD_INFO_SMALL_DECODE_HANDBACKS)


def _random_ids(V, rng, n):
    return rng.integers(0, V.max_id + 1, size=n).astype(np.int32)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4095, 4096, 4097, 8191, 8192, 8193])
def test_alignment_and_chunk_edges(tok, V, n):
    """d_tokens at byte offsets 0 / 4 / 8 / 12 (16-byte loads only at 0: the scalar branches), d_out at 0 / 1 / 7 / 15 (the window's
    shift, head and tail stores), capacity exact."""
    rng = np.random.default_rng(100 + n)
    ids = _random_ids(V, rng, n)
    want, _ = _truth(V, ids)
    assert want == _gather(V, ids)
    for tok_shift in (0, 4, 8, 12):
        for out_shift in (0, 1, 7, 15):
            rc, _, nb, got = _device(tok, ids, tok_shift, out_shift, capacity=len(want))
            assert rc == 0 and nb == len(want) and got.tobytes() == want, (n, tok_shift, out_shift)


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def windows_case(V):
    """Three chunks: 4096 short ids with an odd byte total (the next chunk's base is odd), 4096 ids of tokens of 17..113 bytes whose bytes
    take three passes of the window with a token across each seam, and a partial chunk of long tokens."""
    rng = np.random.default_rng(7)
    ids_all = np.arange(V.max_id + 1)
    short = ids_all[V.lens <= 3]
    mid = ids_all[(V.lens >= 17) & (V.lens <= 20)]
    longest = ids_all[V.lens >= 65]
    a = rng.choice(short, CHUNK)
    if V.lens[a].sum() % 2 == 0:
        a[0] = short[V.lens[short] == (2 if V.lens[a[0]] != 2 else 1)][0]
    b = rng.choice(mid, CHUNK)
    b[rng.choice(CHUNK, len(longest), replace=False)] = longest  # (74 tokens of 65..113 bytes)
    c = rng.choice(ids_all[V.lens >= 17], 1500)
    assert V.lens[a].sum() % 2 == 1
    local = np.cumsum(V.lens[b])
    assert 2 * WINDOW < local[-1] <= 3 * WINDOW, "three passes of the window"
    assert WINDOW not in local and 2 * WINDOW not in local, "a token lies across each seam of the window"
    assert V.lens[b].min() >= 17 and V.lens[b].max() == 113
    ids = np.concatenate([a, b, c]).astype(np.int32)
    return ids, _truth(V, ids)[0]


def test_several_windows_at_an_unaligned_chunk_base(tok, V, windows_case):
    ids, want = windows_case
    for out_shift in (0, 5):
        rc, _, nb, got = _device(tok, ids, 0, out_shift, capacity=len(want))
        assert rc == 0 and nb == len(want) and got.tobytes() == want, out_shift
    rc, _, nb, got = _device(tok, ids, 8, 3, capacity=len(want) + 100, room=len(want) + 100)
    assert rc == 0 and nb == len(want) and got[:len(want)].tobytes() == want and (got[len(want):] == 0xFF).all()
    assert tok.decode_bytes(ids) == want
    offs = np.asarray([0, 0, 17, CHUNK - 1, CHUNK + 1, 2 * CHUNK, 2 * CHUNK, len(ids) - 1, len(ids)], dtype=np.int64)
    got, bo = tok.decode_batch(ids, offs)
    assert got == want and np.array_equal(bo, _truth(V, ids, offs)[1])


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
def test_more_than_1024_chunks(tok, V):
    """1025 * 4096 + 5 ids: td_decode_chunks' loop makes a second trip; more than 1 048 576 documents: td_decode_doc_offsets' too."""
    rng = np.random.default_rng(3)
    n = 1025 * CHUNK + 5
    small = np.arange(V.max_id + 1)[V.lens <= 2]
    ids = rng.choice(small, n).astype(np.int32)
    want = _gather(V, ids)
    k = 5000
    assert _gather(V, ids[-k:]) == _truth(V, ids[-k:])[0], "the gather is decode_numpy's"
    lens = V.lens[ids]
    assert len(want) == lens.sum() and 6_000_000 < len(want) < 9_000_000
    rc, _, nb, got = _device(tok, ids, 0, 9, capacity=len(want))
    assert rc == 0 and nb == len(want)
    assert got.tobytes() == want
    got, bo = tok.decode_batch(ids, np.asarray([0, n], dtype=np.int64))
    assert got == want and bo.tolist() == [0, len(want)]
    # documents of 0 or 1 ids
    offs = np.sort(np.concatenate([np.arange(n + 1), rng.integers(0, n + 1, size=20_000), [0, 0, n, n]])).astype(np.int64)
    assert len(offs) - 1 > 1_048_576 and (np.diff(offs) <= 1).all() and (np.diff(offs) == 0).sum() > 20_000
    got, bo = tok.decode_batch(ids, offs)
    byte_at = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert got == want and np.array_equal(bo, byte_at[offs])


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
def test_document_offsets_at_chunk_seams(tok, V):
    rng = np.random.default_rng(4)
    ids = _random_ids(V, rng, 12_000)
    n = len(ids)
    for offs in ([0, 0, 0, 7, CHUNK, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK, 2 * CHUNK, n, n, n], [0, n], [0, CHUNK, 2 * CHUNK, n],
                 [0, 0, n], [0, n, n]):
        offs = np.asarray(offs, dtype=np.int64)
        want, wo = _truth(V, ids, offs)
        got, bo = tok.decode_batch(ids, offs)
        assert np.array_equal(bo, wo) and got == want, offs.tolist()
    got, bo = tok.decode_batch(np.zeros(0, dtype=np.int32), np.zeros(6, dtype=np.int64))  # every document empty
    assert got == b"" and bo.tolist() == [0] * 6
    got, bo = tok.decode_batch(ids[:5], np.asarray([0, 0, 5, 5], dtype=np.int64))  # (1024 ids and fewer: td_decode_batch has no small form)
    assert got == _truth(V, ids[:5])[0] and bo.tolist() == [0, 0, len(got), len(got)]


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------
def _raises_bad_token(fn, bad_id: int):
    with pytest.raises(capi.TokenDaggerHipError) as e:
        fn()
    assert e.value.code == E_BAD_TOKEN and re.search(rf"Invalid token for decoding: {bad_id}(?!\d)", str(e.value)), str(e.value)


def test_the_lowest_bad_index_wins(tok, V):
    R = H.ref_tokenizer()
    rng = np.random.default_rng(5)
    good = _random_ids(V, rng, 12_000)
    bads = [V.max_id + 1, -1, INT32_MIN]
    for rot in range(3):  # every bad value once at the lowest index
        ids = good.copy()
        where = {5: bads[rot], CHUNK: bads[(rot + 1) % 3], 9000: bads[(rot + 2) % 3]}
        for i, v in where.items():
            ids[i] = v
        _raises_bad_token(lambda: tok.decode_bytes(ids), where[5])
        _raises_bad_token(lambda: tok.decode_batch(ids, np.asarray([0, 3, len(ids)], dtype=np.int64)), where[5])
        with pytest.raises(ref.RefError, match=f"Invalid token for decoding: {where[5]}$"):
            R.decode_bytes(ids)
        rc, pos, _, _ = _device(tok, ids, 4 * rot, rot, capacity=1 << 20)
        assert (rc, pos) == (E_BAD_TOKEN, 5), (rot, rc, pos)
        ids[5] = good[5]  # the lowest is in the second chunk now, the other one behind it in the third
        _raises_bad_token(lambda: tok.decode_bytes(ids), where[CHUNK])
        rc, pos, _, _ = _device(tok, ids, 0, 0, capacity=1 << 20)
        assert (rc, pos) == (E_BAD_TOKEN, CHUNK)
    for bad in bads:  # only the last id
        for n in (12_000, 700):
            ids = good[:n].copy()
            ids[-1] = bad
            _raises_bad_token(lambda: tok.decode_bytes(ids), bad)
            with pytest.raises(ref.RefError, match=f"Invalid token for decoding: {bad}$"):
                R.decode_bytes(ids)
            rc, pos, _, _ = _device(tok, ids, 0, 0, capacity=1 << 20)
            assert (rc, pos) == (E_BAD_TOKEN, n - 1)
    assert tok.decode_bytes(good) == _truth(V, good)[0], "the handle answers the next call"


def test_ids_in_the_holes_of_a_vocabulary_raise():
    toy = {bytes([i]): i for i in range(256)}
    toy[b"ab"] = 300
    pat, _, _ = H.llama4()
    Rt = ref.RefTokenizer(pat, toy, {})
    t = capi.HipTokenizer(pat, toy, {}, device=0)
    try:
        assert t.info(capi.TD_INFO_MAX_ID) == 300
        for n in (8, 3000):  # td_small_decode and the general path
            base = np.asarray([97, 300, 255, 0] * (n // 4), dtype=np.int32)
            assert t.decode_bytes(base) == Rt.decode_bytes(base) == b"aab\xff\x00" * (n // 4)
            for hole in (256, 257, 299, 301):
                ids = base.copy()
                ids[n - 2] = hole
                _raises_bad_token(lambda: t.decode_bytes(ids), hole)
                with pytest.raises(ref.RefError, match=f"Invalid token for decoding: {hole}$"):
                    Rt.decode_bytes(ids)
    finally:
        t.close()


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------
def test_capacity_at_the_total_and_one_below(tok, V):
    rng = np.random.default_rng(6)
    for n in (700, 9000):  # (td_decode_bytes: the one-launch path and the general one)
        ids = _random_ids(V, rng, n)
        want, _ = _truth(V, ids)
        total = len(want)
        rc, _, nb, got = _device(tok, ids, 0, 3, capacity=total)
        assert rc == 0 and nb == total and got.tobytes() == want
        for cap in (total - 1, 0):
            rc, pos, nb, got = _device(tok, ids, 0, 3, capacity=cap, room=total)
            assert rc == E_CAPACITY and nb == total and pos == total, (n, cap, rc, nb, pos)
            assert (got[cap:] == 0xFF).all(), "nothing is written at or behind the capacity given"
        offs = np.asarray([0, 1, n // 2, n], dtype=np.int64)
        bo_want = _truth(V, ids, offs)[1]
        for form in ("bytes", "batch"):
            for small in (1, 0):
                tok.set_option(capi.TD_OPT_SMALL_PATH, small)
                try:
                    for cap in (total, total - 1, 0):
                        out = np.full(total + 64, 0xFF, dtype=np.uint8)
                        nb = ctypes.c_int64(-1)
                        before = _dcounters(tok)
                        if form == "bytes":
                            rc = tok._lib.td_decode_bytes(tok._h, ids.ctypes.data, n, out.ctypes.data, cap, ctypes.byref(nb))
                        else:
                            bo = np.full(len(offs), -1, dtype=np.int64)
                            rc = tok._lib.td_decode_batch(tok._h, ids.ctypes.data, offs.ctypes.data, len(offs) - 1, out.ctypes.data, cap,
                                                          bo.ctypes.data, ctypes.byref(nb))
                        moved = tuple(x - y for x, y in zip(_dcounters(tok), before))
                        assert moved == ((1, 0) if form == "bytes" and small and n <= 1024 else (0, 0)), (form, small, n, moved)
                        assert nb.value == total, (form, small, n, cap)
                        if cap == total:
                            assert rc == 0 and out[:total].tobytes() == want and (out[total:] == 0xFF).all()
                            assert form == "bytes" or np.array_equal(bo, bo_want)
                        else:
                            assert rc == E_CAPACITY and (out[cap:] == 0xFF).all(), (form, small, n, cap, rc)
                finally:
                    tok.set_option(capi.TD_OPT_SMALL_PATH, 1)


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------------
def test_small_decode_at_16384_bytes(tok, V):
    rng = np.random.default_rng(8)
    ids_all = np.arange(V.max_id + 1)
    of = {k: ids_all[V.lens == k] for k in (15, 16, 17)}
    full = rng.choice(of[16], 1024).astype(np.int32)

    def run(ids, moved):
        """One td_decode_bytes call with the exact capacity (no guess of the binding's, no second call)."""
        want = _truth(V, ids)[0]
        out = np.full(len(want) + 64, 0xFF, dtype=np.uint8)
        nb = ctypes.c_int64(-1)
        before = _dcounters(tok)
        rc = tok._lib.td_decode_bytes(tok._h, ids.ctypes.data, len(ids), out.ctypes.data, len(want), ctypes.byref(nb))
        after = _dcounters(tok)
        assert (after[0] - before[0], after[1] - before[1]) == moved, (after, before, moved)
        assert rc == 0 and nb.value == len(want) and out[:len(want)].tobytes() == want and (out[len(want):] == 0xFF).all()
        return want

    assert len(run(full, (1, 0))) == 16384           # answered by the kernel
    over = full.copy()
    over[rng.integers(0, 1024)] = of[17][3]
    assert len(run(over, (0, 1))) == 16385           # handed back
    under = full.copy()
    under[rng.integers(0, 1024)] = of[15][3]
    assert len(run(under, (1, 0))) == 16383
    run(np.concatenate([full, full[:1]]), (0, 0))    # 1025 ids: the kernel is not asked
    bad = full.copy()
    bad[700], bad[3] = V.max_id + 5, -9
    for small in (1, 0):
        tok.set_option(capi.TD_OPT_SMALL_PATH, small)
        try:
            before = _dcounters(tok)
            _raises_bad_token(lambda: tok.decode_bytes(bad), -9)
            assert tuple(x - y for x, y in zip(_dcounters(tok), before)) == ((1, 0) if small else (0, 0)), "an error the kernel reports is its answer"
        finally:
            tok.set_option(capi.TD_OPT_SMALL_PATH, 1)
    with pytest.raises(ref.RefError, match="Invalid token for decoding: -9$"):
        H.ref_tokenizer().decode_bytes(bad)
