"""Decode rows on the GPU (td_decode_rows.hip) against tests/decode_rows_truth.py: exact comparisons throughout.  The contract is
the section "decode rows" of include/tokendagger_hip.h; every error is a status code, no case makes the device fault.  In the
device form every output lies inside a larger FILL-filled tensor whose guards must stay untouched."""
import numpy as np
import pytest

import decode_rows_truth as dt
import helpers as H
from tokendagger_amd import capi
from tokendagger_amd.capi import decode_spec  # noqa: F401  (the feature under test: without it nothing here runs)

pytestmark = pytest.mark.gpu

TILE = 4096
FILL = 0x5A          # bytes around `out`
FILL64 = -7777       # the guard elements around out_offsets, seg_ids and info
GUARD = 64


@pytest.fixture(scope="module")
def tok():
    pat, mr, special = H.llama4()
    return capi.HipTokenizer(pat, mr, special, device=0)


@pytest.fixture(scope="module")
def voc():
    """The Llama-4 test vocabulary as the truths take it, computed once: (dict id -> bytes, Vocab, sorted special ids)."""
    pat, mr, special = H.llama4()
    t = {r: b for b, r in mr.items()}
    return t, dt.Vocab(t), sorted(special.values())


@pytest.fixture(scope="module")
def golden_truth(golden, voc):
    ids, offs = golden["enc"].astype(np.int32), golden["enc_offsets"].astype(np.int64)
    assert len(ids) == 828407 and len(offs) - 1 == 3335 and int(np.diff(offs).max()) == 263300
    return ids, offs, dt.decode_numpy(ids, voc[1], tok_offsets=offs)


def _spec(kw):
    return decode_spec(kw.get("row_stride", 0), kw.get("skip", ()), kw.get("stop", ()), keep_stop=kw.get("keep_stop", False),
                       skip_negative=kw.get("skip_negative", False), skip_special=kw.get("skip_special", False))


def _call_kw(kw):
    return {k: kw[k] for k in ("tok_offsets", "lengths", "n_segs") if k in kw}


def _same(got, want, what=""):
    assert got[0] == want[0], what
    for x, y in zip(got[1:4], want[1:4]):
        assert np.array_equal(np.asarray(x, dtype=np.int64), y), (what, x, y)


def _host(tok, ids, want, what="", **kw):
    got = tok.decode_rows(ids, _spec(kw), **_call_kw(kw))
    _same(got, want, what)
    return got


def _device(tok, ids, want_bytes, ids_shift=0, out_shift=0, capacity=None, null_out=False, stream=None, **kw):
    """td_decode_rows_device on uploaded buffers -> (bytes | None, offs, seg_ids, info, guards untouched, (code, pos)).  capacity
    None: want_bytes (the truth's byte count).  ids_shift / out_shift: the pointers are advanced off the 16-byte grid."""
    import torch
    dev = torch.device("cuda", 0)
    ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    rows = kw.get("row_stride", 0) > 0
    d_ids = torch.from_numpy(np.concatenate([np.full(ids_shift, 12345, dtype=np.int32), ids])).to(dev)
    assert d_ids.data_ptr() % 16 == 0
    o = None if rows else np.ascontiguousarray(kw["tok_offsets"], dtype=np.int64)
    ln = np.ascontiguousarray(kw["lengths"], dtype=np.int32) if rows and kw.get("lengths") is not None else None
    n = len(o) - 1 if o is not None else (len(ln) if ln is not None else kw["n_segs"])
    d_o = torch.from_numpy(o).to(dev) if o is not None else None
    d_ln = torch.from_numpy(ln).to(dev) if ln is not None and len(ln) else None
    cap = want_bytes if capacity is None else capacity
    d_out = torch.full((cap + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device=dev)
    assert d_out.data_ptr() % 16 == 0
    d_offs = torch.full((n + 1 + 2 * GUARD,), FILL64, dtype=torch.int64, device=dev)
    d_seg = torch.full((n + 2 * GUARD,), FILL64, dtype=torch.int64, device=dev)
    d_info = torch.full((4 + 2 * GUARD,), FILL64, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    rc = tok.decode_rows_device(d_ids.data_ptr() + 4 * ids_shift if len(ids) else 0, len(ids), d_o.data_ptr() if d_o is not None else 0,
                                d_ln.data_ptr() if d_ln is not None else 0, n, _spec(kw), 0 if null_out else d_out.data_ptr() + GUARD + out_shift,
                                0 if null_out else cap, d_offs.data_ptr() + 8 * GUARD, d_seg.data_ptr() + 8 * GUARD, d_info.data_ptr() + 8 * GUARD, s)
    assert rc is None  # (nothing comes back but through device_status)
    status = tok.device_status_pos(s)
    out, offs, seg, info = d_out.cpu().numpy(), d_offs.cpu().numpy(), d_seg.cpu().numpy(), d_info.cpu().numpy()
    a = GUARD + out_shift
    wrote = 0 if (null_out or status[0] == capi.TD_E_CAPACITY) else min(cap, max(int(info[GUARD]), 0))
    guards = bool((out[:a] == FILL).all() and (out[a + wrote:] == FILL).all() and (offs[:GUARD] == FILL64).all() and
                  (offs[GUARD + n + 1:] == FILL64).all() and (seg[:GUARD] == FILL64).all() and (seg[GUARD + n:] == FILL64).all() and
                  (info[:GUARD] == FILL64).all() and (info[GUARD + 4:] == FILL64).all())
    return out[a:a + wrote].tobytes(), offs[GUARD:GUARD + n + 1], seg[GUARD:GUARD + n], info[GUARD:GUARD + 4], guards, status


def _device_ok(tok, ids, want, what="", **kw):
    got = _device(tok, ids, len(want[0]), **kw)
    assert got[5][0] == capi.TD_OK and got[4], (what, got[5], got[4])
    _same(got, want, what)
    return got


def _both(tok, voc, ids, what="", **kw):
    """Host and device forms against the numpy truth (computed once per case)."""
    want = dt.decode_numpy(np.asarray(ids).reshape(-1), voc[1], special_ids=voc[2], **kw)
    _host(tok, ids, want, what, **kw)
    _device_ok(tok, ids, want, what, **kw)
    return want


# ---- the golden ids ---------------------------------------------------------------------------------------------------------------

def test_golden_ids_plain_spec(tok, golden, golden_truth):
    ids, offs, want = golden_truth
    assert want[0] == golden["text"].tobytes() and np.array_equal(want[1], golden["offsets"].astype(np.int64))
    old = tok.decode_batch(ids, offs)
    assert old[0] == want[0] and np.array_equal(old[1], want[1])
    _host(tok, ids, want, tok_offsets=offs)
    got = _device_ok(tok, ids, want, tok_offsets=offs)
    assert got[3].tolist() == [len(want[0]), len(ids), 0, 0] and np.array_equal(got[2], np.diff(offs))


@pytest.mark.parametrize("ids_shift,out_shift", [(1, 1), (2, 7), (3, 15)])
def test_golden_ids_off_the_16_byte_grid(tok, golden_truth, ids_shift, out_shift):
    ids, offs, want = golden_truth
    _device_ok(tok, ids, want, tok_offsets=offs, ids_shift=ids_shift, out_shift=out_shift)


# ---- a stop carried across tiles -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("at", [10, 4095, 4096, 3 * TILE + 4])
def test_stop_carried_across_tiles(tok, voc, at):
    n = 3 * TILE + 5
    rng = np.random.default_rng(at)
    eos = voc[2][1]
    ids = rng.integers(1000, 100000, size=n).astype(np.int32)
    ids[at] = eos
    junk = np.asarray([voc[1].max_id + 50, -1, 2**31 - 1, -100, voc[1].max_id + 1], dtype=np.int32)
    ids[at + 1:] = junk[np.arange(n - at - 1) % len(junk)]
    kw = dict(tok_offsets=np.asarray([0, n], dtype=np.int64), stop=[eos])
    want = _both(tok, voc, ids, **kw)
    assert want[2].tolist() == [at + 1] and want[3].tolist() == [len(want[0]), at, 1, 1]
    assert want[0] == b"".join(voc[0][int(x)] for x in ids[:at])


# ---- tile edges -------------------------------------------------------------------------------------------------------------------

def test_segments_on_tile_edges(tok, voc):
    rng = np.random.default_rng(3)
    offs = np.asarray([0, 4095, 4096, 4097, 2 * TILE - 1, 2 * TILE, 2 * TILE, 2 * TILE + 1, 3 * TILE, 4 * TILE + 1, 4 * TILE + 1], dtype=np.int64)
    ids = rng.integers(1000, 100000, size=int(offs[-1]) + 3).astype(np.int32)
    eos = voc[2][1]
    _both(tok, voc, ids, tok_offsets=offs)
    ids[[4094, 4096, 2 * TILE - 1, 3 * TILE - 1, 3 * TILE]] = eos  # stops on the last, only and first positions around the edges
    _both(tok, voc, ids, tok_offsets=offs, stop=[eos])
    _both(tok, voc, ids, tok_offsets=offs, stop=[eos], keep_stop=True)
    _both(tok, voc, ids, tok_offsets=offs[2:-2] + 0, stop=[eos])  # tok_offsets[0] > 0, ids behind the last segment


def test_tiles_without_a_live_byte(tok, voc):
    rng = np.random.default_rng(4)
    pad = voc[1].max_id + 1
    ids = rng.integers(1000, 100000, size=5 * TILE).astype(np.int32)
    ids[TILE:2 * TILE] = pad                      # a tile whose every id is skipped
    ids[3 * TILE:4 * TILE] = -100                 # ... and one of negative ids
    kw = dict(skip=[pad], skip_negative=True)
    _both(tok, voc, ids, tok_offsets=np.asarray([0, 5 * TILE], dtype=np.int64), **kw)
    _both(tok, voc, ids, tok_offsets=np.asarray([0, TILE + 7, 2 * TILE - 7, 5 * TILE], dtype=np.int64), **kw)
    # a tile behind a stop, between two live tiles: the stop at the end of tile 0, the next segment starts with tile 2
    eos = voc[2][1]
    ids[TILE - 1] = eos
    want = _both(tok, voc, ids, tok_offsets=np.asarray([0, 2 * TILE, 5 * TILE], dtype=np.int64), stop=[eos], **kw)
    assert want[2].tolist() == [TILE, 3 * TILE]


# ---- empty segments and empty calls -----------------------------------------------------------------------------------------------

def test_runs_of_empty_segments(tok, voc):
    ids = np.asarray([1234, 5678, 91011], dtype=np.int32)
    front = np.concatenate([np.zeros(5001, dtype=np.int64), [1, 3]])      # 5000 empty segments in front of one id
    want = _both(tok, voc, ids, tok_offsets=front)
    assert want[1][:5001].tolist() == [0] * 5001 and want[2][:5000].sum() == 0
    behind = np.concatenate([[0, 2], np.full(5001, 3, dtype=np.int64)])   # ... and 5000 behind the last id
    want = _both(tok, voc, ids, tok_offsets=behind)
    assert (want[1][2:] == len(want[0])).all()
    _both(tok, voc, ids, tok_offsets=np.asarray([2, 2, 2, 2], dtype=np.int64))  # nothing visited, offsets above 0


def test_empty_calls(tok, voc):
    ids = np.asarray([1234, 5678], dtype=np.int32)
    none = np.zeros(0, dtype=np.int32)
    _both(tok, voc, ids, tok_offsets=np.asarray([1], dtype=np.int64))            # n_segs == 0
    _both(tok, voc, none, tok_offsets=np.asarray([0], dtype=np.int64))           # ... and n_tokens == 0
    _both(tok, voc, none, tok_offsets=np.asarray([0, 0, 0], dtype=np.int64))     # n_tokens == 0 with segments
    _both(tok, voc, none, row_stride=5, n_segs=0)
    _both(tok, voc, none, row_stride=5, n_segs=0, lengths=np.zeros(0, dtype=np.int32))


# ---- window passes ----------------------------------------------------------------------------------------------------------------

def test_window_passes(tok, voc):
    lens = voc[1].lens
    longest = int(np.argmax(lens))
    assert int(lens[longest]) == 113
    ids = np.full(TILE, longest, dtype=np.int32)
    want = _both(tok, voc, ids, tok_offsets=np.asarray([0, TILE], dtype=np.int64))
    assert len(want[0]) == 113 * TILE  # about 463 KB from one tile
    long_ids = np.flatnonzero(lens >= 16)
    assert len(long_ids) == 7659
    ids = np.random.default_rng(6).choice(long_ids, size=2 * TILE).astype(np.int32)
    want = dt.decode_numpy(ids, voc[1], tok_offsets=np.asarray([0, 100, 2 * TILE], dtype=np.int64))
    _host(tok, ids, want, tok_offsets=np.asarray([0, 100, 2 * TILE], dtype=np.int64))
    for shift in (0, 5):
        _device_ok(tok, ids, want, tok_offsets=np.asarray([0, 100, 2 * TILE], dtype=np.int64), out_shift=shift)


# ---- rows form --------------------------------------------------------------------------------------------------------------------

def test_rows_with_every_length(tok, voc):
    rng = np.random.default_rng(7)
    ids = rng.integers(1000, 100000, size=(37, 19)).astype(np.int32)
    lengths = (np.arange(37) % 20).astype(np.int32)
    for r in range(37):
        ids[r, lengths[r]:] = [-1, voc[1].max_id + 9][r % 2]  # what lies behind a row's length is never looked at
    want = _both(tok, voc, ids, row_stride=19, lengths=lengths)
    assert want[2].tolist() == lengths.tolist()
    full = rng.integers(1000, 100000, size=(37, 19)).astype(np.int32)
    _both(tok, voc, full, row_stride=19, n_segs=37)  # no lengths: every row is whole


def test_rows_of_a_tile_and_of_one_id(tok, voc):
    rng = np.random.default_rng(8)
    eos = voc[2][1]
    ids = rng.integers(1000, 100000, size=(4, TILE)).astype(np.int32)
    ids[1, 17] = ids[2, TILE - 1] = ids[3, 0] = eos
    want = _both(tok, voc, ids, row_stride=TILE, n_segs=4, stop=[eos])
    assert want[2].tolist() == [TILE, 18, TILE, 1]
    ids = rng.integers(1000, 100000, size=(TILE, 1)).astype(np.int32)
    lengths = (np.arange(TILE) % 3 != 0).astype(np.int32)
    _both(tok, voc, ids, row_stride=1, lengths=lengths)


@pytest.fixture(scope="module")
def generation(voc):
    """An [8, 300] batch as a model leaves it: BOS, prompt, completion, one EOS, then padding with n_vocab; row 7 never stops."""
    rng = np.random.default_rng(9)
    bos, eos, pad = voc[2][0], voc[2][1], voc[1].max_id + 1
    batch = np.full((8, 300), pad, dtype=np.int32)
    cut = []
    for r in range(8):
        n = [5, 40, 120, 299, 1, 77, 200, 300][r]
        row = rng.integers(1000, 100000, size=n).astype(np.int32)
        row[0] = bos
        if r < 7:
            row[-1] = eos
        batch[r, :n] = row
        cut.append([int(x) for x in row if x not in (bos, eos, pad)])
    return batch, cut, bos, eos, pad


def test_generation_batch(tok, voc, generation):
    batch, cut, bos, eos, pad = generation
    want = _both(tok, voc, batch, row_stride=300, n_segs=8, skip=[pad, bos], stop=[eos])
    assert [want[0][want[1][r]:want[1][r + 1]] for r in range(8)] == [b"".join(voc[0][x] for x in row) for row in cut]
    assert want[2].tolist() == [5, 40, 120, 299, 1, 77, 200, 300] and want[3][3] == 7
    kept = _both(tok, voc, batch, row_stride=300, n_segs=8, skip=[pad, bos], stop=[eos], keep_stop=True)
    assert len(kept[0]) == len(want[0]) + 7 * len(voc[0][eos])
    # TD_DECODE_SKIP_SPECIAL is the list of the vocabulary's special ids
    a = _both(tok, voc, batch, row_stride=300, n_segs=8, skip=[pad], stop=[eos], skip_special=True)
    b = _both(tok, voc, batch, row_stride=300, n_segs=8, skip=[pad] + voc[2], stop=[eos])
    _same(a, b)
    _same(a, want)


def test_python_decode_rows(voc, generation):
    import tokendagger as tiktoken
    batch, cut, bos, eos, pad = generation
    pat, mr, special = H.llama4()
    enc = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    assert enc.decode_rows(batch, skip=[pad, bos], stop=[eos]) == [enc.decode(row) for row in cut]
    r = enc.decode_rows_to_numpy(batch, skip=[pad, bos], stop=[eos])
    assert r.seg_ids.tolist() == [5, 40, 120, 299, 1, 77, 200, 300] and r.n_stopped == 7 and r.offsets[-1] == len(r.data)
    flat = np.concatenate([np.asarray(row, dtype=np.int32) for row in cut])
    offs = np.concatenate([[0], np.cumsum([len(row) for row in cut])]).astype(np.int64)
    assert enc.decode_rows(flat, tok_offsets=offs) == [enc.decode(row) for row in cut]
    with pytest.raises(tiktoken.TokenDaggerError):
        enc.decode_rows(batch)  # the padding is no token
    with pytest.raises(tiktoken.TokenDaggerError):
        enc.decode_rows(flat)


# ---- a label stream ---------------------------------------------------------------------------------------------------------------

def test_label_stream(tok, golden, golden_truth, voc):
    ids, offs, _ = golden_truth
    doc = np.repeat(np.arange(len(offs) - 1), np.diff(offs))
    lab = np.where(doc % 2 == 0, ids, -100).astype(np.int32)
    want = _both(tok, voc, lab, tok_offsets=offs, skip_negative=True)
    text, toffs = golden["text"].tobytes(), golden["offsets"]
    assert want[0] == b"".join(text[int(toffs[d]):int(toffs[d + 1])] for d in range(0, len(offs) - 1, 2))
    first = int(np.flatnonzero(lab == -100)[0])
    got = _device(tok, lab, len(want[0]), tok_offsets=offs)
    assert got[5] == (capi.TD_E_BAD_TOKEN, first) and got[4]
    with pytest.raises(capi.TokenDaggerHipError) as e:
        tok.decode_rows(lab, _spec({}), tok_offsets=offs)
    assert e.value.code == capi.TD_E_BAD_TOKEN and f"index {first}" in str(e.value)
    _host(tok, lab, want, tok_offsets=offs, skip_negative=True)  # the handle is usable


# ---- errors: status codes, the device left usable ---------------------------------------------------------------------------------

def test_errors_are_status_codes(tok, voc):
    rng = np.random.default_rng(10)
    n = 3 * TILE
    good = rng.integers(1000, 100000, size=n).astype(np.int32)
    offs = np.asarray([0, 100, 9500, n], dtype=np.int64)
    want = dt.decode_numpy(good, voc[1], tok_offsets=offs)

    def usable():
        _device_ok(tok, good, want, tok_offsets=offs)

    bad = good.copy()
    bad[[5, 9000]] = voc[1].max_id + 3
    got = _device(tok, bad, len(want[0]), tok_offsets=offs)
    assert got[5] == (capi.TD_E_BAD_TOKEN, 5) and got[4]
    usable()
    for null_out in (False, True):  # one byte short, and the sizing call
        got = _device(tok, good, len(want[0]), tok_offsets=offs, capacity=len(want[0]) - 1, null_out=null_out)
        assert got[5] == (capi.TD_E_CAPACITY, len(want[0])) and got[4] and got[0] == b""
        _same((want[0],) + got[1:4], want)
        usable()
    with pytest.raises(capi.TokenDaggerHipError) as e:
        tok.decode_rows(good, _spec({}), tok_offsets=offs, capacity=len(want[0]) - 1)
    assert e.value.code == capi.TD_E_CAPACITY and e.value.n_bytes == len(want[0])
    _same((want[0], e.value.out_offsets, e.value.seg_ids, e.value.info), want)
    down = np.asarray([0, 9500, 100, n], dtype=np.int64)
    got = _device(tok, good, len(want[0]), tok_offsets=down)
    assert got[5] == (capi.TD_E_INVALID, 1) and got[4]
    usable()
    got = _device(tok, good, len(want[0]), tok_offsets=np.asarray([0, 100, n + 1], dtype=np.int64))
    assert got[5] == (capi.TD_E_INVALID, 2) and got[4]
    usable()
    rows = good[:37 * 19].reshape(37, 19)
    lengths = np.full(37, 19, dtype=np.int32)
    lengths[20] = 20
    got = _device(tok, rows, 8 * 37 * 19 * 4, row_stride=19, lengths=lengths)
    assert got[5] == (capi.TD_E_INVALID, 20) and got[4]
    usable()
    for call in (lambda: tok.decode_rows(good, _spec({}), tok_offsets=down),
                 lambda: tok.decode_rows(rows, _spec(dict(row_stride=19)), lengths=lengths),
                 lambda: tok.decode_rows(good, _spec(dict(skip=[3, -4])), tok_offsets=offs),
                 lambda: _device(tok, good, 64, tok_offsets=offs, stop=[-1])):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            call()
        assert e.value.code == capi.TD_E_INVALID
    usable()


# ---- the table's cache ------------------------------------------------------------------------------------------------------------

def test_table_cache_and_clones(tok, voc, generation):
    import torch
    batch, cut, bos, eos, pad = generation
    a = dict(row_stride=300, n_segs=8, skip=[pad, bos], stop=[eos])
    b = dict(row_stride=300, n_segs=8, skip=[pad], stop=[int(batch[1, 20])], keep_stop=True)
    wa = dt.decode_numpy(batch.reshape(-1), voc[1], **a)
    wb = dt.decode_numpy(batch.reshape(-1), voc[1], **b)
    assert wa[0] != wb[0]
    for kw, want in ((a, wa), (b, wb), (a, wa), (a, wa)):
        _device_ok(tok, batch, want, **kw)
    one, two = tok.clone(), tok.clone()
    try:
        dev = torch.device("cuda", 0)
        s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        for _ in range(2):
            _device_ok(one, batch, wa, stream=s1.cuda_stream, **a)
            _device_ok(two, batch, wb, stream=s2.cuda_stream, **b)
        _device_ok(one, batch, wb, stream=s2.cuda_stream, **b)  # another list on another stream of the same handle
        _device_ok(one, batch, wa, stream=s1.cuda_stream, **a)
    finally:
        one.close()
        two.close()
