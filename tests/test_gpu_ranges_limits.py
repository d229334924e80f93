"""td_range_labels (tokendagger_amd/csrc/td_ranges.hip) at the limits its design text names: a document table that does not fit
LDS, windows of ranges in LDS and in global memory beside it, more ranges than one pass of the chunk scan and than one sweep of
td_rng_check's grid, more documents than one sweep of td_rng_docs' grid, range chunk borders, pointers off the 16-byte grid and
ragged totals, the explicit-starts instantiation on all of these, and the errors found on those paths.

Every comparison is exact, against ranges_numpy of tests/ranges_truth.py; the small cases also against ranges_walk.  Token
lengths come from the vocabulary on the host.  No case makes the device fault: every error is one the library reports.

The library has no counter for the path a tile took, so every case proves from its inputs that it reaches the path it names,
by two predicates written here from the kernel's code:

  table_entries   what tile_table (td_rows_common.h) counts; the table has RC_LDS_DOCS = 4352 slots, filled 256 a step, and a
                  tile FITS iff a step holds fewer than 256 entries below the tile's end, that is iff the count is < 4352
  window_entries  w1 - w0 of td_rng_apply; the window is STAGED in LDS iff this is <= RNG_WIN = 512

A case whose predicate does not hold fails.  td_rng_apply's own grid cap (1 << 20 tiles, four billion ids) is out of a test's
reach; nothing here approximates it."""
import numpy as np
import pytest

import offsets_truth as OT
import ranges_truth as rt
from ranges_gpu_helpers import TILE, WIN, _bulk_ranges, _check, _device_call, _doc_sizes, _every_other_byte, _same, _spec, tok, vocab  # noqa: F401

pytestmark = pytest.mark.gpu

LDS_DOCS = 4352              # td::RC_LDS_DOCS
CHUNK = 1024                 # td::RNG_CHUNK: ranges a workgroup of td_rng_check, four a lane
PASS = 4 * 256 * CHUNK       # ranges one pass of chunks_excl_scan covers (four chunks a lane, 256 lanes)
CHECK_SWEEP = 2048 * CHUNK   # ranges one sweep of td_rng_check's grid covers (RC_MAX_GRID workgroups)
DOCS_SWEEP = 4096 * 256      # documents one sweep of td_rng_docs' grid covers
FILL = 77


# ---- the shape predicates -------------------------------------------------------------------------------------------------------
def table_entries(offs, tile=TILE):
    """Per tile: the tok_offsets entries (the sentinel behind the last document included), from the tile's first document on,
    whose value is below the tile's end: tile_table's return value n when the table fits.  d0 is the last document that begins
    at or before the tile's first id (group_last_le), so empty documents in front of it, on the tile's edge, are not counted.
    The tile fits iff this is < RC_LDS_DOCS = 4352: seventeen steps of 256 entries, and the loop ends at the first step that
    holds an entry at or above the limit; 4352 entries below it fill every step."""
    offs = np.asarray(offs, dtype=np.int64)
    n_docs, total = len(offs) - 1, int(offs[-1])
    t0 = np.arange(0, total, tile, dtype=np.int64)
    end = np.minimum(t0 + tile, total)
    d0 = np.searchsorted(offs[:n_docs], t0, "right") - 1
    return np.searchsorted(offs, end, "left") - d0


def window_entries(offs, ro, rg, s, e, tile=TILE):
    """Per tile: w1 - w0 of td_rng_apply.  w0: the last range of the tile's first document that begins at or before the start
    of the tile's first id (none: the document's first range, or where it would be); w1: one behind the last range of the
    tile's last document that begins at or before the end of the tile's last id (none: one behind its first; a document
    without ranges: where they would be).  s, e: every id's start and end in its document."""
    offs, ro = np.asarray(offs, dtype=np.int64), np.asarray(ro, dtype=np.int64)
    n_docs, total = len(offs) - 1, int(offs[-1])
    out = []
    for t0 in range(0, total, tile):
        last = min(t0 + tile, total) - 1
        d0 = int(np.searchsorted(offs[:n_docs], t0, "right")) - 1
        dl = int(np.searchsorted(offs[:n_docs], last, "right")) - 1
        f0, f1, l0, l1 = int(ro[d0]), int(ro[d0 + 1]), int(ro[dl]), int(ro[dl + 1])
        w0 = max(f0, f0 + int(np.searchsorted(rg[f0:f1, 0], s[t0], "right")) - 1)
        w1 = l0 if l1 == l0 else max(l0, l0 + int(np.searchsorted(rg[l0:l1, 0], e[last], "right")) - 1) + 1
        out.append(w1 - w0)
    return np.asarray(out, dtype=np.int64)


def _kinds(lengths, ids, offs, ro, rg, starts=None):
    """-> (fits, staged), a boolean per tile."""
    total = int(offs[-1])
    s = OT.covered_byte_starts(ids[:total], offs, lengths) if starts is None else np.asarray(starts, dtype=np.int64)[:total]
    e = s + lengths[np.asarray(ids[:total], dtype=np.int64)]
    return table_entries(offs) < LDS_DOCS, window_entries(offs, ro, rg, s, e) <= WIN


def test_the_predicates_on_hand_cases():
    # 10 ids a tile: documents [0, 3) [3, 3) [3, 3) [3, 12) [12, 12) [12, 25); the sentinel 25
    offs = [0, 3, 3, 3, 12, 12, 25]
    assert table_entries(offs, 10).tolist() == [4, 3, 1]  # 0 3 3 3 | (d0 = 3: 3) 12 12 | (d0 = 5: 12); the sentinel is never below the end
    assert table_entries([0, 10, 10, 10, 15], 10).tolist() == [1, 1]  # empty documents exactly on the edge cost nothing
    assert table_entries([0, 7, 7, 7], 10).tolist() == [1] and table_entries([0, 0, 0], 10).tolist() == []
    ro = np.asarray([0, 2, 3, 3, 6, 6, 7])
    rg = np.asarray([(0, 1), (5, 6), (0, 0), (2, 3), (10, 11), (40, 50), (100, 200)])
    s = np.concatenate([np.arange(3), np.arange(9), np.arange(13)]) * 4  # every id has four bytes
    # tile 0: ids 0 - 9, document 0 from byte 0 (w0 = 0) to document 3's id 6, bytes [24, 28): ranges 3, 4 begin in front (w1 = 5)
    # tile 1: document 3's id 7 at byte 28 (w0 = 4) to document 5's id 7, bytes [28, 32): none begins in front (w1 = 6 + 1)
    # tile 2: document 5 from byte 32 (none at or in front: w0 = 6) to byte 52 (w1 = 7)
    assert window_entries(offs, ro, rg, s, s + 4, 10).tolist() == [5, 3, 1]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _build(rng, lengths, pool, n_ids, tagged=(), k_real=4, every_other=()):
    """Documents of n_ids[d] ids drawn from pool -> (ids, tok_offsets, range_offsets, ranges).  A document with ids gets k_real
    random sorted ranges inside its bytes (the last one up to its end), or, when it is in every_other, a range of one byte on
    every other byte; the documents in `tagged` (empty ones) get one range (0, 0)."""
    n_ids = np.asarray(n_ids, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(n_ids)]).astype(np.int64)
    ids = np.asarray(pool, dtype=np.int32)[rng.integers(0, len(pool), int(offs[-1]))]
    sizes = _doc_sizes(lengths, ids, offs)
    cnt = np.zeros(len(n_ids), dtype=np.int64)
    cnt[np.asarray(tagged, dtype=np.int64)] = 1
    mine = {}
    for d in np.flatnonzero(n_ids > 0).tolist():
        if d in every_other:
            mine[d] = _every_other_byte(int(sizes[d]) // 2)
        else:
            mine[d] = np.sort(rng.integers(0, sizes[d] + 1, 2 * k_real)).reshape(-1, 2)
            mine[d][-1, 1] = sizes[d]
        cnt[d] = len(mine[d])
    ro = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    rg = np.zeros((int(ro[-1]), 2), dtype=np.int64)
    for d, r in mine.items():
        rg[ro[d]:ro[d + 1]] = r
    return ids, offs, ro, rg


def _both_forms(tok, lengths, ids, offs, ro, rg, rules=rt.RULES, walk=False):
    """The covered form and the explicit form on the covering starts: both equal the truth, and so each other."""
    starts = OT.covered_byte_starts(ids, offs, lengths)
    covered = _check(tok, lengths, ids, offs, ro, rg, rules=rules)
    explicit = _check(tok, lengths, ids, offs, ro, rg, rules=rules, starts=starts)
    for rule in rules:
        _same(explicit[rule], covered[rule], rule)
        if walk:
            _same(covered[rule], rt.ranges_walk(ids, offs, ro, rg, lengths, rule), rule)
    return covered


# ---- 1. the table boundary ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tagged", [False, True], ids=["window staged", "window global"])
@pytest.mark.parametrize("E", [4348, 4349, 4350, 4351, 4352, 4353, 5000])
def test_empty_run_at_the_table_limit(tok, vocab, E, tagged):
    """[3 ids] + E empty documents + [7 ids], one tile: E + 2 entries lie below the tile's end (0, then E + 1 times 3), so
    E = 4349 is the last run whose table fits.  A (0, 0) range on every seventh empty document (more than 600) puts the
    window, which spans the run, beyond RNG_WIN."""
    lengths, pool = vocab[3], vocab[4]
    rng = np.random.default_rng(100 + E)
    n_ids = np.concatenate([[3], np.zeros(E, dtype=np.int64), [7]])
    tags = np.arange(1, E + 1)[::7] if tagged else ()
    ids, offs, ro, rg = _build(rng, lengths, pool, n_ids, tags, k_real=2)
    assert table_entries(offs).tolist() == [E + 2]
    fits, staged = _kinds(lengths, ids, offs, ro, rg)
    assert fits.tolist() == [E <= 4349] and staged.tolist() == [not tagged] and (len(tags) >= 600 or not tagged)
    t = _both_forms(tok, lengths, ids, offs, ro, rg, walk=True)
    assert len(t["overlap"][2]) == E + 3


@pytest.mark.parametrize("tagged", [False, True], ids=["no ranges on the run", "(0, 0) on every seventh"])
@pytest.mark.parametrize("where", ["near the edge", "on the edge", "at the end"])
def test_empty_run_of_5000_around_a_tile_edge(tok, vocab, where, tagged):
    lengths, pool = vocab[3], vocab[4]
    rng = np.random.default_rng(7 + len(where))
    E = 5000
    before, after = {"near the edge": (4090, 20), "on the edge": (4096, 5), "at the end": (4100, 0)}[where]
    n_ids = np.concatenate([[before], np.zeros(E, dtype=np.int64), [after] if after else []]).astype(np.int64)
    tags = np.arange(1, E + 1)[::7] if tagged else ()
    ids, offs, ro, rg = _build(rng, lengths, pool, n_ids, tags, k_real=6)
    fits, staged = _kinds(lengths, ids, offs, ro, rg)
    if where == "near the edge":    # tile 0 holds the run and the second document's first six ids, tile 1 begins inside that document
        assert table_entries(offs).tolist() == [E + 2, 1]
        assert fits.tolist() == [False, True] and staged.tolist() == [not tagged, True]
    elif where == "on the edge":    # the run begins where tile 1 begins: tile 1's first document is the one behind the run
        assert table_entries(offs).tolist() == [1, 1]
        assert fits.tolist() == [True, True] and staged.tolist() == [True, True]
    else:                           # behind the last id: no tile sees the run, td_rng_docs alone handles it
        assert table_entries(offs).tolist() == [1, 1]
        assert fits.tolist() == [True, True] and staged.tolist() == [True, True] and offs[-1] == offs[1]
    t = _both_forms(tok, lengths, ids, offs, ro, rg)
    assert len(t["start"][2]) == len(n_ids) + 1 and t["start"][3][0] > 0


# ---- 2. all four kinds of tile in one batch ---------------------------------------------------------------------------------------------
def test_every_combination_of_table_and_window_in_one_batch(tok, vocab):
    lengths, pool = vocab[3], vocab[4]
    rng = np.random.default_rng(21)
    E = 5000
    run = np.zeros(E, dtype=np.int64)
    # tile 0: one document, four ranges; tile 1: one document, a range on every other byte; tile 2: a run of empty documents
    # without ranges between two documents; tile 3: the same with (0, 0) on every fifth; tile 4: the rest of the last document
    n_ids = np.concatenate([[TILE, TILE, 2000], run, [2096, 2000], run, [2096 + 300]]).astype(np.int64)
    second = 3 + E + 2
    ids, offs, ro, rg = _build(rng, lengths, pool, n_ids, tagged=np.arange(second, second + E)[::5], every_other={1})
    assert offs[-1] == 4 * TILE + 300
    fits, staged = _kinds(lengths, ids, offs, ro, rg)
    assert list(zip(fits.tolist(), staged.tolist())) == [(True, True), (True, False), (False, True), (False, False), (True, True)]
    for f in (False, True):
        for s in (False, True):
            assert ((fits == f) & (staged == s)).sum() >= 1
    t = _both_forms(tok, lengths, ids, offs, ro, rg)
    assert t["overlap"][3][0] > TILE and t["inside"][3][0] > 100 and t["overlap"][3][1] > TILE // 2


# ---- 3. many documents -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tagged", [False, True], ids=["no ranges on empty documents", "(0, 0) on a tenth of them"])
def test_more_documents_than_one_sweep_of_the_document_kernel(tok, vocab, tagged):
    """1.2 million documents, one in fifty with one to five ids: about seventeen tiles with some 68 000 documents each, none of
    whose tables fits; td_rng_docs strides, td_lab_finish writes more than a million trained offsets.  BOTH variants search
    their windows in global memory: a tile has some 1400 documents with a range even without the ranges on the empty ones, so
    "table does not fit, window staged" is not met at this size (it is in the table-limit cases and in the batch of four kinds)."""
    lengths, pool = vocab[3], vocab[4]
    rng = np.random.default_rng(33)
    n_docs = 1_200_000
    assert n_docs > DOCS_SWEEP
    n_ids = np.where(rng.random(n_docs) < 0.02, rng.integers(1, 6, n_docs), 0).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(n_ids)]).astype(np.int64)
    ids = pool[rng.integers(0, len(pool), int(offs[-1]))]
    sizes = _doc_sizes(lengths, ids, offs)
    real = n_ids > 0
    cnt = real.astype(np.int64)
    if tagged:
        cnt[~real & (rng.random(n_docs) < 0.1)] = 1
    ro = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    rg = np.zeros((int(ro[-1]), 2), dtype=np.int64)
    begin = (rng.random(n_docs) * (sizes + 1)).astype(np.int64)
    end = begin + (rng.random(n_docs) * (sizes - begin + 1)).astype(np.int64)
    rg[ro[:-1][real]] = np.stack([begin[real], end[real]], axis=1)
    assert (rg[:, 1] <= np.repeat(sizes, cnt)).all() and offs[-1] > 16 * TILE
    fits, staged = _kinds(lengths, ids, offs, ro, rg)
    assert not fits.any() and len(fits) >= 17
    assert not staged.any() and (len(rg) > 130_000 or not tagged)  # (some 1400 documents with a range in a tile, without the empty ones')
    t = _check(tok, lengths, ids, offs, ro, rg)
    assert len(t["overlap"][2]) == n_docs + 1 and t["overlap"][3][0] > t["inside"][3][0] > 5000 and t["overlap"][3][1] > 5000


# ---- 4. many ranges ------------------------------------------------------------------------------------------------------------------
N_MANY = CHECK_SWEEP + 3000 + 77
K = 5
FIRSTS = [K * CHUNK - 1, K * CHUNK, K * CHUNK + 1, PASS, PASS + 1, CHECK_SWEEP]


def _many_ranges(lengths, firsts, seed):
    """N_MANY ranges of one byte on every other byte of their documents; a document's first range at every index of `firsts`
    (so it begins at 0 behind one that ends high), an empty document without ranges among them.  The documents are as long as
    their ranges need: ids of four to nine bytes, about 0.3 of an id a range."""
    rng = np.random.default_rng(seed)
    long_ids = np.flatnonzero((lengths >= 4) & (lengths <= 9))[:50].astype(np.int32)
    counts = np.diff([0] + list(firsts) + [N_MANY])
    ids = long_ids[rng.integers(0, len(long_ids), N_MANY // 2 + 4 * len(counts) + 8)]
    cs = np.concatenate([[0], np.cumsum(lengths[ids])])
    offs, pos = [0], 0
    for c in counts.tolist():  # the fewest ids whose bytes hold 2 c - 1 bytes of ranges
        pos = int(np.searchsorted(cs, cs[pos] + 2 * c, "left"))
        assert pos < len(cs)
        offs.append(pos)
    mid = len(counts) // 2   # the empty document: in front of the document whose first range is firsts[mid - 1]
    offs = np.asarray(offs[:mid + 1] + offs[mid:], dtype=np.int64)
    cnt = np.concatenate([counts[:mid], [0], counts[mid:]])
    ro = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    rg = np.concatenate([_every_other_byte(int(c)) for c in counts])
    return ids[:pos].copy(), offs, ro, rg


@pytest.fixture(scope="module")
def many_ranges(vocab):
    return _many_ranges(vocab[3], FIRSTS, 44)


def _assert_many(lengths, ids, offs, ro, rg, firsts):
    assert len(rg) == N_MANY > CHECK_SWEEP + 3000 and N_MANY > 2 * PASS and (np.diff(offs) == 0).sum() == 1
    assert set(firsts) <= set(ro.tolist())
    for r in firsts:  # the first range begins at 0, the one in front of it, another document's, ends above it
        assert rg[r, 0] == 0 and rg[r - 1, 1] >= 1
    fits, staged = _kinds(lengths, ids, offs, ro, rg)
    assert fits.all() and not staged.any() and len(fits) > 100


def test_more_ranges_than_two_passes_of_the_chunk_scan_first_ranges_on_the_borders(tok, vocab, many_ranges):
    """Documents that begin at range indices 1024 k - 1, 1024 k, 1024 k + 1, 1024 * 1024, 1024 * 1024 + 1 and 2048 * 1024 (six
    indices need seven documents with ranges, three of them with one range): a first-range bit read wrong is a false
    TD_E_INVALID."""
    lengths = vocab[3]
    ids, offs, ro, rg = many_ranges
    _assert_many(lengths, ids, offs, ro, rg, FIRSTS)
    t = _check(tok, lengths, ids, offs, ro, rg, rules=("overlap", "inside"))
    assert t["overlap"][3][2] == N_MANY and t["overlap"][3][0] >= len(ids) - len(offs) and t["inside"][3][0] == 0


def test_more_ranges_than_two_passes_of_the_chunk_scan_documents_across_the_borders(tok, vocab):
    """Four documents, one empty; the two long ones lie across range 1024 * 1024 and across range 2048 * 1024, so ids of one
    document take cum + rchunks from both sides of a pass of chunks_excl_scan: a lost carry is a wrong m there."""
    lengths = vocab[3]
    firsts = [700_000, 1_500_000]
    ids, offs, ro, rg = _many_ranges(lengths, firsts, 45)
    _assert_many(lengths, ids, offs, ro, rg, firsts)
    assert len(offs) == 5 and ro[1] < PASS < ro[3] < CHECK_SWEEP < ro[4]
    t = _check(tok, lengths, ids, offs, ro, rg, rules=("overlap", "inside"))
    assert t["overlap"][3][2] == N_MANY and t["overlap"][3][0] >= len(ids) - len(offs) and t["overlap"][3][1] >= len(ids) - len(offs)


# ---- 5. a chunk border inside one window ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_second", [101, 601], ids=["staged", "global"])
def test_a_window_across_a_chunk_border(tok, vocab, n_second):
    """Tile 0 is a document with ranges 0 - 999, tile 1 a document with ranges 1000 - 1100 (1600): its window takes cum from
    chunk 0 and from chunk 1."""
    lengths, pool = vocab[3], vocab[4]
    rng = np.random.default_rng(55)
    offs = np.asarray([0, TILE, 2 * TILE - 9], dtype=np.int64)
    ids = pool[rng.integers(0, len(pool), int(offs[-1]))]
    sizes = _doc_sizes(lengths, ids, offs)
    parts = []
    for size, k in zip(sizes.tolist(), (1000, n_second)):
        cuts = np.sort(rng.integers(0, size + 1, 2 * k)).reshape(-1, 2)
        cuts[0, 0], cuts[-1, 1] = 0, size  # every range of the document is in the tile's window
        parts.append(cuts)
    ro = np.asarray([0, 1000, 1000 + n_second], dtype=np.int64)
    rg = np.concatenate(parts).astype(np.int64)
    s = OT.covered_byte_starts(ids, offs, lengths)
    assert window_entries(offs, ro, rg, s, s + lengths[ids]).tolist() == [1000, n_second] and ro[1] < CHUNK < ro[2] - 1
    fits, staged = _kinds(lengths, ids, offs, ro, rg)
    assert fits.all() and staged.tolist() == [False, n_second <= WIN]
    t = _both_forms(tok, lengths, ids, offs, ro, rg, walk=n_second <= WIN)
    assert t["overlap"][3][1] > 100 and t["inside"][3][0] > 100


# ---- the device form with buffers that stay -----------------------------------------------------------------------------------------------
def _behind(arr, dtype, shift, room=0, fill=0):
    """arr on the device, `shift` elements behind an aligned allocation, `room` more behind it -> (the view, the whole buffer)."""
    import torch
    dev = torch.device("cuda", 0)
    arr = np.ascontiguousarray(arr)
    big = torch.full((len(arr) + shift + room,), fill, dtype=dtype, device=dev)
    big[shift:shift + len(arr)] = torch.from_numpy(arr).to(dev)
    view = big[shift:shift + len(arr)]
    assert big.data_ptr() % 256 == 0 and view.data_ptr() == big.data_ptr() + shift * big.element_size()
    return view, big


class _Resident:
    """A batch on the device once, called many times.  shift: elements in front of ids / labels (int32), mask (bytes), ranges
    and starts (int64) inside their aligned allocations."""

    def __init__(self, ids, offs, ro, rg, starts=None, shift=0):
        import torch
        self.n, self.n_docs, self.n_ranges, self.shift = len(ids), len(offs) - 1, len(rg), shift
        self.ids, _ = _behind(np.asarray(ids, dtype=np.int32), torch.int32, shift)
        self.offs, _ = _behind(np.asarray(offs, dtype=np.int64), torch.int64, 0)
        self.ro, _ = _behind(np.asarray(ro, dtype=np.int64), torch.int64, 0)
        self.rg, _ = _behind(np.ascontiguousarray(rg, dtype=np.int64).reshape(-1), torch.int64, shift)
        self.starts = _behind(np.asarray(starts, dtype=np.int64), torch.int64, shift)[0] if starts is not None else None

    def set_range(self, r, begin, end):
        self.rg[2 * r], self.rg[2 * r + 1] = int(begin), int(end)

    def call(self, tok, spec, ranges_ptr=None, raises=None):
        """-> (labels, mask, trained_offsets, counts as numpy, the whole label and mask buffers, (code, err_pos))"""
        import torch
        from tokendagger_amd import capi
        dev = torch.device("cuda", 0)
        sh = self.shift
        lab, lab_all = _behind(np.full(max(self.n, 1), FILL, dtype=np.int32), torch.int32, sh, 4, FILL)
        mask, mask_all = _behind(np.full(max(self.n, 1), FILL, dtype=np.uint8), torch.uint8, sh, 4, FILL)
        toff = torch.full((self.n_docs + 1,), FILL, dtype=torch.int64, device=dev)
        counts = torch.full((4,), FILL, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        args = (self.ids.data_ptr() if self.n else 0, self.n, self.offs.data_ptr(), self.n_docs, self.ro.data_ptr(),
                (self.rg.data_ptr() if self.n_ranges else 0) if ranges_ptr is None else ranges_ptr, self.n_ranges, spec, lab.data_ptr(),
                mask.data_ptr(), toff.data_ptr(), counts.data_ptr(), self.starts.data_ptr() if self.starts is not None else 0, stream)
        if raises is None:
            tok.range_labels_device(*args)
        else:
            with pytest.raises(capi.TokenDaggerHipError) as ex:
                tok.range_labels_device(*args)
            assert ex.value.code == raises
        status = tok.device_status_pos(stream)
        return [lab.cpu().numpy(), mask.cpu().numpy(), toff.cpu().numpy(), counts.cpu().numpy()], (lab_all.cpu().numpy(), mask_all.cpu().numpy()), status


def _untouched(outs, whole):
    for o in list(outs) + list(whole):
        assert (o == FILL).all()


# ---- 6. bad ranges at the chunk, pass and sweep borders --------------------------------------------------------------------------------------
def test_out_of_order_ranges_at_the_borders_report_their_index(tok, vocab, many_ranges):
    """One bad range at a time in the batch of case 4, device form: begins in front of the end before it (prev_end comes from
    the lane, the chunk or the sweep in front), or, where the index is a document's first range, ends in front of its begin."""
    from tokendagger_amd import capi
    lengths = vocab[3]
    ids, offs, ro, rg = many_ranges
    assert len(rg) == N_MANY > CHECK_SWEEP
    dev = _Resident(ids, offs, ro, rg)
    firsts = set(ro.tolist())

    def spoil(r):
        if r in firsts:
            dev.set_range(r, rg[r, 1], rg[r, 0])   # reversed
        else:
            assert 0 <= rg[r, 0] - 2 < rg[r - 1, 1]
            dev.set_range(r, rg[r, 0] - 2, rg[r, 1])  # begins in front of the end before it; the one behind it stays in order

    spots = [CHUNK - 1, CHUNK, CHUNK + 1, PASS - 1, PASS, CHECK_SWEEP, N_MANY - 1]
    assert [r in firsts for r in spots] == [False, False, False, False, True, True, False]
    for r in spots:
        spoil(r)
        outs, whole, status = dev.call(tok, _spec())
        assert status == (capi.TD_E_INVALID, r), (status, r)
        _untouched(outs, whole)
        dev.set_range(r, *rg[r])
    for low, high in ((CHECK_SWEEP - 5, CHECK_SWEEP + 1500), (PASS + CHUNK + 3, CHECK_SWEEP + 4)):  # the lower of two wins
        spoil(low), spoil(high)
        outs, whole, status = dev.call(tok, _spec())
        assert status == (capi.TD_E_INVALID, low), (status, low, high)
        _untouched(outs, whole)
        dev.set_range(low, *rg[low]), dev.set_range(high, *rg[high])
    outs, _, status = dev.call(tok, _spec("inside"))  # everything restored: the batch is good again
    assert status[0] == 0
    _same(outs, rt.ranges_numpy(ids, offs, ro, rg, lengths, "inside"))


# ---- 7. "beyond the document" where the documents are found in global memory -------------------------------------------------------------------
def _beyond(tok, lengths, ids, offs, ro, rg, offenders, want):
    """offenders: (range index, its new end); the device form reports `want`."""
    from tokendagger_amd import capi
    far = rg.copy()
    for r, end in offenders:
        far[r, 1] = end
    _, status = _device_call(tok, ids, len(ids), offs, ro, far, _spec())
    assert status == (capi.TD_E_INVALID, want), (status, want)


def test_a_range_beyond_its_document_found_through_the_global_search(tok, vocab):
    lengths, pool = vocab[3], vocab[4]
    rng = np.random.default_rng(66)
    E = 5000
    run = np.zeros(E, dtype=np.int64)
    # a, b: [50 ids] + the run + [50 ids]; one tile, its table does not fit
    ids, offs, ro, rg = _build(rng, lengths, pool, np.concatenate([[50], run, [50]]), tagged=np.arange(1, E + 1)[::50])
    sizes = _doc_sizes(lengths, ids, offs)
    fits, _ = _kinds(lengths, ids, offs, ro, rg)
    assert fits.tolist() == [False]
    last = len(rg) - 1
    assert rg[last, 1] == sizes[-1]
    _beyond(tok, lengths, ids, offs, ro, rg, [(last, sizes[-1] + 1)], last)
    on_empty = int(ro[2501])
    assert ro[2502] == on_empty + 1 and offs[2501] == offs[2502] and on_empty < last
    _beyond(tok, lengths, ids, offs, ro, rg, [(on_empty, 1)], on_empty)
    _beyond(tok, lengths, ids, offs, ro, rg, [(last, sizes[-1] + 1), (on_empty, 1)], on_empty)
    _check(tok, lengths, ids, offs, ro, rg, rules=("overlap",))  # the handle is fine afterwards
    # c: two tiles, one of each kind; the offenders are the last ranges of a document that ends in the one and in the other
    for n_ids, kinds, docs in ((np.concatenate([[50], run, [50, TILE, 100]]), [False, True], (E + 1, E + 3)),
                               (np.concatenate([[100, TILE - 100 + 50], run, [50]]), [True, False], (0, E + 2))):
        ids, offs, ro, rg = _build(rng, lengths, pool, n_ids)
        sizes = _doc_sizes(lengths, ids, offs)
        fits, _ = _kinds(lengths, ids, offs, ro, rg)
        assert fits.tolist() == kinds
        first, second = (int(ro[d + 1]) - 1 for d in docs)
        assert (offs[docs[0] + 1] - 1) // TILE == 0 and (offs[docs[1] + 1] - 1) // TILE == 1 and first < second
        hit = [(first, sizes[docs[0]] + 1), (second, sizes[docs[1]] + 1)]
        _beyond(tok, lengths, ids, offs, ro, rg, hit[:1], first)
        _beyond(tok, lengths, ids, offs, ro, rg, hit[1:], second)
        _beyond(tok, lengths, ids, offs, ro, rg, hit, first)
        _check(tok, lengths, ids, offs, ro, rg, rules=("overlap",))


# ---- 8. pointers off the 16-byte grid, ragged totals ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1, 3, 15, 17])
def test_device_pointers_off_the_16_byte_grid(tok, vocab, r):
    """d_ids and d_labels one int32, d_mask one byte, d_ranges and d_starts one int64 behind an aligned allocation: the dword
    loads of the ids, rows_put4's dword stores and the mask's byte stores, where the aligned call takes int4, int4 and uint4."""
    from tokendagger_amd import capi
    lengths, pool = vocab[3], vocab[4]
    rng = np.random.default_rng(80 + r)
    total = 2 * TILE + r
    offs = np.asarray([0, TILE - 7, TILE - 7, total], dtype=np.int64)
    ids = np.concatenate([pool[rng.integers(0, len(pool), total)], np.full(300, -7, dtype=np.int32)])  # 300 slots behind the ids
    ro, rg = _bulk_ranges(rng, _doc_sizes(lengths, ids[:total], offs), 40, min_k=20)
    fits, staged = _kinds(lengths, ids, offs, ro, rg)
    assert fits.all() and staged.all() and len(fits) == (3 if r else 2)
    starts = np.concatenate([OT.covered_byte_starts(ids[:total], offs, lengths), np.zeros(300, np.int64)])
    for st in (None, starts):
        aligned, shifted = _Resident(ids, offs, ro, rg, st, shift=0), _Resident(ids, offs, ro, rg, st, shift=1)
        assert shifted.ids.data_ptr() % 16 == 4 and shifted.rg.data_ptr() % 16 == 8 and aligned.ids.data_ptr() % 16 == 0
        assert st is None or shifted.starts.data_ptr() % 16 == 8
        for rule in rt.RULES:
            want = rt.ranges_numpy(ids[:total], offs, ro, rg, lengths, rule, -1)
            for dev in (aligned, shifted):
                (lab, m, to, counts), (lab_all, mask_all), status = dev.call(tok, _spec(rule, -1))
                assert status[0] == 0
                _same((lab[:total], m[:total], to, counts), want, (rule, dev.shift))
                assert (lab[total:] == FILL).all() and (m[total:] == FILL).all()                  # the 300 slots behind the ids
                assert (lab_all[:dev.shift] == FILL).all() and (mask_all[:dev.shift] == FILL).all()  # the element in front
                assert (lab_all[dev.shift + len(ids):] == FILL).all() and (mask_all[dev.shift + len(ids):] == FILL).all()
    # ranges at 4 mod 8: refused by the call itself, nothing is launched
    outs, whole, status = shifted.call(tok, _spec(), ranges_ptr=shifted.rg.data_ptr() + 4, raises=capi.TD_E_INVALID)
    assert status[0] == 0
    _untouched(outs, whole)


# ---- 9. explicit starts that skip text, at size -----------------------------------------------------------------------------------------------
def _stretched(rng, lengths, pool, offs):
    """Covering starts plus a random gap of 0 - 3 bytes in front of every id -> (ids, starts, the documents' stretched sizes)."""
    total = int(offs[-1])
    ids = pool[rng.integers(0, len(pool), total)]
    doc = np.repeat(np.arange(len(offs) - 1), np.diff(offs))
    gaps = np.concatenate([[0], np.cumsum(rng.integers(0, 4, total))])
    starts = OT.covered_byte_starts(ids, offs, lengths) + gaps[1:] - gaps[offs[doc]]
    sizes = np.zeros(len(offs) - 1, dtype=np.int64)
    np.maximum.at(sizes, doc, starts + lengths[ids])
    return ids, starts.astype(np.int64), sizes


@pytest.mark.parametrize("dense", [False, True], ids=["at most 30 ranges a document", "a range on every other byte"])
def test_explicit_starts_that_skip_text_over_three_tiles(tok, vocab, dense):
    lengths, pool = vocab[3], vocab[4]
    rng = np.random.default_rng(90)
    offs = np.asarray([0, 1500, TILE + 1, 3 * TILE - 40, 3 * TILE + 333], dtype=np.int64)
    ids, starts, sizes = _stretched(rng, lengths, pool, offs)
    assert not np.array_equal(starts, OT.covered_byte_starts(ids, offs, lengths))
    if dense:
        rg = np.concatenate([_every_other_byte(int(s) // 2) for s in sizes])
        ro = np.concatenate([[0], np.cumsum(sizes // 2)]).astype(np.int64)
    else:
        ro, rg = _bulk_ranges(rng, sizes, 30, min_k=10)
    fits, staged = _kinds(lengths, ids, offs, ro, rg, starts)
    assert fits.all() and len(fits) == 4 and (not staged.any() if dense else staged.all())
    t = _check(tok, lengths, ids, offs, ro, rg, starts=starts)
    assert t["overlap"][3][0] > (2 * TILE if dense else 1000) and t["overlap"][3][1] > 100
    # one tile of the same kind against the walk
    offs = np.asarray([0, 700, 700, 2900, TILE - 5], dtype=np.int64)
    ids, starts, sizes = _stretched(rng, lengths, pool, offs)
    if dense:
        rg = np.concatenate([_every_other_byte(int(s) // 2) for s in sizes])
        ro = np.concatenate([[0], np.cumsum(sizes // 2)]).astype(np.int64)
    else:
        ro, rg = _bulk_ranges(rng, sizes, 30)
    fits, staged = _kinds(lengths, ids, offs, ro, rg, starts)
    assert fits.tolist() == [True] and staged.tolist() == [not dense]
    _check(tok, lengths, ids, offs, ro, rg, starts=starts, truth=rt.ranges_walk)


# ---- 10. nothing but empty documents ----------------------------------------------------------------------------------------------------------
def test_nothing_but_empty_documents(tok, vocab):
    import torch
    from tokendagger_amd import capi
    lengths = vocab[3]
    n_docs = 5000
    offs = np.zeros(n_docs + 1, dtype=np.int64)
    ids = np.zeros(0, dtype=np.int32)
    cnt = np.zeros(n_docs, dtype=np.int64)
    cnt[::3] = 1
    cnt[10] = 2
    ro = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    rg = np.zeros((int(ro[-1]), 2), dtype=np.int64)
    assert table_entries(offs).tolist() == [] and len(rg) > 1600
    for rule in rt.RULES:
        lab, m, to, counts = tok.range_labels(ids, offs, (ro, rg), _spec(rule), mask=True, trained_offsets=True)
        assert len(lab) == 0 and len(m) == 0 and to.tolist() == [0] * (n_docs + 1) and counts.tolist() == [0, 0, 0, 0]
        _same((lab, m, to, counts), rt.ranges_numpy(ids, offs, ro, rg, lengths, rule))
    d = 1998  # (a multiple of three: it has one range)
    bad = int(ro[d])
    assert cnt[d] == 1
    far = rg.copy()
    far[bad] = (0, 1)
    outs, status = _device_call(tok, ids, 0, offs, ro, far, _spec())
    assert status == (capi.TD_E_INVALID, bad)
    with pytest.raises(capi.TokenDaggerHipError) as ex:
        tok.range_labels(ids, offs, (ro, far), _spec())
    assert ex.value.code == capi.TD_E_INVALID
    # the explicit form knows nothing about a document's length: null ids, no ids at all, a starts pointer that is never read
    nothing = torch.zeros(1, dtype=torch.int64, device=torch.device("cuda", 0))
    dev = _Resident(ids, offs, ro, far)
    dev.starts = nothing
    (lab, m, to, counts), whole, status = dev.call(tok, _spec())
    assert status[0] == 0 and to.tolist() == [0] * (n_docs + 1) and counts.tolist() == [0, 0, 1, 0]
    _untouched((lab, m), whole)
    _check(tok, lengths, ids, offs, ro, rg, rules=("overlap",))
