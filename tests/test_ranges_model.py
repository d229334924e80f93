"""Loss labels from byte ranges without a GPU: the two truths of tests/ranges_truth.py against each other and against hand-written
cases, the CPU model of the kernels' decomposition (tests/twin/ranges_model.cpp over tokendagger_amd/csrc/td_ranges_args.h)
against both truths, td_range_plan through the C ABI, and the character-to-byte conversion of the text forms."""
import ctypes
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import helpers as H
import offsets_truth as OT
import ranges_truth as rt


@pytest.fixture(scope="module")
def vocab():
    pat, mr, special = H.llama4()
    lengths = OT.id_lengths(OT.id_bytes(mr, special))
    pool = []  # a few ids of every byte length from 1 to 12, and the longest tokens
    for k in range(1, 13):
        pool += np.flatnonzero(lengths == k)[:3].tolist()
    pool += np.argsort(-lengths)[:3].tolist()
    return lengths, np.asarray(pool, dtype=np.int32), mr


def _same(a, b, what=""):
    for k, (p, q) in enumerate(zip(a, b)):
        assert p.dtype == q.dtype and p.shape == q.shape and np.array_equal(p, q), (what, k)


def test_truths_agree_on_random_cases(vocab):
    lengths, pool, _ = vocab
    rng = np.random.default_rng(5)
    seen = dict(empty_doc=0, no_ranges=0, empty_range=0, touching=0, one_byte=0, at_end=0, partial=0)
    for it in range(400):
        ids, offs, ro, rg = rt.random_case(rng, lengths, pool, max_docs=12 if it % 8 else 60)
        for rule in rt.RULES:
            ign = int(rng.integers(-5, 3))
            w = rt.ranges_walk(ids, offs, ro, rg, lengths, rule, ign)
            _same(w, rt.ranges_numpy(ids, offs, ro, rg, lengths, rule, ign), (it, rule))
            st = OT.covered_byte_starts(ids, offs, lengths)  # the explicit form on covering starts is the covered form
            _same(w, rt.ranges_numpy(ids, offs, ro, rg, lengths, rule, ign, starts=st), (it, rule, "starts"))
            _same(w, rt.ranges_walk(ids, offs, ro, rg, lengths, rule, ign, starts=st), (it, rule, "walk starts"))
        seen["partial"] += int(w[3][1])
        seen["empty_doc"] += int((np.diff(offs) == 0).sum())
        seen["no_ranges"] += int((np.diff(ro) == 0).sum())
        seen["empty_range"] += int((rg[:, 0] == rg[:, 1]).sum())
        seen["one_byte"] += int((rg[:, 1] - rg[:, 0] == 1).sum())
        for d in range(len(offs) - 1):
            mine = rg[ro[d]:ro[d + 1]]
            size = int(lengths[ids[offs[d]:offs[d + 1]]].sum())
            seen["touching"] += int((mine[1:, 0] == mine[:-1, 1]).sum())
            seen["at_end"] += int(len(mine) > 0 and mine[-1, 1] == size and size > 0)
    assert all(v >= 50 for v in seen.values()), seen


def _one(vocab, text_pieces, ranges, rule, starts=None):
    """One document of the given pieces (each one id of the vocabulary) -> the trained flags and counts[1]."""
    lengths, _, mr = vocab
    ids = np.asarray([mr[p] for p in text_pieces], dtype=np.int32)
    offs = np.asarray([0, len(ids)], dtype=np.int64)
    ro = np.asarray([0, len(ranges)], dtype=np.int64)
    rg = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    w = rt.ranges_walk(ids, offs, ro, rg, lengths, rule, -100, starts)
    _same(w, rt.ranges_numpy(ids, offs, ro, rg, lengths, rule, -100, starts), (ranges, rule))
    assert np.array_equal(w[0], np.where(w[1] == 1, ids, -100))
    return w[1].tolist(), int(w[3][1])


def _pieces(vocab):
    """Three ids of three bytes each: they lie at [0, 3) [3, 6) [6, 9), the middle one is the id under test."""
    return [b for b in (b"abc", b"the", b"ing", b"and", b"ion", b"ent") if b in vocab[2]][:3]


@pytest.mark.parametrize("ranges,overlap,inside,start,partial", [
    ([(4, 9)], [0, 1, 1], [0, 0, 1], [0, 0, 1], 1),           # astride a range's left edge
    ([(0, 5)], [1, 1, 0], [1, 0, 0], [1, 1, 0], 1),           # astride its right edge
    ([(3, 4), (4, 6)], [0, 1, 0], [0, 1, 0], [0, 1, 0], 0),   # two touching ranges cover it: they behave as one
    ([(3, 4), (5, 6)], [0, 1, 0], [0, 0, 0], [0, 1, 0], 1),   # ... with a byte between them they do not
    ([(4, 4)], [0, 0, 0], [0, 0, 0], [0, 0, 0], 0),           # an empty range inside it marks nothing
    ([(3, 3), (3, 6), (6, 6)], [0, 1, 0], [0, 1, 0], [0, 1, 0], 0),  # empty ranges at both of its edges
    ([(4, 5)], [0, 1, 0], [0, 0, 0], [0, 0, 0], 1),           # a range of one byte, shorter than the id
    ([(3, 4)], [0, 1, 0], [0, 0, 0], [0, 1, 0], 1),           # only its first byte
    ([(0, 9)], [1, 1, 1], [1, 1, 1], [1, 1, 1], 0),           # the whole document, ending exactly at its end
    ([], [0, 0, 0], [0, 0, 0], [0, 0, 0], 0),
])
def test_hand_cases_pin_every_rule(vocab, ranges, overlap, inside, start, partial):
    PIECES = _pieces(vocab)
    assert len(PIECES) == 3
    for rule, want in (("overlap", overlap), ("inside", inside), ("start", start)):
        got, n_partial = _one(vocab, PIECES, ranges, rule)
        assert got == want and n_partial == partial, (ranges, rule, got, n_partial)


def test_explicit_starts_with_skipped_text(vocab):
    # the ids lie at [2, 5) [7, 10) [10, 13): the text has two bytes in front of the first id and between the first two
    starts = np.asarray([2, 7, 10], dtype=np.int64)
    PIECES = _pieces(vocab)
    assert _one(vocab, PIECES, [(0, 2), (5, 8)], "overlap", starts) == ([0, 1, 0], 1)
    assert _one(vocab, PIECES, [(0, 2), (5, 8)], "start", starts) == ([0, 1, 0], 1)
    assert _one(vocab, PIECES, [(2, 7), (10, 40)], "inside", starts) == ([1, 0, 1], 0)


# ---- the CPU model over the shared header -------------------------------------------------------------------------------------------
ROOT = Path(__file__).resolve().parents[1]
RULE_ID = {"overlap": 0, "inside": 1, "start": 2}


@pytest.fixture(scope="module")
def model(vocab):
    src = ROOT / "tests" / "twin" / "ranges_model.cpp"
    out = ROOT / "tests" / "twin" / "_build" / "librangesmodel.so"
    out.parent.mkdir(parents=True, exist_ok=True)
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))  # (td_ranges_args.h declares its launch with HIP's host types)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__",
                           f"-I{rocm / 'include'}", str(src), "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    lib.ranges_model.restype = ctypes.c_int
    lib.ranges_model.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 8
    lib.ranges_model_defaults.argtypes = [ctypes.c_void_p]
    lengths = np.ascontiguousarray(vocab[0], dtype=np.int64)

    def run(ids, offs, ro, rg, rule, ignore, sizes, rng, starts=None):
        """-> ((labels, mask, trained_offsets, counts) | None, (code, err_pos), kinds[6])"""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        offs, ro = np.ascontiguousarray(offs, dtype=np.int64), np.ascontiguousarray(ro, dtype=np.int64)
        rg = np.ascontiguousarray(rg, dtype=np.int64).reshape(-1, 2)
        st = None if starts is None else np.ascontiguousarray(starts, dtype=np.int64)
        total = int(offs[-1])
        sz = np.asarray(sizes, dtype=np.int64)
        order = rng.permutation(-(-total // int(sz[0]))).astype(np.int64)
        labels = np.full(max(total, 1), 12345, dtype=np.int32)
        mask = np.full(max(total, 1), 77, dtype=np.uint8)
        toff = np.full(len(offs), -1, dtype=np.int64)
        counts = np.full(4, -1, dtype=np.int64)
        kinds = np.zeros(6, dtype=np.int64)
        pos = ctypes.c_int64(-1)
        rc = lib.ranges_model(ids.ctypes.data, len(ids), offs.ctypes.data, len(offs) - 1, st.ctypes.data if st is not None else None, ro.ctypes.data,
                              rg.ctypes.data, len(rg), RULE_ID[rule], ignore, lengths.ctypes.data, len(lengths), sz.ctypes.data, order.ctypes.data,
                              labels.ctypes.data, mask.ctypes.data, toff.ctypes.data, counts.ctypes.data, ctypes.byref(pos), kinds.ctypes.data)
        assert rc >= 0, rc
        return (labels[:total], mask[:total], toff, counts) if rc == 0 else None, (rc, pos.value), kinds
    run.lib = lib
    return run


def test_model_defaults_are_the_kernels_sizes(model):
    d = np.zeros(7, dtype=np.int64)
    model.lib.ranges_model_defaults(d.ctypes.data)
    csrc = ROOT / "tokendagger_amd" / "csrc"

    def const(text, name):
        m = re.search(r"constexpr int " + name + r" = ([0-9]+);", text)
        assert m, name
        return int(m.group(1))
    common, lab, args = (csrc / "td_rows_common.h").read_text(), (csrc / "td_labels_args.h").read_text(), (csrc / "td_ranges_args.h").read_text()
    assert re.search(r"constexpr int RNG_TILE = LAB_TILE;", args) and const(common, "RC_TILE") == const(lab, "LAB_TILE")
    # tile, window, table, the table's step (a workgroup), range chunk, the chunks a pass of chunks_excl_scan takes, ids a lane
    assert d.tolist() == [const(lab, "LAB_TILE"), const(args, "RNG_WIN"), const(common, "RC_LDS_DOCS"), const(common, "RC_THREADS"),
                          const(args, "RNG_CHUNK"), 4 * const(common, "RC_THREADS"), const(lab, "LAB_TILE") // const(lab, "LAB_THREADS")]
    assert const(common, "RC_SCAN_CHUNK") == const(args, "RNG_CHUNK")


def _small_sizes(rng):
    """tile 4 - 64, window 1 - 8, table 2 - 16 (a multiple of its step), chunk 4 - 16, chunks a pass 1 - 4, ids a lane 1 - 8"""
    step = int(rng.integers(1, 5))
    return [int(rng.integers(4, 65)), int(rng.integers(1, 9)), step * int(rng.integers(max(1, -(-2 // step)), 16 // step + 1)), step,
            int(rng.integers(4, 17)), int(rng.integers(1, 5)), int(rng.integers(1, 9))]


def _with_empty_runs(rng, lengths, pool, sparse=False):
    """A random case with runs of empty documents spliced in, some of them with empty ranges (0, 0).  sparse: most documents lose
    their ranges and the runs have none, so that a tile of many documents still has a small window."""
    ids, offs, ro, rg = rt.random_case(rng, lengths, pool, max_docs=10 if not sparse else 40, max_len=30 if not sparse else 6)
    n_ids = np.diff(offs).tolist()
    per = [rg[ro[d]:ro[d + 1]] if not sparse or rng.random() < 0.15 else rg[:0] for d in range(len(n_ids))]
    for _ in range(int(rng.integers(1, 4))):
        at, run = int(rng.integers(0, len(n_ids) + 1)), int(rng.integers(3, 40))
        p_tag = 0.0 if sparse else (0.0, 0.1, 0.5)[int(rng.integers(0, 3))]
        tags = [np.zeros((int(rng.random() < p_tag), 2), dtype=np.int64) for _ in range(run)]
        n_ids[at:at] = [0] * run
        per[at:at] = tags
    offs = np.concatenate([[0], np.cumsum(n_ids)]).astype(np.int64)
    ro = np.concatenate([[0], np.cumsum([len(r) for r in per])]).astype(np.int64)
    rg = np.concatenate(per).reshape(-1, 2) if per else np.zeros((0, 2), np.int64)
    return ids, offs, ro, rg.astype(np.int64)


def _gapped(rng, ids, offs, lengths):
    """Covering starts plus a gap of 0 - 2 bytes in front of every id."""
    doc = np.repeat(np.arange(len(offs) - 1), np.diff(offs))
    gaps = np.concatenate([[0], np.cumsum(rng.integers(0, 3, len(ids)))])
    return (OT.covered_byte_starts(ids, offs, lengths) + gaps[1:] - gaps[offs[doc]]).astype(np.int64)


def test_model_equals_both_truths_with_small_sizes(vocab, model):
    lengths, pool, _ = vocab
    rng = np.random.default_rng(77)
    seen = np.zeros(6, dtype=np.int64)
    for it in range(1500):
        if it % 3 == 0:
            ids, offs, ro, rg = _with_empty_runs(rng, lengths, pool, sparse=it % 2 == 0)
        else:
            ids, offs, ro, rg = rt.random_case(rng, lengths, pool, max_docs=12 if it % 8 else 60)
        sizes = _small_sizes(rng)
        ign = int(rng.integers(-5, 3))
        covering = OT.covered_byte_starts(ids, offs, lengths)
        for rule in rt.RULES:
            want = rt.ranges_numpy(ids, offs, ro, rg, lengths, rule, ign)
            got, status, kinds = model(ids, offs, ro, rg, rule, ign, sizes, rng)
            assert status[0] == 0, (it, rule, sizes, status)
            _same(got, want, (it, rule, sizes))
            seen += kinds
            got, status, kinds = model(ids, offs, ro, rg, rule, ign, sizes, rng, starts=covering)
            assert status[0] == 0
            _same(got, want, (it, rule, sizes, "explicit"))
            seen += kinds
            if it % 5 == 0:
                _same(got, rt.ranges_walk(ids, offs, ro, rg, lengths, rule, ign), (it, rule, "walk"))
        rule = rt.RULES[it % 3]
        st = _gapped(rng, ids, offs, lengths)
        got, status, kinds = model(ids, offs, ro, rg, rule, ign, sizes, rng, starts=st)
        assert status[0] == 0
        _same(got, rt.ranges_numpy(ids, offs, ro, rg, lengths, rule, ign, st), (it, rule, sizes, "gapped"))
        if it % 5 == 0:
            _same(got, rt.ranges_walk(ids, offs, ro, rg, lengths, rule, ign, st), (it, "gapped walk"))
        seen += kinds
    # tiles that fit / do not fit the table x windows staged / not staged; staged windows across a chunk border; later passes of the scan
    assert (seen >= 1000).all(), seen.tolist()


def test_model_with_the_kernels_sizes(vocab, model):
    lengths, pool, _ = vocab
    rng = np.random.default_rng(78)
    d = np.zeros(7, dtype=np.int64)
    model.lib.ranges_model_defaults(d.ctypes.data)
    n_ids = np.concatenate([[3000], np.zeros(4400, dtype=np.int64), [2000, 300], np.zeros(30, dtype=np.int64), [4000]])
    offs = np.concatenate([[0], np.cumsum(n_ids)]).astype(np.int64)
    ids = pool[rng.integers(0, len(pool), int(offs[-1]))]
    cs = np.concatenate([[0], np.cumsum(lengths[ids])])
    sizes = cs[offs[1:]] - cs[offs[:-1]]
    per = [np.sort(rng.integers(0, s + 1, 2 * ((300 if d_ else 60) if s else int(d_ % 4 == 0)))).reshape(-1, 2) for d_, s in enumerate(sizes.tolist())]
    ro = np.concatenate([[0], np.cumsum([len(r) for r in per])]).astype(np.int64)
    rg = np.concatenate(per).astype(np.int64)
    seen = np.zeros(6, dtype=np.int64)
    for rule in rt.RULES:
        for st in (None, OT.covered_byte_starts(ids, offs, lengths)):
            got, status, kinds = model(ids, offs, ro, rg, rule, -100, d.tolist(), rng, starts=st)
            assert status[0] == 0
            _same(got, rt.ranges_numpy(ids, offs, ro, rg, lengths, rule), rule)
            seen += kinds
    # a tile beyond the table and the window, one beyond the window, one within both whose window lies across range 2048
    assert (seen[[0, 2, 3, 4]] == 6).all(), seen.tolist()


def _first_bad(offs, ro, rg, doc_sizes):
    """What the contract names: the lowest range that is negative, reversed or begins in front of the end before it in its document;
    if there is none and doc_sizes is given (the covered form), the lowest range that ends beyond its document."""
    beyond = None
    order = None
    for d in range(len(ro) - 1):
        prev = 0
        for r in range(int(ro[d]), int(ro[d + 1])):
            b, e = int(rg[r, 0]), int(rg[r, 1])
            if order is None and (b < prev or e < b):
                order = r
            if beyond is None and doc_sizes is not None and e > doc_sizes[d]:
                beyond = r
            prev = e
    return order if order is not None else beyond


def test_model_reports_the_index_the_contract_names(vocab, model):
    lengths, pool, _ = vocab
    rng = np.random.default_rng(79)
    n_order = n_beyond = n_both = 0
    for it in range(600):
        ids, offs, ro, rg = _with_empty_runs(rng, lengths, pool) if it % 2 else rt.random_case(rng, lengths, pool)
        if len(rg) == 0:
            continue
        cs = np.concatenate([[0], np.cumsum(lengths[ids])])
        doc_sizes = (cs[offs[1:]] - cs[offs[:-1]]).tolist()
        rdoc = np.repeat(np.arange(len(ro) - 1), np.diff(ro))
        bad = rg.copy()
        kinds_of = []
        for r in rng.integers(0, len(rg), int(rng.integers(1, 4))).tolist():
            kind = int(rng.integers(0, 4)) if it % 3 else 3
            kinds_of.append(kind)
            if kind == 0:
                bad[r] = (bad[r, 1] + 1, bad[r, 0])        # reversed
            elif kind == 1:
                bad[r, 0] = -1 - int(rng.integers(0, 3))   # negative
            elif kind == 2 and r > ro[rdoc[r]]:
                bad[r, 0] = bad[r - 1, 1] - 1              # begins inside the range before it (or is negative)
            else:
                bad[r, 1] = max(doc_sizes[rdoc[r]], bad[r, 0]) + 1 + int(rng.integers(0, 3))  # ends beyond its document
                if r + 1 < ro[rdoc[r] + 1]:
                    bad[r + 1:ro[rdoc[r] + 1]] = bad[r, 1]  # (what follows stays in order: empty ranges further out still)
        sizes = _small_sizes(rng)
        want = _first_bad(offs, ro, bad, doc_sizes)
        assert want is not None
        _, status, _ = model(ids, offs, ro, bad, rt.RULES[it % 3], -100, sizes, rng)
        assert status == (1, want), (it, status, want, sizes)
        in_order = _first_bad(offs, ro, bad, None)
        n_order += in_order is not None
        n_beyond += in_order is None
        n_both += in_order is not None and any(k == 3 for k in kinds_of)
        # the explicit form checks the order only
        got, status, _ = model(ids, offs, ro, bad, "overlap", -100, sizes, rng, starts=OT.covered_byte_starts(ids, offs, lengths))
        if in_order is not None:
            assert status == (1, in_order), (it, status, in_order)
        else:
            assert status[0] == 0
            _same(got, rt.ranges_numpy(ids, offs, ro, bad, lengths, "overlap", -100, OT.covered_byte_starts(ids, offs, lengths)))
    assert n_order >= 100 and n_beyond >= 100 and n_both >= 20, (n_order, n_beyond, n_both)
    # bad offsets: the document
    ids, offs, ro, rg = rt.random_case(np.random.default_rng(5), lengths, pool, max_docs=12)
    assert len(offs) > 4 and len(rg) > 2
    for which, d, v in (("tok", 2, -1), ("range", 3, -2), ("tok", 0, 1), ("range", 0, 1)):
        o, r = offs.copy(), ro.copy()
        (o if which == "tok" else r)[d] = v
        _, status, _ = model(ids, o, r, rg, "overlap", -100, [8, 4, 4, 2, 4, 2, 2], rng)
        assert status[0] == 1 and 0 <= status[1] < len(offs) - 1, (which, d, status)


def _plan_fails(capi, ranges, doc_lens=None):
    with pytest.raises(capi.TokenDaggerHipError) as e:
        capi.range_plan(ranges, doc_lens)
    assert e.value.code == capi.TD_E_INVALID
    return e.value.bad


def test_range_plan_through_the_c_abi(vocab):
    import __graft_entry__ as g
    g.build_hip()
    from tokendagger_amd import capi
    lengths, pool, _ = vocab
    rng = np.random.default_rng(9)
    for it in range(100):
        ids, offs, ro, rg = rt.random_case(rng, lengths, pool)
        doc_lens = np.asarray([int(lengths[ids[offs[d]:offs[d + 1]]].sum()) for d in range(len(offs) - 1)], dtype=np.int64)
        want = [int((rg[:, 1] > rg[:, 0]).sum()), int((rg[:, 1] - rg[:, 0]).sum())]
        assert capi.range_plan((ro, rg)).tolist() == want
        assert capi.range_plan((ro, rg), doc_lens).tolist() == want
        per_doc = [rg[ro[d]:ro[d + 1]].tolist() for d in range(len(offs) - 1)]
        assert capi.range_plan(per_doc).tolist() == want  # (the list form)
    good = [[(0, 2), (2, 5)], [], [(1, 1), (3, 9), (9, 9)]]   # global range indices 0 1 | | 2 3 4
    assert capi.range_plan(good).tolist() == [3, 11]
    assert capi.range_plan(good, [5, 0, 9]).tolist() == [3, 11]
    assert _plan_fails(capi, [[(0, 2), (2, 5)], [], [(1, 1), (9, 3), (9, 9)]]) == 3      # reversed
    assert _plan_fails(capi, [[(0, 2), (1, 5)], [], [(1, 1)]]) == 1                        # overlapping
    assert _plan_fails(capi, [[(0, 2)], [], [(4, 6), (1, 2), (7, 8)]]) == 2                # unsorted
    assert _plan_fails(capi, [[(0, 2)], [(-1, 2)], [(4, 6)]]) == 1                         # negative
    assert _plan_fails(capi, good, [5, 0, 8]) == 3                                         # beyond doc_lens (the first such range)
    assert _plan_fails(capi, good, [4, 0, 9]) == 1
    assert _plan_fails(capi, [[], [(0, 1)]], [3, 0]) == 0                                  # a document without bytes
    rg = np.asarray([(0, 1), (2, 3), (4, 5)], dtype=np.int64)
    assert _plan_fails(capi, (np.asarray([0, 2, 1, 3]), rg)) == 1                          # bad range_offsets: decreasing at document 1
    assert _plan_fails(capi, (np.asarray([1, 2, 3]), rg)) == 0                             # not starting at 0
    assert _plan_fails(capi, (np.asarray([0, -1, 3]), rg)) == 0                            # negative
    with pytest.raises(ValueError):
        capi.range_plan((np.asarray([0, 2, 4]), rg))                                       # more ranges than the array has
    with pytest.raises(ValueError):
        capi.range_spec("middle")


def test_chars_to_bytes_against_str_slicing():
    import __graft_entry__ as g
    g.build_hip()
    from tokendagger_amd import capi
    rng = np.random.default_rng(2)
    alphabet = ["a", "é", "ß", "中", "文", "\U0001F600", " ", "\n", "z", "ñ", "́", "€"]
    docs = ["".join(alphabet[i] for i in rng.integers(0, len(alphabet), n)) for n in (0, 1, 7, 40, 0, 300, 2)]
    docs.append("plain ascii only")
    text, offs = H.pack_docs([d.encode("utf-8") for d in docs])
    per_doc, want = [], []
    for d in docs:
        cuts = np.sort(rng.integers(0, len(d) + 1, 2 * int(rng.integers(0, 5)))).reshape(-1, 2).tolist()
        if d and rng.random() < 0.7:
            cuts.append((cuts[-1][1] if cuts else 0, len(d)))  # a range that ends at the document's end
        per_doc.append(cuts)
        want += [(len(d[:a].encode("utf-8")), len(d[:b].encode("utf-8"))) for a, b in cuts]
    ro, rg = capi.chars_to_bytes(text, offs, per_doc)
    assert ro.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in per_doc])]).tolist()
    assert rg.dtype == np.int64 and rg.tolist() == [list(w) for w in want]
    # the bytes a converted range selects are the characters the str slice selects
    data = bytes(text) if not isinstance(text, bytes) else text
    for d, doc in enumerate(docs):
        for (a, b), (ba, bb) in zip(per_doc[d], rg[ro[d]:ro[d + 1]].tolist()):
            assert data[offs[d] + ba:offs[d] + bb].decode("utf-8") == doc[a:b]
    with pytest.raises(ValueError):
        capi.chars_to_bytes(text, offs, [[(0, len(d) + 1)] for d in docs])  # behind the last character
