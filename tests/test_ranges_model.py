"""Loss labels from byte ranges without a GPU: the two truths of tests/ranges_truth.py against each other and against hand-written
cases, td_range_plan through the C ABI, and the character-to-byte conversion of the text forms."""
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
