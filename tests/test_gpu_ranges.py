"""Loss labels from byte ranges on the GPU (td_range_labels, td_range_labels_device, td_encode_batch_range_labels,
td_encode_batch_range_label_rows, the Python methods) against ranges_numpy of tests/ranges_truth.py.  All comparisons are exact.
No case here makes the device fault: every error is one the library reports by a status code.

The sizes the cases are built around (tokendagger_amd/csrc/td_ranges_args.h): a workgroup labels a TILE of 4096 ids, sixteen a
lane; the ranges a tile's ids can touch are searched in LDS when there are at most WIN = 512 of them, in global memory otherwise;
one round of the carry kernel covers 1024 tiles."""
import numpy as np
import pytest

import helpers as H
import offsets_truth as OT
import ranges_truth as rt
from ranges_gpu_helpers import (TILE, WIN, _bulk_ranges, _check, _device_alloc, _device_call, _doc_sizes, _every_other_byte,  # noqa: F401
                                _same, _spec, tok, vocab)

pytestmark = pytest.mark.gpu

CARRY_ROUND = 1024 * TILE
OPENER = b"<|header_start|>assistant<|header_end|>"
CLOSERS = [b"<|eot|>", b"<|eom|>"]
AUTOGEN = r"[a-zA-Z]+|\s+|[0-9]+|[^\w\s]"  # skips '_' and 'é'
COMBOS = [(m, o) for m in (False, True) for o in (False, True)]


@pytest.fixture(scope="module")
def wtok():
    from tokendagger_amd import wrapper
    return wrapper.llama4_scout(0)


def test_random_cases(tok, vocab):
    lengths, pool = vocab[3], vocab[4]
    rng = np.random.default_rng(31)
    for it in range(150):
        ids, offs, ro, rg = rt.random_case(rng, lengths, pool, max_docs=12 if it % 8 else 300)
        rule = rt.RULES[it % 3]
        _check(tok, lengths, ids, offs, ro, rg, rules=(rule,), combos=(COMBOS[it % 4],), ignore=int(rng.integers(-5, 3)))
        if it % 10 == 0:
            _same(rt.ranges_numpy(ids, offs, ro, rg, lengths, rule), rt.ranges_walk(ids, offs, ro, rg, lengths, rule), it)


def test_three_tiles_one_document_three_ranges_every_rule_and_output(tok, vocab):
    lengths, pool = vocab[3], vocab[4]
    rng = np.random.default_rng(1)
    n = 3 * TILE + 100
    ids = pool[rng.integers(0, len(pool), n)]
    offs = np.asarray([0, n], dtype=np.int64)
    s = OT.covered_byte_starts(ids, offs, lengths)
    size = int(s[-1] + lengths[ids[-1]])
    # out of tile 0 into tile 1 from the middle of an id; inside tile 1, one byte; from tile 2 to the document's end
    rg = np.asarray([(s[TILE - 30] + 1, s[TILE + 40] + 1), (s[TILE + 2000] + 1, s[TILE + 2000] + 2), (s[2 * TILE + 5], size)], dtype=np.int64)
    t = _check(tok, lengths, ids, offs, np.asarray([0, 3]), rg, combos=COMBOS)
    assert t["overlap"][3][0] > t["inside"][3][0] > 1000 and t["overlap"][3][1] >= 2
    _same(t["start"], rt.ranges_walk(ids, offs, [0, 3], rg, lengths, "start"))


def test_twenty_thousand_small_documents(tok, vocab):
    lengths, pool = vocab[3], vocab[4]
    rng = np.random.default_rng(2)
    n_ids = rng.integers(0, 6, 20000)
    n_ids[TILE // 3:TILE // 3 + 40] = 0           # a run of empty documents
    offs = np.concatenate([[0], np.cumsum(n_ids)]).astype(np.int64)
    for t in range(1, int(offs[-1]) // TILE):     # empty documents exactly at tile edges
        d = int(np.searchsorted(offs, t * TILE))
        if offs[d] == t * TILE and d + 1 < len(offs) - 1:
            n_ids[d] = 0
    offs = np.concatenate([[0], np.cumsum(n_ids)]).astype(np.int64)
    ids = pool[rng.integers(0, len(pool), int(offs[-1]))]
    ro, rg = _bulk_ranges(rng, _doc_sizes(lengths, ids, offs), 2)
    t = _check(tok, lengths, ids, offs, ro, rg)
    assert len(t["overlap"][2]) == 20001 and t["overlap"][3][0] > 5000 and t["overlap"][3][1] > 500


@pytest.mark.parametrize("off", [-1, 0, 1])
def test_document_and_range_edges_on_a_tile_boundary(tok, vocab, off):
    lengths, pool = vocab[3], vocab[4]
    rng = np.random.default_rng(3)
    n = 2 * TILE + 50
    ids = pool[rng.integers(0, len(pool), n)]
    q = TILE + off
    # two documents that meet at id q: a range up to the end of the first, a range from the start of the second
    offs = np.asarray([0, q, n], dtype=np.int64)
    sizes = _doc_sizes(lengths, ids, offs)
    s = OT.covered_byte_starts(ids, offs, lengths)
    rg = np.asarray([(s[q - 3], sizes[0]), (0, s[q + 2])], dtype=np.int64)
    t = _check(tok, lengths, ids, offs, np.asarray([0, 1, 2]), rg)
    assert t["inside"][1][q - 3:q + 2].tolist() == [1, 1, 1, 1, 1] and t["inside"][1][q - 4] == 0 and t["inside"][1][q + 2] == 0
    # one document: a range that ends, and one that begins, exactly where id q begins
    offs = np.asarray([0, n], dtype=np.int64)
    s = OT.covered_byte_starts(ids, offs, lengths)
    for rg in ([(s[q - 5], s[q])], [(s[q], s[q + 5])], [(s[q - 5], s[q]), (s[q], s[q + 5])], [(s[q] - 1, s[q] + 1)]):
        t = _check(tok, lengths, ids, offs, np.asarray([0, len(rg)]), np.asarray(rg, dtype=np.int64))
    assert t["overlap"][1][q - 1:q + 1].tolist() == [1, 1] and t["overlap"][3][1] == int(lengths[ids[q - 1]] > 1) + int(lengths[ids[q]] > 1)


def test_one_byte_ranges_on_every_other_byte_search_global_memory(tok, vocab):
    lengths = vocab[3]
    rng = np.random.default_rng(4)
    long_ids = np.flatnonzero((lengths >= 4) & (lengths <= 9))[:50].astype(np.int32)
    n = 2 * TILE + 77
    ids = long_ids[rng.integers(0, len(long_ids), n)]
    offs = np.asarray([0, 1000, n], dtype=np.int64)
    sizes = _doc_sizes(lengths, ids, offs)
    rg = np.concatenate([_every_other_byte(int(sizes[0]) // 2), _every_other_byte(int(sizes[1]) // 2)])
    ro = np.asarray([0, sizes[0] // 2, len(rg)], dtype=np.int64)
    assert len(rg) > n and len(rg) // 3 > WIN  # more ranges than ids; every tile's window is beyond the LDS limit
    t = _check(tok, lengths, ids, offs, ro, rg)
    assert t["inside"][3][0] == 0 and t["overlap"][3][0] == n and t["overlap"][3][1] == n


@pytest.mark.parametrize("n_ranges", [WIN - 1, WIN, WIN + 1])
def test_a_window_at_the_lds_limit(tok, vocab, n_ranges):
    """One tile, one document: every range of the document can be touched by the tile, so the window is the document's ranges;
    WIN of them are searched in LDS, WIN + 1 in global memory."""
    lengths = vocab[3]
    rng = np.random.default_rng(5)
    long_ids = np.flatnonzero((lengths >= 4) & (lengths <= 9))[:50].astype(np.int32)
    ids = long_ids[rng.integers(0, len(long_ids), TILE - 9)]
    offs = np.asarray([0, len(ids)], dtype=np.int64)
    rg = _every_other_byte(n_ranges) + 6
    t = _check(tok, lengths, ids, offs, np.asarray([0, n_ranges]), rg)
    assert t["overlap"][3][2] == n_ranges and t["overlap"][3][0] > 150


def test_more_ids_than_one_round_of_the_carry_kernel(tok, vocab):
    lengths, pool = vocab[3], vocab[4]
    rng = np.random.default_rng(6)
    n = CARRY_ROUND + 2 * TILE + 11
    ids = pool[rng.integers(0, len(pool), n)]
    offs = np.asarray([0, 5, CARRY_ROUND - 3, CARRY_ROUND - 3, n], dtype=np.int64)
    sizes = _doc_sizes(lengths, ids, offs)
    ro, out = [0], []
    for size in sizes.tolist():
        out.append(np.sort(rng.integers(0, size + 1, 2000 if size > 1000 else 2)).reshape(-1, 2))
        ro.append(ro[-1] + len(out[-1]))
    out[-1][-1, 1] = sizes[-1]
    t = _check(tok, lengths, ids, offs, np.asarray(ro, dtype=np.int64), np.concatenate(out).astype(np.int64), rules=("inside",))
    assert t["inside"][3][0] > n // 4 and t["inside"][2][-1] == t["inside"][3][0]


def test_ids_longer_than_64_bytes(tok, vocab):
    lengths = vocab[3]
    giants = np.flatnonzero(lengths > 64).astype(np.int32)
    assert len(giants) >= 8, "the Llama-4 vocabulary has whitespace and punctuation tokens of up to 113 bytes"
    rng = np.random.default_rng(7)
    ids = giants[rng.integers(0, len(giants), TILE + 300)]
    offs = np.asarray([0, 17, 17, TILE + 300], dtype=np.int64)
    ro, rg = _bulk_ranges(rng, _doc_sizes(lengths, ids, offs), 40)
    t = _check(tok, lengths, ids, offs, ro, rg)
    assert t["overlap"][3][1] > 20


def test_explicit_starts_equal_the_covered_form(tok, vocab):
    lengths, pool = vocab[3], vocab[4]
    rng = np.random.default_rng(8)
    n_ids = rng.integers(0, 700, 30)
    offs = np.concatenate([[0], np.cumsum(n_ids)]).astype(np.int64)
    ids = pool[rng.integers(0, len(pool), int(offs[-1]))]
    ro, rg = _bulk_ranges(rng, _doc_sizes(lengths, ids, offs), 30)
    starts = tok.token_starts(ids, offs)
    assert np.array_equal(starts, OT.covered_byte_starts(ids, offs, lengths))
    for rule in rt.RULES:
        covered = tok.range_labels(ids, offs, (ro, rg), _spec(rule), mask=True, trained_offsets=True)
        explicit = tok.range_labels(ids, offs, (ro, rg), _spec(rule), mask=True, trained_offsets=True, starts=starts)
        _same(explicit, covered, rule)
        _same(covered, rt.ranges_numpy(ids, offs, ro, rg, lengths, rule))


def _autogen_docs():
    rng = np.random.default_rng(3)
    words = ["snake_case", "é", "_", "__init__", "naïve", "café", "x", "42", "!", " ", "\n", "émigré", "_é_", "中文", "\U0001F600"]
    docs = ["_leading gap", "middle_gap here", "trailing gap_", "___", "", "é", "", "plain text 1 2 3"]
    for n in (100, 5000):
        docs.append("".join(words[i] + (" " if i % 3 else "") for i in rng.integers(0, len(words), n)))
    return [d.encode("utf-8") for d in docs]


def test_explicit_starts_on_a_pattern_that_skips_text(vocab):
    from tokendagger_amd import capi
    lengths = vocab[3]
    t = capi.HipTokenizer(AUTOGEN, vocab[1], vocab[2], device=0)
    docs = _autogen_docs()
    text, offs = H.pack_docs(docs)
    ids, toffs, starts = t.encode_batch_with_starts(text, offs, unit=capi.TD_UNIT_BYTES)
    assert not np.array_equal(starts, OT.covered_byte_starts(ids, toffs, lengths)), "the documents must skip text"
    rng = np.random.default_rng(9)
    ro, rg = _bulk_ranges(rng, np.diff(np.asarray(offs, dtype=np.int64)), 25)
    for rule in rt.RULES:
        want = rt.ranges_numpy(ids, toffs, ro, rg, lengths, rule, -100, starts)
        _same(t.range_labels(ids, toffs, (ro, rg), _spec(rule), mask=True, trained_offsets=True, starts=starts), want, rule)
        _same(want, rt.ranges_walk(ids, toffs, ro, rg, lengths, rule, -100, starts), rule)
    assert want[3][0] > 100
    # the text form cannot know where the ids lie: it says so
    with pytest.raises(capi.TokenDaggerHipError) as e:
        t.encode_batch_range_labels(text, offs, [], (ro, rg), _spec())
    assert e.value.code == capi.TD_E_INVALID and "explicit starts" in str(e.value)
    # ... and the handle still works
    _same(t.range_labels(ids, toffs, (ro, rg), _spec(rule), mask=True, trained_offsets=True, starts=starts), want)
    t.close()


def test_device_form_equals_the_host_form_and_leaves_the_slots_behind_the_ids(tok, vocab):
    lengths, pool = vocab[3], vocab[4]
    rng = np.random.default_rng(10)
    n_ids = rng.integers(0, 900, 20)
    offs = np.concatenate([[0], np.cumsum(n_ids)]).astype(np.int64)
    total = int(offs[-1])
    ids = np.concatenate([pool[rng.integers(0, len(pool), total)], np.full(300, -7, dtype=np.int32)])  # 300 slots behind the ids
    ro, rg = _bulk_ranges(rng, _doc_sizes(lengths, ids[:total], offs), 12)
    for rule in rt.RULES:
        (lab, m, to, counts), status = _device_call(tok, ids, len(ids), offs, ro, rg, _spec(rule, -1))
        assert status[0] == 0
        host = tok.range_labels(ids[:total], offs, (ro, rg), _spec(rule, -1), mask=True, trained_offsets=True)
        _same((lab[:total], m[:total], to, counts), host, rule)
        _same(host, rt.ranges_numpy(ids[:total], offs, ro, rg, lengths, rule, -1))
        assert (lab[total:] == 77).all() and (m[total:] == 77).all()
    starts = OT.covered_byte_starts(ids[:total], offs, lengths)
    (lab, m, to, counts), status = _device_call(tok, ids, len(ids), offs, ro, rg, _spec("start", -1),
                                                starts=np.concatenate([starts, np.zeros(300, np.int64)]))
    assert status[0] == 0
    _same((lab[:total], m[:total], to, counts), rt.ranges_numpy(ids[:total], offs, ro, rg, lengths, "start", -1))
    assert (lab[total:] == 77).all() and (m[total:] == 77).all()


def _error_case(vocab):
    lengths, pool = vocab[3], vocab[4]
    rng = np.random.default_rng(11)
    offs = np.asarray([0, 100, 100, 5000, 9000, 3 * TILE], dtype=np.int64)
    ids = pool[rng.integers(0, len(pool), 3 * TILE)]
    ro, rg = _bulk_ranges(rng, _doc_sizes(lengths, ids, offs), 6, min_k=4)
    return lengths, ids, offs, ro, rg


def _untouched(outs):
    for o in outs:
        assert (o == 77).all()


def test_an_id_outside_the_vocabulary(tok, vocab):
    from tokendagger_amd import capi
    lengths, ids, offs, ro, rg = _error_case(vocab)
    bad = ids.copy()
    bad[[6000, 1234, 11000]] = [len(lengths) + 5, -3, len(lengths) + 9]
    starts = OT.covered_byte_starts(ids, offs, lengths)
    for st in (None, starts):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            tok.range_labels(bad, offs, (ro, rg), _spec(), starts=st)
        assert e.value.code == capi.TD_E_BAD_TOKEN and "index 1234" in str(e.value)
        _, status = _device_call(tok, bad, len(bad), offs, ro, rg, _spec(), starts=st)
        assert status == (capi.TD_E_BAD_TOKEN, 1234)
    _check(tok, lengths, ids, offs, ro, rg, rules=("overlap",))  # the handle is fine afterwards


def test_a_range_past_the_covered_bytes(tok, vocab):
    from tokendagger_amd import capi
    lengths, ids, offs, ro, rg = _error_case(vocab)
    sizes = _doc_sizes(lengths, ids, offs)
    # the last range of documents 3 and 4 one byte beyond their ids' bytes; document 1 has no ids: a range [0, 1) there is beyond too
    for docs, first in (((4,), int(ro[5]) - 1), ((3, 4), int(ro[4]) - 1)):
        far = rg.copy()
        for d in docs:
            assert ro[d + 1] > ro[d]
            far[ro[d + 1] - 1, 1] = sizes[d] + 1
        with pytest.raises(capi.TokenDaggerHipError) as e:
            tok.range_labels(ids, offs, (ro, far), _spec())
        assert e.value.code == capi.TD_E_INVALID
        _, status = _device_call(tok, ids, len(ids), offs, ro, far, _spec())
        assert status == (capi.TD_E_INVALID, first)
    ro2 = ro.copy()
    ro2[2:] += 1
    far = np.concatenate([rg[:ro[2]], [[0, 1]], rg[ro[2]:]])  # (behind the empty ranges the document may have)
    _, status = _device_call(tok, ids, len(ids), offs, ro2, far, _spec())
    assert status == (capi.TD_E_INVALID, int(ro[2]))
    # with explicit starts the upper bound is not checked: nothing is known about the document's length
    far = rg.copy()
    far[-1, 1] = sizes[4] + 1000
    starts = OT.covered_byte_starts(ids, offs, lengths)
    (lab, m, to, counts), status = _device_call(tok, ids, len(ids), offs, ro, far, _spec(), starts=starts)
    assert status[0] == 0
    _same((lab, m, to, counts), rt.ranges_numpy(ids, offs, ro, far, lengths, "overlap", -100, starts))
    _check(tok, lengths, ids, offs, ro, rg, rules=("overlap",))


@pytest.mark.parametrize("kind", ["unsorted", "overlapping", "reversed", "negative"])
def test_ranges_out_of_order_on_the_device_form(tok, vocab, kind):
    from tokendagger_amd import capi
    lengths, ids, offs, ro, rg = _error_case(vocab)
    bad = rg.copy()
    spots = []
    for d in (4, 3):  # two bad ranges: the lowest index is reported
        assert ro[d + 1] - ro[d] >= 3
        r = int(ro[d]) + 1
        bad[r - 1], bad[r] = (10, 20), (30, 40)
        if kind == "unsorted":
            bad[r] = (2, 5)
        elif kind == "overlapping":
            bad[r] = (19, 40)
        elif kind == "reversed":
            bad[r] = (40, 30)
        else:
            bad[r - 1] = (-4, 20)
            r -= 1
        bad[r + 1 if kind != "negative" else r + 2:ro[d + 1]] += 100  # (what follows stays in order)
        spots.append(r)
    outs, status = _device_call(tok, ids, len(ids), offs, ro, bad, _spec())
    assert status == (capi.TD_E_INVALID, min(spots)), (status, spots)
    _untouched(outs)
    with pytest.raises(capi.TokenDaggerHipError) as e:
        tok.range_labels(ids, offs, (ro, bad), _spec())
    assert e.value.code == capi.TD_E_INVALID and f"range {min(spots)} " in str(e.value)
    _check(tok, lengths, ids, offs, ro, rg, rules=("overlap",))


@pytest.mark.parametrize("kind", ["tok decreasing", "tok negative", "tok beyond", "tok nonzero start", "range decreasing", "range negative",
                                  "range nonzero start", "range end"])
def test_bad_offsets_raise_through_device_status_and_write_nothing(tok, vocab, kind):
    from tokendagger_amd import capi
    lengths, ids, offs, ro, rg = _error_case(vocab)
    o, r, n = offs.copy(), ro.copy(), len(ids)
    if kind == "tok decreasing":
        o[3] = 50
    elif kind == "tok negative":
        o[1] = -3
    elif kind == "tok beyond":
        n = 3 * TILE - 5
    elif kind == "tok nonzero start":
        o[0] = 2
    elif kind == "range decreasing":
        r[4] = r[3] - 1
    elif kind == "range negative":
        r[1] = -2
    elif kind == "range nonzero start":
        r[0] = 1
    else:
        r[5] -= 1
    outs, status = _device_call(tok, ids, n, o, r, rg, _spec())
    assert status[0] == capi.TD_E_INVALID and 0 <= status[1] < len(offs) - 1, status
    _untouched(outs)
    if kind not in ("tok beyond", "range end"):  # (the host form has no n_tokens / n_ranges of its own to disagree with)
        with pytest.raises((capi.TokenDaggerHipError, ValueError)):
            tok.range_labels(ids, o, (r, rg), _spec())
    _check(tok, lengths, ids, offs, ro, rg, rules=("overlap",))
    for bad_spec in (capi.RangeSpec(3, -100, 0), capi.RangeSpec(0, -100, 1), capi.RangeSpec(0, 1 << 40, 0)):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            tok.range_labels(ids, offs, (ro, rg), bad_spec)
        assert e.value.code == capi.TD_E_INVALID and "td_range_labels" in str(e.value)


def _chat_ranges(text, doffs, train_close):
    """The assistant-content byte ranges of chat text, by searching the literals in the bytes: from behind an opener (while outside a
    span) to the next closer (with train_close: to its end), or to the document's end."""
    import re
    pat = re.compile(b"|".join(re.escape(x) for x in [OPENER] + CLOSERS))
    data = bytes(text)
    per_doc = []
    for d in range(len(doffs) - 1):
        doc = data[doffs[d]:doffs[d + 1]]
        mine, begin = [], None
        for m in pat.finditer(doc):
            if m.group() == OPENER:
                if begin is None:
                    begin = m.end()
            elif begin is not None:
                mine.append((begin, m.end() if train_close else m.start()))
                begin = None
        if begin is not None:
            mine.append((begin, len(doc)))
        per_doc.append(mine)
    return per_doc


@pytest.fixture(scope="module")
def chat():
    import td_corpus
    return td_corpus.chat(384 << 10, seed=5)


@pytest.mark.parametrize("train_close", [False, True])
def test_chat_ranges_equal_the_span_labels(wtok, chat, train_close):
    """Two device features against each other: special tokens are pieces of their own, so every edge of these ranges is an edge
    of an id, the three rules coincide and no id is partially marked."""
    text, doffs = chat
    span = wtok.encode_batch_to_labels(text, doffs, open=[OPENER.decode()], close=[c.decode() for c in CLOSERS], train_close=train_close,
                                       mask=True, trained_offsets=True)
    ranges = _chat_ranges(text, doffs, train_close)
    assert span.counts[0] > 5000 and sum(len(r) for r in ranges) == span.counts[1] >= 50
    for rule in rt.RULES:
        r = wtok.encode_batch_to_range_labels(text, doffs, ranges, rule=rule, mask=True, trained_offsets=True)
        assert np.array_equal(r.ids, span.ids) and np.array_equal(r.tok_offsets, span.tok_offsets)
        _same((r.labels, r.mask, r.trained_offsets), (span.labels, span.mask, span.trained_offsets), rule)
        assert r.counts.tolist() == [int(span.counts[0]), 0, sum(e - b for d in ranges for b, e in d), 0]
    r2 = wtok.ids_to_range_labels(span.ids, span.tok_offsets, ranges, rule="inside")
    assert np.array_equal(r2.labels, span.labels) and r2.mask is None and r2.trained_offsets is None


def _rows_equal(a, b, what):
    assert type(a) is type(b), what
    if isinstance(a, tuple):
        assert len(a) == len(b), what
        for k, (p, q) in enumerate(zip(a, b)):
            _rows_equal(p, q, (what, k))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), what
    else:
        assert a == b, what


@pytest.mark.parametrize("layout", ["concat", "pad", "bestfit", "windows"])
def test_range_labeled_rows_equal_the_two_steps(wtok, chat, layout):
    text, doffs = chat
    ranges = _chat_ranges(text, doffs, True)
    two = wtok.encode_batch_to_range_labels(text, doffs, ranges, rule="inside")
    kw = dict(layout=layout, bos="<|begin_of_text|>" if layout != "concat" else None, eos="<|end_of_text|>")
    if layout == "windows":
        kw.update(overlap=32, mask_overlap=True)
    want = wtok.ids_to_labeled_rows(two.ids, two.labels, two.tok_offsets, 256, **kw)
    got = wtok.encode_batch_to_range_labeled_rows(text, doffs, ranges, 256, rule="inside", **kw)
    _rows_equal(got, want, layout)
    on = got.labels != -100
    assert np.array_equal(got.labels[on], got.rows.ids[on])
    # every trained id is in the rows once; PAD keeps the first 256 - BOS - EOS ids of a document only
    o = two.tok_offsets
    kept = sum(int((two.labels[o[d]:min(o[d + 1], o[d] + 254)] != -100).sum()) for d in range(len(o) - 1))
    assert two.counts[0] > 5000 and on.sum() >= (kept if layout == "pad" else two.counts[0]) and kept > 500


def test_character_ranges_on_multi_byte_text(wtok):
    rng = np.random.default_rng(12)
    words = ["Grüße", "naïve", "中文字符", "\U0001F600\U0001F680", "plain", "Ελληνικά", "é", "12", "x"]
    docs = ["", "é"] + [" ".join(words[i] for i in rng.integers(0, len(words), n)) for n in (3, 40, 400, 2500)]
    text, offs = H.pack_docs([d.encode("utf-8") for d in docs])
    chars, want = [], []
    for d in docs:
        cuts = np.sort(rng.integers(0, len(d) + 1, 2 * min(len(d), 20))).reshape(-1, 2).tolist()
        if d:
            cuts.append((cuts[-1][1], len(d)))
        chars.append(cuts)
        want.append([(len(d[:a].encode("utf-8")), len(d[:b].encode("utf-8"))) for a, b in cuts])
    for rule in rt.RULES:
        by_chars = wtok.encode_batch_to_range_labels(text, offs, chars, rule=rule, unit="chars", mask=True, trained_offsets=True)
        by_bytes = wtok.encode_batch_to_range_labels(text, offs, want, rule=rule, mask=True, trained_offsets=True)
        _rows_equal(tuple(by_chars), tuple(by_bytes), rule)
        assert by_chars.counts[0] > 300
    got = wtok.encode_batch_to_range_labeled_rows(text, offs, chars, 128, layout="bestfit", unit="chars", pad=0)
    _rows_equal(got, wtok.ids_to_labeled_rows(by_bytes.ids, wtok.encode_batch_to_range_labels(text, offs, want).labels, by_bytes.tok_offsets,
                                              128, layout="bestfit", pad=0), "rows")
    with pytest.raises(ValueError):
        wtok.ids_to_range_labels(by_bytes.ids, by_bytes.tok_offsets, want, rule="sideways")
