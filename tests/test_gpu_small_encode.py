"""td_small_encode — the ONE kernel behind every single-string call and every host batch of at most 4 KiB and 1024 documents — against
the compiled reference in every pattern family: PCRE2 running the very pattern string, CoreBPE::encode / encode_ordinary (the
reference's src/tiktoken/tiktoken.cpp:169-234 and 156-167).  Ids and document offsets bit for bit.  (Documents that are not well-formed
UTF-8 — cut inside a character, a stray continuation byte — are undefined in the reference, which runs PCRE2 with NO_UTF_CHECK; their
truth is this package's restatement, small_inputs.truth_ids.)

Every "answered by the kernel" / "handed back" below is an assertion on TD_INFO_SMALL_ENCODES / TD_INFO_SMALL_ENCODE_HANDBACKS around the
call: none of these tests passes because the general path answered instead.  The inputs are built by tests/small_inputs.py; the counts
and sizes they promise are checked without a GPU in tests/test_small_inputs_model.py."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import helpers as H
import small_inputs as S
from oracle import ref
from tokendagger_amd import capi

pytestmark = pytest.mark.gpu

ANSWERED, HANDED_BACK, NOT_ASKED = (1, 0), (0, 1), (0, 0)


def _counters(tok):
    return tok.info(capi.TD_INFO_SMALL_ENCODES), tok.info(capi.TD_INFO_SMALL_ENCODE_HANDBACKS)


def _batch(tok, text: bytes, offs, expect, mode: int = 0, capacity: int | None = None):
    """One td_encode_batch call (capacity large enough that the binding never calls twice) -> (ids, offsets); `expect`: by how much
    (answered, handed back) move."""
    before = _counters(tok)
    ids, out = tok.encode_batch(text, offs, mode=mode, capacity=len(text) + 16 if capacity is None else capacity)
    after = _counters(tok)
    assert (after[0] - before[0], after[1] - before[1]) == expect, (text[:40], len(text), len(offs) - 1, "answered / handed back moved by",
                                                                   (after[0] - before[0], after[1] - before[1]), "expected", expect)
    return ids, out


def _one(tok, doc: bytes, expect, mode: int = 0):
    return _batch(tok, doc, np.asarray([0, len(doc)], dtype=np.int64), expect, mode)[0]


def _expect(name: str, doc: bytes):
    if len(doc) > S.SMALL_MAX_BYTES:
        return NOT_ASKED
    return HANDED_BACK if S.hands_back(name, doc) else ANSWERED


def _expect_batch(name: str, text: bytes, offs):
    if len(text) > S.SMALL_MAX_BYTES or len(offs) - 1 > S.SMALL_MAX_DOCS:
        return NOT_ASKED
    return HANDED_BACK if any(S.hands_back(name, text[offs[d]:offs[d + 1]]) for d in range(len(offs) - 1)) else ANSWERED


def _make(name: str, resident: bool = False):
    assert ref.available(), "oracle/_ref/libtdref.so is missing: build it where a checkout of the reference exists (oracle/build_ref.sh)"
    _, mr, special = H.llama4()
    old = os.environ.get("TD_SMALL_RESIDENT")
    if resident:
        os.environ["TD_SMALL_RESIDENT"] = "1"
    try:
        return capi.HipTokenizer(S.SPELLINGS[name], mr, special, device=0)
    finally:
        if resident:
            if old is None:
                del os.environ["TD_SMALL_RESIDENT"]
            else:
                os.environ["TD_SMALL_RESIDENT"] = old


@pytest.fixture(scope="module", params=list(S.SPELLINGS))
def fam(request):
    """(name of the spelling, its handle): one handle per spelling for the whole module."""
    tok = _make(request.param)
    assert _counters(tok) == (0, 0)
    yield request.param, tok
    tok.close()


@pytest.fixture(scope="module")
def llama():
    tok = _make("llama4")
    yield tok
    tok.close()


def test_counters_start_at_zero_and_a_clone_s_too(llama):
    before = _counters(llama)
    _one(llama, b"Hello, world!", ANSWERED)
    assert _counters(llama) == (before[0] + 1, before[1])
    c = llama.clone()
    try:
        assert _counters(c) == (0, 0) and (c.info(capi.TD_INFO_SMALL_DECODES), c.info(capi.TD_INFO_SMALL_DECODE_HANDBACKS)) == (0, 0)
        _one(c, b"a" * 1025, HANDED_BACK)
        assert _counters(c) == (0, 1) and _counters(llama) == (before[0] + 1, before[1])
    finally:
        c.close()
    llama.set_option(capi.TD_OPT_SMALL_PATH, 0)
    _one(llama, b"Hello, world!", NOT_ASKED)
    llama.set_option(capi.TD_OPT_SMALL_PATH, 1)
    assert llama.encode(b"").tolist() == [] and _counters(llama) == (before[0] + 1, before[1])  # (an empty call wakes no kernel)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
def test_documents_alone(fam):
    name, tok = fam
    handed = 0
    for k, doc in enumerate(S.documents()):
        e = _expect(name, doc)
        handed += e == HANDED_BACK
        assert np.array_equal(_one(tok, doc, e), S.truth_ids(name, doc)), (name, doc[:60])
        if k % 5 == 0:
            assert np.array_equal(_one(tok, doc, e, mode=1), S.truth_ids(name, doc, mode=1)), (name, doc[:60], "encode_ordinary")
    assert handed >= 4, "the documents with a piece above 1024 bytes"


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
def _borders(name, tok):
    for doc in S.border_inputs():
        assert np.array_equal(_one(tok, doc, ANSWERED), S.truth_ids(name, doc)), (name, doc)


def test_every_lane_border(fam):
    _borders(*fam)


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
def test_document_cuts_inside_a_small_batch(fam):
    name, tok = fam
    for what, (text, offs, answered) in S.cut_batches().items():
        e = _expect_batch(name, text, offs)
        assert (e == ANSWERED) == answered and (answered or e == NOT_ASKED), what
        ids, out = _batch(tok, text, offs, e)
        want, wo = S.truth_batch(name, text, offs)
        assert np.array_equal(out, wo) and np.array_equal(ids, want), (name, what)
    for text, offs in list(S.random_cuts()) + [S.whole(d) for d in S.eos_batches()]:
        ids, out = _batch(tok, text, offs, ANSWERED)
        want, wo = S.truth_batch(name, text, offs)
        assert np.array_equal(out, wo) and np.array_equal(ids, want), (name, len(text), len(offs))


@pytest.mark.parametrize("name", S.EOS_SPELLINGS)
def test_the_end_of_a_document_is_the_end_of_the_subject(name):
    """`\\s++$`: a whitespace tail at a document end inside a batch is one piece, whatever the next document starts with."""
    tok = _make(name)
    try:
        for docs in S.eos_batches():
            text, offs = S.whole(docs)
            ids, out = _batch(tok, text, offs, ANSWERED)
            want, wo = S.truth_batch(name, text, offs)
            assert np.array_equal(out, wo) and np.array_equal(ids, want), (name, docs[:4])
            _, rt, ro = S.reference(name).encode_batch(np.frombuffer(text, dtype=np.uint8), offs)  # (all well-formed: the reference's batch form)
            assert np.array_equal(out, ro) and np.array_equal(ids, rt)
            for d, doc in enumerate(docs):  # ... and the same documents one by one
                if doc:
                    assert np.array_equal(_one(tok, doc, ANSWERED), ids[out[d]:out[d + 1]]), (name, doc)
                else:
                    assert out[d] == out[d + 1]
    finally:
        tok.close()


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
def test_sizes(fam):
    name, tok = fam
    for text, answered in S.size_texts():
        e = _expect(name, text)
        assert e == (ANSWERED if answered else NOT_ASKED), len(text)
        assert np.array_equal(_one(tok, text, e), S.truth_ids(name, text)), (name, len(text), text[:30])


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------
def _miss_batches(tok):
    for n_short, n_long in S.MISS_COUNTS:
        text = S.miss_text(n_short, n_long)
        assert np.array_equal(_one(tok, text, ANSWERED), S.truth_ids("llama4", text)), (n_short, n_long)


def test_the_miss_merge_s_second_and_third_batch(llama):
    """256 / 257 / 512 / 513 missed pieces of at most 16 bytes, 64 / 65 / 128 / 129 of 17..64 bytes, and both classes interleaved
    (counts checked in test_small_inputs_model.py): a lane per piece, 256 respectively 64 pieces at a time."""
    _miss_batches(llama)


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------
def test_encode_ordinary_on_a_vocabulary_that_is_not_merge_closed():
    """use_fastpath = 0: no piece is looked up, every piece of 2..64 bytes is merged (2048 of them fill the miss list), a longer one
    skips the whole-piece table."""
    toy = S.toy_open_vocab()
    Rt = ref.RefTokenizer(S.SPELLINGS["llama4"], toy, {})
    tok = capi.HipTokenizer(S.SPELLINGS["llama4"], toy, {}, device=0)
    try:
        assert tok.info(capi.TD_INFO_MERGE_CLOSED) == 0
        for text in S.toy_open_inputs():
            assert np.array_equal(_one(tok, text, ANSWERED, mode=1), Rt.encode_ordinary(text)), text[:12]
            assert np.array_equal(_one(tok, text, ANSWERED, mode=0), Rt.encode(text)), text[:12]
        assert _one(tok, S.TOY_LONG_TOKEN, ANSWERED, mode=0).tolist() == [259], "the whole-piece hit of a piece above 64 bytes"
        assert _one(tok, S.TOY_LONG_TOKEN, ANSWERED, mode=1).tolist() == [257, ord("c"), ord("d")] * 20
        assert _one(tok, b"abcd", ANSWERED, mode=0).tolist() == [258] and _one(tok, b"abcd", ANSWERED, mode=1).tolist() == [257, ord("c"), ord("d")]
    finally:
        tok.close()


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------------
def _long_pieces(name, tok):
    _, mr, _ = H.llama4()
    seen = set()
    for mode in (0, 1):
        for text, n in S.long_single_pieces():
            e = ANSWERED if n <= S.LONG_MAX else HANDED_BACK
            seen.add((n, e))
            assert np.array_equal(_one(tok, text, e, mode), S.truth_ids(name, text, mode)), (name, text[:8], n, mode)
        whole = 0
        for text, t in S.long_token_texts():
            ids = _one(tok, text, ANSWERED, mode)
            assert np.array_equal(ids, S.truth_ids(name, text, mode)), (name, t, mode)
            if t in S.reference(name).split_pieces(text):  # the token is a piece: the whole-piece hit (tiktoken.cpp:209-215)
                whole += 1
                assert mr[t] in ids.tolist(), (name, t)
        assert whole > 20
        for what, (text, n_long) in S.long_many().items():
            assert np.array_equal(_one(tok, text, ANSWERED, mode), S.truth_ids(name, text, mode)), (name, what, mode)
    assert {(1024, ANSWERED), (1025, HANDED_BACK), (65, ANSWERED), (64, ANSWERED)} <= seen


def test_long_pieces_inside_the_kernel(fam):
    _long_pieces(*fam)


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------------
def test_errors_and_capacity(llama):
    holes = S.toy_holes_vocab()
    pat = S.SPELLINGS["llama4"]
    Rf = ref.RefTokenizer(pat, S.full_byte_vocab(), {})
    tok = capi.HipTokenizer(pat, holes, {}, device=0)
    try:
        for what, text in S.ERROR_INPUTS.items():
            bad = S.pieces_with_unknown_bytes(Rf, text, holes)
            before = _counters(tok)
            with pytest.raises(capi.TokenDaggerHipError) as e:
                tok.encode_batch(text, np.asarray([0, len(text)], dtype=np.int64), capacity=len(text) + 16)
            assert e.value.code == 4, (what, str(e.value))
            assert _counters(tok) == (before[0] + 1, before[1]), "an error the kernel reports is its answer"
            pos = int(re.search(r"byte offset (\d+)", str(e.value)).group(1))
            assert any(a <= pos < b for a, b in bad), (what, pos, bad)
            ok = b"ab de, fg\n"  # the handle answers the next call
            assert np.array_equal(_one(tok, ok, ANSWERED), Rf.encode(ok))
    finally:
        tok.close()
    text = S.miss_text(257, 0)
    want = S.truth_ids("llama4", text)
    offs = np.asarray([0, len(text)], dtype=np.int64)
    before = _counters(llama)
    with pytest.raises(capi.TokenDaggerHipError) as e:
        llama.encode_batch(text, offs, capacity=len(want) - 1)
    assert e.value.code == capi.TD_E_CAPACITY and str(len(want)) in str(e.value)
    assert _counters(llama) == (before[0] + 1, before[1])
    assert np.array_equal(_batch(llama, text, offs, ANSWERED, capacity=len(want))[0], want)


# ---- 9 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["llama4", "cl100k_current"])
def test_the_resident_form(name):
    """TD_SMALL_RESIDENT=1: the same body behind a mailbox, calls back to back (one kernel answers many)."""
    tok = _make(name, resident=True)
    try:
        _borders(name, tok)
        if name == "llama4":
            _miss_batches(tok)
            _long_pieces(name, tok)
    finally:
        tok.close()
