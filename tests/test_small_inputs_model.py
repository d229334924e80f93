"""What tests/test_gpu_small_encode.py relies on, checked without a GPU: the sizes, the miss counts and the long-piece lengths of
tests/small_inputs.py, from the compiled reference (PCRE2 running the very pattern string) and the vocabulary alone; and, for the four
families the CPU twin knows, the twin's ids on every input against the reference's (CoreBPE::encode, the reference's
src/tiktoken/tiktoken.cpp:169-234) — a scanner bug shared by both device paths shows here first.  Documents that are not well-formed
UTF-8 (cut inside a character) take this package's restatement as truth: the reference leaves them undefined (small_inputs.truth_ids)."""
import numpy as np
import pytest

import helpers as H
import small_inputs as S
from oracle import ref

pytestmark = pytest.mark.skipif(not ref.available(), reason="compiled reference (oracle/_ref) not built")


def _batches():
    out = [(t, o) for t, o, _ in S.cut_batches().values()] + list(S.random_cuts()) + [S.whole(d) for d in S.eos_batches()]
    return out


def test_sizes_stay_inside_the_limits_except_where_meant():
    docs = S.documents()
    assert len(docs) > 1800 and all(docs)
    over = [d for d in docs if len(d) > S.SMALL_MAX_BYTES]
    assert 0 < len(over) < 5, "only a few strings of tests/cases.py exceed the limit"
    assert len(S.PROBES) == 40 and len(set(S.PROBES)) == 40
    assert len(S.border_inputs()) == 3 * 49 * 40 and max(map(len, S.border_inputs())) < 80
    cb = S.cut_batches()
    for name, (text, offs, answered) in cb.items():
        assert len(text) <= S.SMALL_MAX_BYTES and offs[0] == 0 and offs[-1] == len(text) and (np.diff(offs) >= 0).all(), name
        assert (len(offs) - 1 <= S.SMALL_MAX_DOCS) == answered, name
    assert len(cb["every_4_bytes"][1]) - 1 == 1024 and len(cb["every_4_bytes"][0]) == 4096
    assert len(cb["1025_documents"][1]) - 1 == 1025 and len(cb["one_byte_documents"][1]) - 1 == 1024
    t, o = cb["every_4_bytes"][0], cb["every_4_bytes"][1]
    assert sum((t[p] & 0xC0) == 0x80 for p in o[1:-1]) > 50, "cuts inside multi-byte characters"
    e = cb["empty_documents"][1]
    assert e[0] == e[1] == 0 and e[-1] == e[-2] and any(a == b and a % 16 == 0 and a > 0 for a, b in zip(e[1:-2], e[2:-1]))
    for text, offs in S.random_cuts():
        assert 0 < len(text) <= S.SMALL_MAX_BYTES and len(offs) - 1 <= S.SMALL_MAX_DOCS and offs[-1] == len(text) and (np.diff(offs) >= 0).all()
    assert len(S.random_cuts()) == 200 and sum((np.diff(o) == 0).any() for _, o in S.random_cuts()) > 50
    for text, answered in S.size_texts():
        assert (len(text) <= S.SMALL_MAX_BYTES) == answered
    assert sorted({len(t) for t, _ in S.size_texts()}) == sorted(S.SIZES)
    assert S.size_texts()[-2][0].endswith("中".encode()) and S.size_texts()[-1][0].endswith("\U0001F600".encode())
    for t in S.toy_open_inputs():
        assert len(t) <= S.SMALL_MAX_BYTES
    for t, _ in S.long_token_texts():
        assert len(t) <= S.SMALL_MAX_BYTES


def test_miss_counts_hold_exactly():
    _, mr, _ = H.llama4()
    R = S.reference("llama4")
    for n_short, n_long in S.MISS_COUNTS:
        text = S.miss_text(n_short, n_long)
        assert len(text) <= S.SMALL_MAX_BYTES
        assert S.count_misses(R, mr, text) == (n_short, n_long), (n_short, n_long)
        assert S.max_piece(R, text) <= S.SHORT_MAX
        assert all(w in mr for w in S.FILLER_WORDS)
    assert S.MISS_COUNTS[-1][0] >= 300 and S.MISS_COUNTS[-1][1] >= 70
    # the vocabulary that is not merge-closed: under encode_ordinary EVERY piece of 2..64 bytes is merged
    Rt = ref.RefTokenizer(S.SPELLINGS["llama4"], S.toy_open_vocab(), {})
    a, b, c, d, e, f = S.toy_open_inputs()
    assert [len(p) for p in Rt.split_pieces(a)] == [2] * 2048 and len(Rt.split_pieces(c)) == 1 and len(c) == 300
    assert sum(len(p) >= 2 for p in Rt.split_pieces(b)) == 800
    assert Rt.encode(d).tolist() == [258] and Rt.encode_ordinary(d).tolist() == [257, ord("c"), ord("d")]
    assert e == S.TOY_LONG_TOKEN and S.SHORT_MAX < len(e) <= S.LONG_MAX and Rt.split_pieces(e) == [e], "a token above 64 bytes that is a piece"
    assert Rt.encode(e).tolist() == [259] and Rt.encode_ordinary(e).tolist() == [257, ord("c"), ord("d")] * 20
    assert Rt.encode(f).tolist().count(259) == 2 and 259 not in Rt.encode_ordinary(f).tolist()


@pytest.mark.parametrize("name", list(S.SPELLINGS))
def test_long_piece_lengths_are_the_reference_s(name):
    R = S.reference(name)
    for text, want in S.long_single_pieces():
        assert S.max_piece(R, text) == want, (name, text[:8], want)
    assert {w for _, w in S.long_single_pieces()} >= {64, 65, 1023, 1024, 1025}
    for what, (text, n_long) in S.long_many().items():
        lens = [len(p) for p in R.split_pieces(text)]
        assert sum(n > S.SHORT_MAX for n in lens) == n_long and max(lens) <= S.LONG_MAX and len(text) <= S.SMALL_MAX_BYTES, (name, what)
    assert len(S.long_many()["63_of_65"][0]) == 4095


def test_long_tokens_and_error_inputs():
    _, mr, _ = H.llama4()
    toks = S.long_tokens()
    assert len(toks) == 74 and len(toks[0]) == 65 and len(toks[-1]) == 113
    R = S.reference("llama4")
    whole = sum(t in R.split_pieces(text) for text, t in S.long_token_texts())
    assert whole > 20, "some long tokens stand as one piece: the whole-piece hit of the long phase"
    for text, t in S.long_token_texts():
        if t in R.split_pieces(text):
            assert mr[t] in R.encode(text).tolist()
    Rf = ref.RefTokenizer(S.SPELLINGS["llama4"], S.full_byte_vocab(), {})
    known = S.toy_holes_vocab()
    for what, text in S.ERROR_INPUTS.items():
        bad = S.pieces_with_unknown_bytes(Rf, text, known)
        assert len(bad) == (2 if what == "two_unknown_bytes" else 1), what
        if what in S.ERROR_PIECE_LEN:
            assert bad[0][1] - bad[0][0] == S.ERROR_PIECE_LEN[what], what


@pytest.mark.parametrize("name", list(S.TWINS))
def test_cpu_twin_gives_the_reference_s_ids_on_every_input(name):
    R, tw = S.reference(name), S.TWINS[name]()
    singles = list(S.documents()) + list(S.border_inputs()) + [t for t, _ in S.size_texts()] + [t for t, _ in S.long_single_pieces()]
    singles += [t for t, _ in S.long_token_texts()] + [t for t, _ in S.long_many().values()]
    singles += [S.miss_text(a, b) for a, b in S.MISS_COUNTS]
    for k, doc in enumerate(singles):
        want = S.truth_ids(name, doc)
        assert np.array_equal(tw.encode_batch(doc)[0], want), (name, doc[:60])
        if k % 5 == 0 and S.well_formed(doc):
            assert np.array_equal(R.encode_ordinary(doc), want), (name, doc[:60])  # (the Llama-4 vocabulary is merge-closed)
    for text, offs in _batches():
        et, eo = S.truth_batch(name, text, offs)
        if S.well_formed(text) and all(S.well_formed(text[offs[d]:offs[d + 1]]) for d in range(len(offs) - 1)):
            _, rt, ro = R.encode_batch(np.frombuffer(text, dtype=np.uint8), offs)  # (the reference's own batch form, where it is defined)
            assert np.array_equal(ro, eo) and np.array_equal(rt, et)
        gt, go = tw.encode_batch(text, offs)
        assert np.array_equal(go, eo) and np.array_equal(gt, et), (name, len(text), len(offs))
