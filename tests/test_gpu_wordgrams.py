"""Word n-gram repetition on the GPU (td_word_ngrams_device, td_word_ngrams, Tokenizer.word_ngram_stats) against the truth
(tests/wordgrams_truth.py).  stats and totals must be EQUAL.  In the device buffer the text lies between guard bytes inside the
allocation: non-space bytes in front of it, and behind it a space and a copy of the text's first ten words: a kernel that looked outside
the text would extend a word or find a duplicate, and the comparison would show it.  The outputs are filled with 0xFF before every call.
No case here makes the device fault: every error is one the library reports by a status code."""
import numpy as np
import pytest

import helpers as H
import wordgrams_truth as wt

pytestmark = pytest.mark.gpu

ALL = wt.TOP | wt.DUP
FF = -1  # int64 of 0xFF bytes
SLACK = 3


@pytest.fixture(scope="module")
def tok():
    from tokendagger_amd import capi
    pat, mr, special = H.llama4()
    t = capi.HipTokenizer(pat, mr, special, device=0)
    yield t
    t.close()


@pytest.fixture(scope="module")
def cases():
    """Built once, shared and left unchanged: name -> (text, offsets, {groups: (stats, totals)})."""
    return {name: (text, offs, {g: wt.truth(text, offs, g) for g in (wt.TOP, wt.DUP, ALL)}) for name, (text, offs) in wt.cases().items()}


def run(tok, text, offs, groups=ALL, flags=0, shift=0, max_words=None):
    """-> ((stats, totals), (status, position), everything else of both output buffers still 0xFF).  max_words None: the bound from the
    text's length (a word takes two bytes with its separator); 0: the library's default."""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    text, n_docs = bytes(text), len(offs) - 1
    raw = np.frombuffer(b"x" * (16 + shift) + text + b" " + b" ".join((text.split() + [b"z"])[:10]) + b" ", dtype=np.uint8)
    with torch.cuda.stream(stream):
        d_raw = torch.from_numpy(raw.copy()).to(dev)
        d_offs = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).to(dev)
        d_stats = torch.full(((n_docs + SLACK) * wt.COLS,), FF, dtype=torch.int64, device=dev)
        d_tot = torch.full((wt.COLS + SLACK,), FF, dtype=torch.int64, device=dev)
    assert d_raw.data_ptr() % 16 == 0
    s = stream.cuda_stream
    max_words = len(text) // 2 + n_docs + 1 if max_words is None else max_words
    tok.word_ngrams_device(d_raw.data_ptr() + 16 + shift, len(text), d_offs.data_ptr(), n_docs, groups, flags, max_words, d_stats.data_ptr(),
                           d_tot.data_ptr(), s)
    st = tok.device_status_pos(s)
    stream.synchronize()
    stats, tot = d_stats.cpu().numpy(), d_tot.cpu().numpy()
    rest = bool((stats[n_docs * wt.COLS:] == FF).all() and (tot[wt.COLS:] == FF).all())
    return (stats[:n_docs * wt.COLS].reshape(n_docs, wt.COLS), tot[:wt.COLS]), st, rest


def same(got, want, what):
    bad = np.argwhere(got[0] != want[0])
    assert len(bad) == 0, (what, "stats", bad[:6].tolist(), got[0][bad[0][0]].tolist(), want[0][bad[0][0]].tolist())
    assert np.array_equal(got[1], want[1]), (what, "totals", got[1].tolist(), want[1].tolist())


@pytest.mark.parametrize("flags", (0, wt.NO_LDS))
@pytest.mark.parametrize("groups", (wt.TOP, wt.DUP, ALL))
@pytest.mark.parametrize("shift", (0, 1, 15))
def test_device_equals_truth(tok, cases, shift, groups, flags):
    for name, (text, offs, want) in cases.items():
        got, st, rest = run(tok, text, offs, groups, flags, shift, max_words=0 if len(text) < 4096 else None)
        assert st[0] == 0 and rest, (name, st)
        same(got, want[groups], (name, shift, groups, flags))
    assert cases["Thue-Morse and its complement"][2][ALL][0][0, 3] == 1
    assert cases["Thue-Morse, its complement and a copy"][2][ALL][0][0, 3] == 2
    assert cases["a 10-gram in two documents and in one"][2][ALL][0][:, 14].tolist() == [0, 0, 42]
    assert cases[f"a document of {wt.LDS_WORDS + 1} words"][2][ALL][0][0, 14] > 0


def test_capacity_and_bad_arguments(tok, cases):
    from tokendagger_amd import capi
    text, offs, want = cases["many documents a tile, many tiles"]
    need = int(want[ALL][1][0])
    assert need > 1000
    got, st, rest = run(tok, text, offs, ALL, 0, 3, max_words=need - 1)
    assert st == (capi.TD_E_CAPACITY, need) and rest and (got[0] == FF).all() and (got[1] == FF).all()
    got, st, rest = run(tok, text, offs, ALL, 0, 3, max_words=need)
    assert st[0] == 0 and rest
    same(got, want[ALL], "the exact need")
    bad = offs.copy()
    bad[5] = bad[6] + 1
    got, st, rest = run(tok, text, bad, ALL)
    assert st == (capi.TD_E_INVALID, 5) and rest and (got[0] == FF).all() and (got[1] == FF).all()
    for groups, flags in ((0, 0), (4, 0), (-1, 0), (ALL, 2), (ALL, -1)):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            run(tok, text, offs, groups, flags)
        assert e.value.code == capi.TD_E_INVALID


@pytest.mark.parametrize("flags", (0, wt.NO_LDS))
def test_repeats_on_a_poisoned_workspace(tok, cases, flags):
    from tokendagger_amd import capi
    text, offs, want = cases["many documents a tile, many tiles"]
    tok.set_option(capi.TD_OPT_WS_FILL, 0xA5)
    try:
        clone = tok.clone()
    finally:
        tok.set_option(capi.TD_OPT_WS_FILL, -1)
    try:
        for k in range(3):
            got, st, rest = run(clone, text, offs, ALL, flags, 7)
            assert st[0] == 0 and rest
            same(got, want[ALL], ("poisoned", k))
    finally:
        clone.close()


def test_host_buffer_and_python_paths(tok, cases):
    import tokendagger as tiktoken
    text, offs, want = cases["many documents a tile, many tiles"]
    same(tok.word_ngrams(text, offs), want[ALL], "td_word_ngrams")
    text, offs = wt.docs(b"a " * 3000)  # (more words than the default max_words: the second round)
    same(tok.word_ngrams(text, offs), wt.truth(text, offs), "td_word_ngrams, retried")
    text, offs, want = cases["the rule's examples"]
    pat, mr, special = H.llama4()
    tk = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    r = tk.word_ngram_stats(text, offs)
    same((r.stats, r.totals), want[ALL], "Tokenizer.word_ngram_stats")
    assert r.top_fraction(2)[0] == 3 * (2 + 1) / 12 and r.top_fraction(2, joined=False)[0] == 3 * 2 / 12 and r.top_fraction(3)[1] == 0.0
    text, offs, want = cases["a 5-gram twice"]
    r = tk.word_ngram_stats(text, offs, groups="dup")
    assert r.dup_fraction(5).tolist() == [10 / 13, 1.0, 1.0, 15 / 18] and (r.top2_count == 0).all()
    with pytest.raises(ValueError):
        tk.word_ngram_stats(text, offs, groups="some")
