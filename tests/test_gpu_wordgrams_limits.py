"""td_word_ngrams_device at the limits its design text names: td_rp_prefix with more than one tile a lane (257 and 513 tiles, a word that
crosses a lane's whole chunk), a tile whose table of documents does not fit LDS (runs of empty documents: td_wg_tiles' back-fill of
first_word, td_wg_reset's fill at the text's end), more words on the global path than one sweep of td_wg_insert, td_wg_count and
td_wg_cover, long documents in many lanes' chunks of td_wg_long, the LDS table's size steps, the document blocks of td_wg_short, the
capacity check at scale and repeats on a poisoned workspace; then both passes of td_repetition_scan.h on ONE handle with no host wait
between the calls.  tests/test_limit_cases_model.py proves on the CPU which path each case of wordgrams_truth.limit_cases() and
big_cases() reaches; here every result is compared with the truth, exactly.  run() and same() are test_gpu_wordgrams.py's.
No case here makes the device fault: every error is one the library reports by a status code."""
import numpy as np
import pytest

import chain_cases as cc
from helpers import every_case
import repetition_truth as rt
import wordgrams_truth as wt
from test_gpu_wordgrams import ALL, FF, SLACK, run, same, tok  # noqa: F401

pytestmark = pytest.mark.gpu

STRIDE = "global stride"  # (every document with two words is on the global path already: TD_WG_NO_LDS changes nothing)


@pytest.fixture(scope="module")
def limits():
    """Built once, shared and left unchanged: name -> (text, offsets, {groups: (stats, totals)})."""
    return {name: (text, offs, wt.truths(text, offs)) for name, (text, offs) in wt.limit_cases().items()}


@pytest.fixture(scope="module")
def bigs():
    return {name: (text, offs, wt.truths(text, offs)) for name, (text, offs) in wt.big_cases().items()}


@pytest.mark.parametrize("flags", (0, wt.NO_LDS))
@pytest.mark.parametrize("shift", rt.SHIFTS)
def test_limit_cases_equal_truth(tok, limits, shift, flags):
    def one(name, text, offs, want):
        got, st, rest = run(tok, text, offs, ALL, flags, shift)
        assert st[0] == 0 and rest, (name, st)
        same(got, want[ALL], (name, shift, flags))
    every_case({name: c for name, c in limits.items() if not (name == STRIDE and flags)}, one)


@pytest.mark.parametrize("flags", (0, wt.NO_LDS))
@pytest.mark.parametrize("groups", (wt.TOP, wt.DUP, ALL))
@pytest.mark.parametrize("shift", rt.SHIFTS)
def test_big_cases_equal_truth(tok, bigs, shift, groups, flags):
    def one(name, text, offs, want):
        got, st, rest = run(tok, text, offs, groups, flags, shift)
        assert st[0] == 0 and rest, (name, st)
        same(got, want[groups], (name, shift, groups, flags))
    every_case(bigs, one)


@pytest.mark.parametrize("shift", (0, 1))
def test_capacity_at_scale(tok, bigs, shift):
    """256 tiles, and 257: td_rp_prefix's capacity branch behind two tiles a lane"""
    from tokendagger_amd import capi
    text, offs, want = bigs["big A, cut"]
    need = int(want[ALL][1][0])
    assert need > 100000
    got, st, rest = run(tok, text, offs, ALL, 0, shift, max_words=need - 1)
    assert st == (capi.TD_E_CAPACITY, need) and rest and (got[0] == FF).all() and (got[1] == FF).all()
    got, st, rest = run(tok, text, offs, ALL, 0, shift, max_words=need)
    assert st[0] == 0 and rest
    same(got, want[ALL], "the exact need")


def test_repeats_on_a_poisoned_workspace(tok, limits, bigs):
    from tokendagger_amd import capi
    tok.set_option(capi.TD_OPT_WS_FILL, 0xA5)
    try:
        clone = tok.clone()
    finally:
        tok.set_option(capi.TD_OPT_WS_FILL, -1)
    try:
        for text, offs, want in (bigs["big A, cut"], limits[STRIDE]):
            for k in range(3):
                got, st, rest = run(clone, text, offs, ALL, 0, 1)
                assert st[0] == 0 and rest
                same(got, want[ALL], ("poisoned", len(text), k))
    finally:
        clone.close()


# ---- one handle, two passes, no host wait ----------------------------------------------------------------------------------------------------
class Call:
    """One device call, made completely before anything is launched (tests/test_gpu_chains.py's pattern).  The text lies as in run()
    of the two single-pass files: non-separator bytes in front of it, behind it a separator and a copy of its first units, so that a
    kernel that read past the end would lengthen a unit or find a duplicate.  The outputs are 0xFF, with SLACK rows of 0xFF in front
    of them and behind them that nobody may write.  launch() is the library call and nothing else.  want None: a call that must
    write nothing (dev_offs: the offsets it is given)."""

    def __init__(self, kind, text, offs, want, shift, flags=0, dev_offs=None):
        import torch
        self.kind, self.want, self.flags = kind, want, flags
        self.cols = rt.COLS if kind == "rp" else wt.COLS
        text = bytes(text)
        self.n_bytes, self.n_docs = len(text), len(offs) - 1
        if kind == "rp":
            back = b"\n\n" + ([u for u in text.split(b"\n") if u] + [b"z"])[0] + b"\n"
        else:
            back = b" " + b" ".join((text.split() + [b"z"])[:10]) + b" "
        self.text, self.p_text = cc.up(np.frombuffer(text + back, dtype=np.uint8), np.uint8, front=16 + shift, pad=0x78)
        self.offs, self.p_offs = cc.up(offs if dev_offs is None else dev_offs, np.int64)
        self.stats = torch.full(((self.n_docs + 2 * SLACK) * self.cols,), FF, dtype=torch.int64, device=cc.dev())
        self.tot = torch.full((self.cols + 2 * SLACK,), FF, dtype=torch.int64, device=cc.dev())
        self.p_stats, self.p_tot = self.stats.data_ptr() + 8 * SLACK * self.cols, self.tot.data_ptr() + 8 * SLACK

    def launch(self, tok, s):
        if self.kind == "rp":
            tok.repetition_device(self.p_text, self.n_bytes, self.p_offs, self.n_docs, rt.LINES | rt.PARAS, self.n_bytes + 64, self.p_stats, self.p_tot, s)
        else:
            tok.word_ngrams_device(self.p_text, self.n_bytes, self.p_offs, self.n_docs, ALL, self.flags, self.n_bytes // 2 + self.n_docs + 1,
                                   self.p_stats, self.p_tot, s)

    def check(self, what):
        stats, tot = self.stats.cpu().numpy(), self.tot.cpu().numpy()
        if self.want is None:
            assert (stats == FF).all() and (tot == FF).all(), (what, "written although the call was bad")
            return
        lo, n = SLACK * self.cols, self.n_docs * self.cols
        assert (stats[:lo] == FF).all() and (stats[lo + n:] == FF).all(), (what, "stats written outside its rows")
        assert (tot[:SLACK] == FF).all() and (tot[SLACK + self.cols:] == FF).all(), (what, "totals written outside its columns")
        same((stats[lo:lo + n].reshape(self.n_docs, self.cols), tot[SLACK:SLACK + self.cols]), self.want, what)


@pytest.fixture(scope="module")
def rp_truths():
    L, B = rt.limit_cases(), rt.big_cases()
    return {name: (*c[name], rt.truth(*c[name])) for c, name in ((B, "big A, cut"), (L, "4350 empty documents inside a line"))}


def _chain(limits, bigs, rp_truths, bad=False):
    """repetition(big A), word_ngrams(long list), repetition(empty runs), word_ngrams(big A); bad: the second call's offsets decrease"""
    text, offs, want = limits["long list"]
    second = Call("wg", text, offs, want[ALL], 3)
    if bad:
        second = Call("wg", text, offs, None, 3, dev_offs=cc.swapped(offs, 7))
    a, e = rp_truths["big A, cut"], rp_truths["4350 empty documents inside a line"]
    w = bigs["big A, cut"]
    return [Call("rp", a[0], a[1], a[2], 1), second, Call("rp", e[0], e[1], e[2], 15), Call("wg", w[0], w[1], w[2][ALL], 1)]


@pytest.mark.parametrize("n_streams", (1, 2))
def test_both_passes_on_one_handle_with_no_host_wait(tok, limits, bigs, rp_truths, n_streams):
    import torch
    from tokendagger_amd import capi
    streams = [torch.cuda.Stream(device=cc.dev()) for _ in range(n_streams)]
    ops = _chain(limits, bigs, rp_truths)
    torch.cuda.synchronize()
    for i, op in enumerate(ops):
        op.launch(tok, streams[i % n_streams].cuda_stream)
    for s in streams[1:]:  # (one stream: the status read at the end is the only wait)
        s.synchronize()
    assert [tok.device_status_pos(s.cuda_stream)[0] for s in streams] == [capi.TD_OK] * n_streams
    for i, op in enumerate(ops):
        op.check(("chain", n_streams, i))


def test_a_chain_keeps_the_first_unread_error(tok, limits, bigs, rp_truths):
    import torch
    from tokendagger_amd import capi
    stream = torch.cuda.Stream(device=cc.dev())
    ops = _chain(limits, bigs, rp_truths, bad=True)
    torch.cuda.synchronize()
    for op in ops:
        op.launch(tok, stream.cuda_stream)
    assert tok.device_status_pos(stream.cuda_stream) == (capi.TD_E_INVALID, 7)
    stream.synchronize()
    for i, op in enumerate(ops):
        op.check(("error chain", i))
    assert tok.device_status_pos(stream.cuda_stream)[0] == capi.TD_OK, "the error was not cleared by the read"
