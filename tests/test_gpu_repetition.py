"""Duplicate lines and paragraphs on the GPU (td_repetition_device, td_repetition, Tokenizer.repetition_stats) against the truth
(tests/repetition_truth.py).  stats and totals must be EQUAL.  In the device buffer the text lies between guard bytes inside the
allocation: non-LF bytes in front of it, and behind it two LFs and a copy of the text's first line: a kernel that looked outside the
text would extend a line or find a duplicate, and the comparison would show it.  The outputs are filled with 0xFF before every call.
No case here makes the device fault: every error is one the library reports by a status code."""
import numpy as np
import pytest

import helpers as H
import repetition_truth as rt

pytestmark = pytest.mark.gpu

ALL = rt.LINES | rt.PARAS
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
    return {name: (text, offs, {g: rt.truth(text, offs, g) for g in (rt.LINES, rt.PARAS, ALL)}) for name, (text, offs) in rt.cases().items()}


def run(tok, text, offs, groups=ALL, shift=0, max_units=None):
    """-> ((stats, totals), (status, position), everything else of both output buffers still 0xFF).  max_units None: a bound from the
    text's length (a line and a paragraph take a byte each and a delimiter between two); 0: the library's default."""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    text, n_docs = bytes(text), len(offs) - 1
    first = ([u for u in text.split(b"\n") if u] + [b"z"])[0]
    raw = np.frombuffer(b"x" * (16 + shift) + text + b"\n\n" + first + b"\n", dtype=np.uint8)
    with torch.cuda.stream(stream):
        d_raw = torch.from_numpy(raw.copy()).to(dev)
        d_offs = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).to(dev)
        d_stats = torch.full(((n_docs + SLACK) * rt.COLS,), FF, dtype=torch.int64, device=dev)
        d_tot = torch.full((rt.COLS + SLACK,), FF, dtype=torch.int64, device=dev)
    assert d_raw.data_ptr() % 16 == 0
    s = stream.cuda_stream
    max_units = len(text) + 64 if max_units is None else max_units
    tok.repetition_device(d_raw.data_ptr() + 16 + shift, len(text), d_offs.data_ptr(), n_docs, groups, max_units, d_stats.data_ptr(), d_tot.data_ptr(), s)
    st = tok.device_status_pos(s)
    stream.synchronize()
    stats, tot = d_stats.cpu().numpy(), d_tot.cpu().numpy()
    rest = bool((stats[n_docs * rt.COLS:] == FF).all() and (tot[rt.COLS:] == FF).all())
    return (stats[:n_docs * rt.COLS].reshape(n_docs, rt.COLS), tot[:rt.COLS]), st, rest


def same(got, want, what):
    bad = np.argwhere(got[0] != want[0])
    assert len(bad) == 0, (what, "stats", bad[:6].tolist(), got[0][bad[0][0]].tolist(), want[0][bad[0][0]].tolist())
    assert np.array_equal(got[1], want[1]), (what, "totals", got[1].tolist(), want[1].tolist())


@pytest.mark.parametrize("groups", (rt.LINES, rt.PARAS, ALL))
@pytest.mark.parametrize("shift", (0, 1, 15))
def test_device_equals_truth(tok, cases, shift, groups):
    for name, (text, offs, want) in cases.items():
        got, st, rest = run(tok, text, offs, groups, shift, max_units=0 if len(text) < 4096 else None)
        assert st[0] == 0 and rest, (name, st)
        same(got, want[groups], (name, shift, groups))
    assert cases["Thue-Morse and its complement"][2][ALL][0][0, 3] == 0
    assert cases["Thue-Morse, its complement and a copy"][2][ALL][0][0, 3] == 1
    assert cases["the two copies in two documents"][2][ALL][1][3] == 0 and cases["a line of three tiles, twice"][2][ALL][1][3] == 1


def test_capacity_and_bad_arguments(tok, cases):
    from tokendagger_amd import capi
    text, offs, want = cases["many documents a tile, many tiles"]
    need = int(want[ALL][1][0] + want[ALL][1][6])
    assert need > 1000
    got, st, rest = run(tok, text, offs, ALL, 3, max_units=need - 1)
    assert st == (capi.TD_E_CAPACITY, need) and rest and (got[0] == FF).all() and (got[1] == FF).all()
    got, st, rest = run(tok, text, offs, ALL, 3, max_units=need)
    assert st[0] == 0 and rest
    same(got, want[ALL], "the exact need")
    bad = offs.copy()
    bad[5] = bad[6] + 1
    got, st, rest = run(tok, text, bad, ALL)
    assert st == (capi.TD_E_INVALID, 5) and rest and (got[0] == FF).all() and (got[1] == FF).all()
    for groups in (0, 4, -1):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            run(tok, text, offs, groups)
        assert e.value.code == capi.TD_E_INVALID


def test_repeats_on_a_poisoned_workspace(tok, cases):
    from tokendagger_amd import capi
    text, offs, want = cases["many documents a tile, many tiles"]
    tok.set_option(capi.TD_OPT_WS_FILL, 0xA5)
    try:
        clone = tok.clone()
    finally:
        tok.set_option(capi.TD_OPT_WS_FILL, -1)
    try:
        for k in range(3):
            got, st, rest = run(clone, text, offs, ALL, 7)
            assert st[0] == 0 and rest
            same(got, want[ALL], ("poisoned", k))
    finally:
        clone.close()


def test_host_buffer_and_python_paths(tok, cases):
    import tokendagger as tiktoken
    text, offs, want = cases["many documents a tile, many tiles"]
    same(tok.repetition(text, offs), want[ALL], "td_repetition")
    text, offs = rt.docs(b"ab\n" * 3000)  # (more units than the default max_units: the second round)
    same(tok.repetition(text, offs), rt.truth(text, offs), "td_repetition, retried")
    text, offs, want = cases["a paragraph behind different LF runs"]
    pat, mr, special = H.llama4()
    tk = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    r = tk.repetition_stats(text, offs)
    same((r.stats, r.totals), want[ALL], "Tokenizer.repetition_stats")
    assert r.dup_para_fraction[0] == 0.5 and r.dup_line_fraction[0] == 5 / 8 and r.dup_line_char_fraction[0] == 8 / 12
    assert r.dup_para_char_fraction[0] == 8 / 16
    assert tk.repetition_stats(b"\n", np.asarray([0, 1], dtype=np.int64), groups="lines").dup_line_fraction[0] == 0.0
    with pytest.raises(ValueError):
        tk.repetition_stats(text, offs, groups="some")
