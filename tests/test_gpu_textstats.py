"""Per-document text statistics on the GPU (td_text_stats_device, td_text_stats, td_encode_batch_text_stats, the Python methods) against
the truth (tests/textstats_truth.py).  stats and totals must be EQUAL.  In the device buffer the text lies between guard bytes inside the
allocation: a letter and `E2 80` in front of it, `A6 . .` and a LF behind it: a kernel that looked outside the text would complete an
ellipsis, extend a word or end a line, and the comparison would show it.  The outputs are filled with 0xFF before every call.  No case
here makes the device fault: every error is one the library reports by a status code."""
import numpy as np
import pytest

import helpers as H
import textstats_truth as tt

pytestmark = pytest.mark.gpu

ALL = tt.LOCAL | tt.RUNS
FF = -1  # int64 of 0xFF bytes


@pytest.fixture(scope="module")
def tok():
    from tokendagger_amd import capi
    pat, mr, special = H.llama4()
    t = capi.HipTokenizer(pat, mr, special, device=0)
    yield t
    t.close()


@pytest.fixture(scope="module")
def side():
    import torch
    return torch.cuda.Stream(device=torch.device("cuda", 0))


@pytest.fixture(scope="module")
def cases():
    """Built once, shared and left unchanged: name -> (text, offsets, (stats, totals))."""
    return {name: (text, offs, tt.truth(text, offs)) for name, (text, offs) in tt.limit_cases(tt.TILE).items()}


@pytest.fixture(scope="module")
def big():
    text, offs = tt.big_case()
    one = np.asarray([0, len(text)], dtype=np.int64)
    return text, offs, tt.truth(text, offs), one, tt.truth(text, one)


def only(want, groups):
    stats, totals = want[0].copy(), want[1].copy()
    drop = [c for c in range(tt.COLS) if c not in ((tt.LOCAL_COLS if groups & tt.LOCAL else []) + (tt.RUNS_COLS if groups & tt.RUNS else []))]
    stats[:, drop] = 0
    totals[drop] = 0
    return stats, totals


class Resident:
    """A text and its offsets on the device, the text `shift` bytes off the 16-byte grid between its guard bytes."""

    def __init__(self, text, offs, stream, shift=0, n_bytes=None):
        import torch
        dev = torch.device("cuda", 0)
        text = np.frombuffer(bytes(text), dtype=np.uint8)
        self.offs = np.ascontiguousarray(offs, dtype=np.int64)
        self.n_docs, self.n = len(self.offs) - 1, len(text) if n_bytes is None else n_bytes
        front = np.full(16 + shift, 0x61, np.uint8)
        front[-2:] = (0xE2, 0x80)
        back = np.frombuffer(b"\xa6..\n" + b"a" * 12, dtype=np.uint8)
        self.stream = stream
        with torch.cuda.stream(stream):
            self.raw = torch.from_numpy(np.concatenate([front, text, back])).to(dev)
            self.d_offs = torch.from_numpy(self.offs).to(dev)
        self.ptr = self.raw.data_ptr() + 16 + shift
        assert self.raw.data_ptr() % 16 == 0

    def run(self, tok, groups=ALL, totals=True, slack=3, stream=None):
        """-> ((stats, totals), slack untouched, (status, position), the raw stats buffer)"""
        import torch
        dev = torch.device("cuda", 0)
        stream = stream or self.stream
        with torch.cuda.stream(stream):
            d_stats = torch.full(((self.n_docs + slack) * tt.COLS,), FF, dtype=torch.int64, device=dev)
            d_tot = torch.full((tt.COLS + slack,), FF, dtype=torch.int64, device=dev)
        s = stream.cuda_stream
        tok.text_stats_device(self.ptr, self.n, self.d_offs.data_ptr(), self.n_docs, groups, d_stats.data_ptr(), d_tot.data_ptr() if totals else 0, s)
        st = tok.device_status_pos(s)
        stream.synchronize()
        stats, tot = d_stats.cpu().numpy(), d_tot.cpu().numpy()
        ok = bool((stats[self.n_docs * tt.COLS:] == FF).all() and (tot[tt.COLS:] == FF).all())
        return (stats[:self.n_docs * tt.COLS].reshape(self.n_docs, tt.COLS), tot[:tt.COLS]), ok, st, stats


def same(got, want, what):
    bad = np.argwhere(got[0] != want[0])
    assert len(bad) == 0, (what, "stats", bad[:6].tolist(), got[0][bad[0][0]].tolist(), want[0][bad[0][0]].tolist())
    assert np.array_equal(got[1], want[1]), (what, "totals", got[1].tolist(), want[1].tolist())


def test_lengths_lookback_and_clipping_cases(tok, side, cases):
    """Texts of 0, 1, 15, 16, 17, 4095, 4096, 4097 bytes and three tiles, as one document and cut at random; the cross-tile look-back
    cases (a word of three tiles, a line of 2.5 tiles behind 5000 spaces, three dots astride a window and a tile seam, a bullet behind 4100
    spaces, a final line with no LF, only LFs); clipping at document starts (nothing leaks, 40 documents in a window, a boundary at every
    byte of characters, runs of 10 000 empty documents at the start, in the middle and at the end)."""
    from tokendagger_amd import capi
    assert len(cases) > 50
    for name, (text, offs, want) in cases.items():
        n_bytes = 300 if name == "bytes behind the last document" else None
        got, ok, st, _ = Resident(text, offs, side, n_bytes=n_bytes).run(tok)
        assert st[0] == capi.TD_OK and ok, (name, st)
        same(got, want, name)
    s = cases["nothing leaks, at a tile seam"][2][0]
    assert s[1, tt.WORDS_ALPHA] == 0 and s[1, tt.END_TERMINAL] == 0


@pytest.mark.parametrize("shift", range(1, 16))
def test_text_off_the_16_byte_grid(tok, side, cases, shift):
    names = [n for n in cases if n.startswith(("length 1,", "length 15,", "length 16,", "length 17,", "three dots", "nothing leaks"))] + [
        f"length {3 * tt.TILE}, documents", "forty documents inside one window", "a long line, spaces, LF", "a bullet behind spaces",
        "a word of three tiles, its letter first", "runs of empty documents", f"a boundary at byte {shift} of characters", "no documents"]
    for name in names:
        text, offs, want = cases[name]
        groups = ALL if (shift + len(name)) % 3 else tt.RUNS
        got, ok, st, _ = Resident(text, offs, side, shift=shift).run(tok, groups)
        assert st[0] == 0 and ok, (name, st)
        same(got, only(want, groups), (name, shift, groups))


def test_the_big_text(tok, side, big):
    """About 1.2 MiB: 300 tiles (two sweeps of the prefix maximum), documents of every size, then the same text as ONE document."""
    text, offs, want, one, want1 = big
    for shift in (0, 11):
        got, ok, st, _ = Resident(text, offs, side, shift=shift).run(tok)
        assert st[0] == 0 and ok
        same(got, want, ("big", shift))
    got, ok, st, _ = Resident(text, one, side, shift=5).run(tok)
    assert st[0] == 0 and ok
    same(got, want1, "one document")


def test_groups(tok, side, cases, big):
    from tokendagger_amd import capi
    picked = [(n, cases[n]) for n in ("length 4097, documents", "three dots astride the seam +1", "forty documents inside one window")]
    picked.append(("big", (big[0], big[1], big[2])))
    for name, (text, offs, want) in picked:
        r = Resident(text, offs, side, shift=3)
        for groups in (tt.LOCAL, tt.RUNS, ALL):
            got, ok, st, _ = r.run(tok, groups)
            assert st[0] == 0 and ok
            same(got, only(want, groups), (name, groups))
            if groups != ALL:
                assert not got[0][:, tt.RUNS_COLS if groups == tt.LOCAL else tt.LOCAL_COLS].any()
        got, ok, st, _ = r.run(tok, ALL, totals=False)  # (d_totals NULL)
        assert st[0] == 0 and ok and (got[1] == FF).all()
        assert np.array_equal(got[0], want[0])
    text, offs, _ = cases["length 17, documents"]
    r = Resident(text, offs, side)
    for groups in (0, 4, 7, -1):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            r.run(tok, groups)
        assert e.value.code == capi.TD_E_INVALID
        with pytest.raises(capi.TokenDaggerHipError) as e:
            tok.text_stats(text, offs, groups)
        assert e.value.code == capi.TD_E_INVALID


def test_bad_offsets_write_nothing(tok, side, cases):
    from tokendagger_amd import capi
    text, offs, want = cases[f"length {3 * tt.TILE}, documents"]
    n_docs = len(offs) - 1
    assert n_docs > 100
    dec = offs.copy()
    dec[40], dec[90] = dec[41] + 1, dec[91] + 5          # documents 40 and 90 end in front of their start
    past = offs.copy()
    past[70:] += 9                                        # the last documents end behind n_bytes
    first = offs.copy()
    first[0] = 1
    where_past = int(np.argmax(past[1:] > len(text)))
    assert where_past >= 69
    for name, o, n_bytes, where in (("decreasing", dec, None, 40), ("past n_bytes", past, len(text), where_past), ("first is not 0", first, None, 0)):
        r = Resident(text, o, side, n_bytes=n_bytes)
        for groups in (tt.LOCAL, ALL):
            got, ok, st, raw = r.run(tok, groups)
            assert st == (capi.TD_E_INVALID, where), (name, st)
            assert (raw == FF).all() and (got[1] == FF).all(), name
    # and the handle goes on
    got, ok, st, _ = Resident(text, offs, side).run(tok)
    assert st[0] == 0
    same(got, want, "after the errors")


def test_repeats_bit_for_bit_on_a_poisoned_workspace(tok, big):
    """The 1.2 MiB case 20 times on one handle whose workspace is filled with 0xA5 at birth and before every call, into 0xFF-filled
    outputs: the same bytes every time, and the truth.  Once more on two td_clone handles on two streams."""
    import torch
    from tokendagger_amd import capi
    text, offs, want = big[0], big[1], big[2]
    tok.set_option(capi.TD_OPT_WS_FILL, 0xA5)
    try:
        clones = [tok.clone() for _ in range(3)]
    finally:
        tok.set_option(capi.TD_OPT_WS_FILL, -1)
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(3)]
    r = Resident(text, offs, streams[0], shift=7)
    filled = clones[0].info(capi.TD_INFO_WS_FILLED_BYTES)
    firsts = None
    for k in range(20):
        got, ok, st, _ = r.run(clones[0])
        assert st[0] == 0 and ok
        if firsts is None:
            same(got, want, "poisoned")
            firsts = (got[0].tobytes(), got[1].tobytes())
        assert (got[0].tobytes(), got[1].tobytes()) == firsts, k
    assert clones[0].info(capi.TD_INFO_WS_FILLED_BYTES) > filled
    streams[0].synchronize()
    # two clones, two streams, launched back to back before either is waited for
    dev = torch.device("cuda", 0)
    outs = []
    for c, s in zip(clones[1:], streams[1:]):
        s.wait_stream(streams[0])
        with torch.cuda.stream(s):
            d_stats = torch.full((r.n_docs * tt.COLS,), FF, dtype=torch.int64, device=dev)
            d_tot = torch.full((tt.COLS,), FF, dtype=torch.int64, device=dev)
        c.text_stats_device(r.ptr, r.n, r.d_offs.data_ptr(), r.n_docs, ALL, d_stats.data_ptr(), d_tot.data_ptr(), s.cuda_stream)
        outs.append((d_stats, d_tot))
    for (d_stats, d_tot), c, s in zip(outs, clones[1:], streams[1:]):
        assert c.device_status_pos(s.cuda_stream)[0] == 0
        s.synchronize()
        assert (d_stats.cpu().numpy().tobytes(), d_tot.cpu().numpy().tobytes()) == firsts
    for c in clones:
        c.close()


def test_a_generic_pattern_handle_gives_the_same(tok, side, cases, big):
    import cases as C
    from tokendagger_amd import capi
    g = capi.HipTokenizer(C.SUPPORTED_GENERIC_PATTERNS[0], {bytes([b]): b for b in range(256)}, {}, device=0)
    try:
        for name, (text, offs, want) in [(n, cases[n]) for n in (f"length {3 * tt.TILE}, documents", "a boundary at byte 3 of characters")] + [
                ("big", (big[0], big[1], big[2]))]:
            got, ok, st, _ = Resident(text, offs, side, shift=2).run(g)
            assert st[0] == 0 and ok
            same(got, want, ("generic", name))
            same(got, Resident(text, offs, side, shift=2).run(tok)[0], ("generic against Llama-4", name))
    finally:
        g.close()


@pytest.fixture(scope="module")
def mixed():
    """64 KiB of mixed-script text in documents"""
    rng = np.random.default_rng(31)
    words = ["the", "Quick", "brown", "fox.", "naïve", "café!", "Ελληνικά", "русский", "текст?", "中文文本。", "日本語", "한국어", "العربية", "x²", "…", "...",
             "#tag", "{a}", "1234", "٣٤", "é", "“quote”", "？", "！", "- item", "• point", "\U0001F600", "A B", "tab\tbed"]
    parts = []
    while sum(map(len, parts)) < 64 * 1024:
        parts.append((words[int(rng.integers(0, len(words)))] + ("\n" if rng.integers(0, 9) == 0 else " ")).encode())
    text = b"".join(parts)[:64 * 1024]
    return text, tt.cut(rng, len(text), 90)


def test_host_and_python_paths(tok, mixed):
    import tokendagger as tiktoken
    text, offs = mixed
    want = tt.truth(text, offs)
    assert want[1][tt.LETTER_OTHER] > 0 and want[1][tt.MARK] > 0 and want[1][tt.END_TERMINAL] > 0 and want[1][tt.START_BULLET] > 0
    same(tok.text_stats(text, offs), want, "td_text_stats")
    for groups in (tt.LOCAL, tt.RUNS):
        same(tok.text_stats(text, offs, groups), only(want, groups), ("td_text_stats", groups))
    ids, toff = tok.encode_batch(np.frombuffer(text, dtype=np.uint8), offs)
    g = tok.encode_batch_text_stats(text, offs)
    assert np.array_equal(g[0], ids) and np.array_equal(g[1], toff)
    same(g[2:], want, "td_encode_batch_text_stats")
    pat, mr, special = H.llama4()
    tk = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    ts = tk.text_stats(text, offs)
    same((ts.stats, ts.totals), want, "Tokenizer.text_stats")
    assert np.array_equal(ts.words, want[0][:, tt.WORDS]) and np.array_equal(ts.lines_end_terminal, want[0][:, tt.END_TERMINAL])
    assert np.array_equal(tk.text_stats(text, offs, groups="local").stats, only(want, tt.LOCAL)[0])
    w = want[0].astype(np.float64)
    has = want[0][:, tt.WORDS] > 0
    assert has.any() and np.allclose(ts.alpha_word_fraction[has], w[has, tt.WORDS_ALPHA] / w[has, tt.WORDS])
    assert np.allclose(ts.symbol_word_ratio[has], (w[has, tt.HASHES] + w[has, tt.ELLIPSES]) / w[has, tt.WORDS])
    assert np.allclose(ts.mean_word_bytes[has], (w[has, tt.BYTES] - w[has, tt.SPACE]) / w[has, tt.WORDS])
    i2, o2, ts2 = tk.encode_batch_to_numpy_with_stats(text, offs)
    e_ids, e_off = tk.encode_batch_to_numpy(text, offs)
    assert np.array_equal(i2, e_ids) and np.array_equal(o2, e_off)
    same((ts2.stats, ts2.totals), want, "encode_batch_to_numpy_with_stats")
    # an empty document: every derived property is 0.0
    e = tk.text_stats(b"ab", np.asarray([0, 0, 2], dtype=np.int64))
    for name in ("mean_word_bytes", "alpha_word_fraction", "terminal_line_fraction", "ellipsis_line_fraction", "bullet_line_fraction",
                 "symbol_word_ratio", "upper_letter_fraction"):
        v = getattr(e, name)
        assert v.dtype == np.float64 and v[0] == 0.0, name
    assert e.mean_word_bytes[1] == 2.0 and e.alpha_word_fraction[1] == 1.0
    with pytest.raises(ValueError):
        tk.text_stats(text, offs, groups="some")


def test_filter_round_trip(mixed):
    """A mask built from TextStats goes to select_docs and brings exactly the ids of the kept documents."""
    import tokendagger as tiktoken
    text, offs = mixed
    pat, mr, special = H.llama4()
    tk = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    ids, toff, ts = tk.encode_batch_to_numpy_with_stats(text, offs)
    keep = (ts.words >= 50) & (ts.alpha_word_fraction >= 0.6) & (ts.symbol_word_ratio <= 0.12) & (ts.line_max_bytes < 1500)
    kept = np.nonzero(keep)[0]
    assert 0 < len(kept) < len(offs) - 1
    r = tk.select_docs(ids, toff, kept)
    want = np.concatenate([ids[toff[d]:toff[d + 1]] for d in kept])
    assert np.array_equal(r[0], want) and np.array_equal(np.diff(r[1]), (toff[1:] - toff[:-1])[kept])
