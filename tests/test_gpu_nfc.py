"""NFC normalisation on the GPU (td_nfc_check_device, td_nfc_device, td_nfc, td_encode_batch_nfc) against td_nfc_host and the fixture
tests/golden/nfc_golden.npz, never against the running interpreter's unicodedata (which only writes inputs).  Text, offsets, flags, changed
and counts must be EQUAL.  No case here makes the device fault: every error is one the library reports by a status code."""
import numpy as np
import pytest

import helpers as H
import nfc_truth as nt

pytestmark = pytest.mark.gpu

FILL = 0x77
TILE = 4096


@pytest.fixture(scope="module")
def tok():
    from tokendagger_amd import capi
    pat, mr, special = H.llama4()
    return capi.HipTokenizer(pat, mr, special, device=0)


@pytest.fixture(scope="module")
def side():
    import torch
    return torch.cuda.Stream(device=torch.device("cuda", 0))


@pytest.fixture(scope="module")
def cases():
    """Built once, shared and left unchanged: name -> (text, offsets, td_nfc_host's answer)."""
    from tokendagger_amd import capi
    return {name: (text, offs, capi.nfc_host(text, offs)) for name, (text, offs) in nt.limit_cases(TILE).items()}


@pytest.fixture(scope="module")
def nfc_golden():
    from pathlib import Path
    with np.load(Path(__file__).resolve().parent / "golden" / "nfc_golden.npz") as z:
        return {k: z[k] for k in z.files}


def same(got, want, what):
    for i, part in enumerate(("text", "offsets", "flags", "changed", "counts")):
        if got[i] is not None:
            assert np.array_equal(got[i], want[i]), (what, part, got[i][:16], want[i][:16])


def device_call(tok, text, offs, stream, shift=0, cap=None, slack=9, n_bytes=None, check_only=False):
    """td_nfc_check_device, then td_nfc_device on a text whose base lies `shift` bytes off the 16-byte grid -> ((out, out_offsets, check
    flags, changed, counts), the check's counts, slack untouched, the two statuses with their positions)."""
    import torch
    dev = torch.device("cuda", 0)
    text, offs = np.ascontiguousarray(text, dtype=np.uint8), np.ascontiguousarray(offs, dtype=np.int64)
    n_docs, n = len(offs) - 1, len(text) if n_bytes is None else n_bytes
    cap = 3 * len(text) if cap is None else cap
    with torch.cuda.stream(stream):
        raw = torch.from_numpy(np.concatenate([np.full(16 + shift, 0xCC, np.uint8), text, np.full(16, 0xCC, np.uint8)])).to(dev)
        d_offs = torch.from_numpy(offs).to(dev)
        d_out = torch.full((cap + slack,), FILL, dtype=torch.uint8, device=dev)
        d_ooff = torch.full((n_docs + 1 + slack,), FILL, dtype=torch.int64, device=dev)
        d_flags = torch.full((n_docs + slack,), FILL, dtype=torch.uint8, device=dev)
        d_changed = torch.full((n_docs + slack,), FILL, dtype=torch.uint8, device=dev)
        d_c1 = torch.full((8,), FILL, dtype=torch.int64, device=dev)
        d_c2 = torch.full((8,), FILL, dtype=torch.int64, device=dev)
    s = stream.cuda_stream
    tok.nfc_check(raw.data_ptr() + 16 + shift, n, d_offs.data_ptr(), n_docs, d_flags.data_ptr(), d_c1.data_ptr(), s)
    st1 = tok.device_status_pos(s)
    st2 = (0, 0)
    if not check_only:
        tok.nfc_device(raw.data_ptr() + 16 + shift, n, d_offs.data_ptr(), n_docs, d_out.data_ptr(), cap, d_ooff.data_ptr(), d_changed.data_ptr(),
                       d_c2.data_ptr(), s)
        st2 = tok.device_status_pos(s)
    stream.synchronize()
    out, ooff, flags, changed = d_out.cpu().numpy(), d_ooff.cpu().numpy(), d_flags.cpu().numpy(), d_changed.cpu().numpy()
    c1, c2 = d_c1.cpu().numpy(), d_c2.cpu().numpy()
    slack_ok = bool((out[cap:] == FILL).all() and (ooff[n_docs + 1:] == FILL).all() and (flags[n_docs:] == FILL).all() and
                    (changed[n_docs:] == FILL).all())
    need = int(c2[0]) if st2[0] == 0 and not check_only else 0
    return (out[:need] if need <= cap else out, ooff[:n_docs + 1], flags[:n_docs], changed[:n_docs], c2), c1, slack_ok, st1, st2, out


def test_limit_cases_through_the_host_form(tok, cases):
    """Every limit case: the dirty segments, the out-of-order and the in-order pair at every byte offset around a lane seam (16), a tile
    seam (4096) and the next one (8192, the check's step seam at these sizes) and around a document boundary there; documents of 0 and 1
    bytes, documents that begin with marks, truncated sequences followed by continuation bytes, ill-formed bytes, nothing to do, text
    that shrinks in every tile, text that triples, long mark runs, Hangul across a seam, a Maybe with nothing to compose with."""
    assert len(cases) > 400
    for name, (text, offs, want) in cases.items():
        same(tok.nfc(text, offs), want, name)
    text, offs, want = cases["marks 5000"]
    assert want[4][6] == 5001 and want[4][3] == 2
    text, offs, want = cases["nothing to do"]
    assert not want[2].any() and bytes(want[0]) == bytes(text)
    text, offs, want = cases["maybe with nothing to compose"]
    assert want[2].all() and not want[3].any()
    text, offs, want = cases["triples"]
    assert want[4][0] >= 3 * (4 * (TILE // 2 + 3))


def test_the_fixture(tok, nfc_golden):
    out, ooff, flags, changed, counts = tok.nfc(nfc_golden["text"], nfc_golden["offsets"])
    assert bytes(out) == bytes(nfc_golden["want"]) and np.array_equal(ooff, nfc_golden["want_offsets"])
    docs, want = nt.docs_of(nfc_golden["text"], nfc_golden["offsets"]), nt.docs_of(nfc_golden["want"], nfc_golden["want_offsets"])
    assert np.array_equal(changed, np.asarray([a != b for a, b in zip(docs, want)], dtype=np.uint8))


def test_check_and_device_forms(tok, side, cases):
    from tokendagger_amd import capi
    for name, (text, offs, want) in cases.items():
        got, c1, slack_ok, st1, st2, _ = device_call(tok, text, offs, side)
        assert st1[0] == capi.TD_OK, (name, st1)
        assert st2[0] == capi.TD_OK and slack_ok, (name, st2)
        same(got, want, name)
        assert c1.tolist() == [0, int(want[2].sum()), 0, 0, 0, 0, 0, 0], (name, c1)


@pytest.mark.parametrize("shift", range(1, 16))
def test_text_off_the_16_byte_grid(tok, side, cases, shift):
    for name in ("nfd of mixed, documents", "ill-formed", "truncated then continuation", "nothing to do", f"dirty0@{TILE - shift}/{TILE}",
                 f"ooo@{TILE - 1 - shift % 5}|{TILE}", "begins with a mark", "marks 33"):
        text, offs, want = cases[name]
        got, c1, slack_ok, st1, st2, _ = device_call(tok, text, offs, side, shift=shift)
        assert st1[0] == 0 and st2[0] == 0 and slack_ok, (name, st1, st2)
        same(got, want, (name, shift))
        assert c1[1] == int(want[2].sum())


def test_capacity_one_byte_short(tok, side, cases):
    from tokendagger_amd import capi
    text, offs, want = cases["nfd of mixed, documents"]
    need = int(want[4][0])
    got, _, slack_ok, _, st2, raw_out = device_call(tok, text, offs, side, cap=need - 1)
    assert st2 == (capi.TD_E_CAPACITY, need) and slack_ok and (raw_out == FILL).all(), st2
    assert got[4][0] == need and (got[1] == FILL).all()
    got, _, slack_ok, _, st2, _ = device_call(tok, text, offs, side, cap=need)
    assert st2[0] == capi.TD_OK and slack_ok
    same(got, want, "exact capacity")
    with pytest.raises(capi.TokenDaggerHipError) as e:
        tok.nfc(text, offs, capacity=need - 1)
    assert e.value.code == capi.TD_E_CAPACITY and e.value.counts[0] == need
    same(tok.nfc(text, offs, capacity=need), want, "host form, exact capacity")
    assert tok.nfc(text, offs, want_text=False)[4][0] == need


def test_bad_offsets_raise_through_device_status(tok, side, cases):
    from tokendagger_amd import capi
    text, offs, want = cases["nfd of mixed, documents"]
    dec = offs.copy()
    dec[3], dec[4] = offs[4], offs[3]
    first = offs.copy()
    first[0] = 1
    for o, n_bytes, where_want in ((dec, None, 3), (first, None, 0), (offs, len(text) - 10, len(offs) - 2)):
        got, c1, slack_ok, st1, st2, raw_out = device_call(tok, text, o, side, n_bytes=n_bytes)
        assert st1 == (capi.TD_E_INVALID, where_want) and st2 == (capi.TD_E_INVALID, where_want), (st1, st2, where_want)
        assert slack_ok and (raw_out == FILL).all() and (c1 == FILL).all() and (got[4] == FILL).all()
        assert (got[2] == FILL).all() and (got[3] == FILL).all() and (got[1] == FILL).all(), "an output was written although the offsets are bad"
        got, _, _, st1, st2, _ = device_call(tok, text, offs, side)  # (the error is cleared; the next good call)
        assert st1[0] == 0 and st2[0] == 0
        same(got, want, "after an error")
    import torch
    t = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    for call in (lambda: tok.nfc_check(t.data_ptr(), 8, t.data_ptr(), 1, t.data_ptr(), t.data_ptr(), 0),                      # the null stream
                 lambda: tok.nfc_device(t.data_ptr(), 8, t.data_ptr(), 1, t.data_ptr() + 64, 64, t.data_ptr(), 0, t.data_ptr(), 0),
                 lambda: tok.nfc_device(t.data_ptr(), 64, t.data_ptr(), 1, t.data_ptr() + 32, 64, t.data_ptr(), 0, t.data_ptr(), side.cuda_stream),
                 lambda: tok.nfc_check(t.data_ptr(), 8, t.data_ptr() + 4, 1, t.data_ptr(), t.data_ptr(), side.cuda_stream),
                 lambda: tok.nfc(text, dec), lambda: tok.nfc(text, first), lambda: tok.encode_batch_nfc(text, dec)):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            call()
        assert e.value.code == capi.TD_E_INVALID


def test_encode_batch_nfc(tok, cases):
    from tokendagger_amd import capi
    for name in ("nfd of mixed, documents", "nothing to do", "nfc of mixed", "begins with a mark", "empty documents", "empty", "marks 33"):
        text, offs, want = cases[name]
        for mode in (capi.TD_MODE_ENCODE, capi.TD_MODE_ORDINARY):
            ids, toff, norm, noff, changed, counts = tok.encode_batch_nfc(text, offs, mode, return_text=True)
            wi, wo = tok.encode_batch(want[0], want[1], mode)
            assert np.array_equal(ids, wi) and np.array_equal(toff, wo), (name, mode)
            assert bytes(norm) == bytes(want[0]) and np.array_equal(noff, want[1]) and np.array_equal(changed, want[3]), name
            assert counts[0] == want[4][0] and counts[1] == want[4][1], (name, counts)
            if want[4][1]:
                assert np.array_equal(counts, want[4])
        ids2, toff2, norm2, _, _, _ = tok.encode_batch_nfc(text, offs)  # (the normalised text is not asked for)
        wi, wo = tok.encode_batch(want[0], want[1])
        assert norm2 is None and np.array_equal(ids2, wi) and np.array_equal(toff2, wo), name
    text, offs, want = cases["nfd of mixed, documents"]
    plain, _ = tok.encode_batch(text, offs)
    assert not np.array_equal(plain, tok.encode_batch_nfc(text, offs)[0]), "the text was not normalised in front of the encode"


@pytest.mark.parametrize("fill", [0x5A, 0xFF])
def test_clone_on_a_second_stream_and_poisoned_workspaces(tok, side, cases, fill):
    """The whole of it once more (every limit case through the check, the device form and the host form, the encode on some) on a clone
    whose workspace is filled with `fill` from its first allocation on, on a stream of its own: everything must EQUAL td_nfc_host's
    answer, as it does without the fill (the tests above), so the runs are the same bit for bit; a second call repeats the first."""
    from tokendagger_amd import capi
    import torch
    other = torch.cuda.Stream(device=torch.device("cuda", 0))
    encoded = ("nfd of mixed, documents", "marks 300", "hangul across a seam", "triples", "many empty documents", "ill-formed below 0xCC")
    assert set(encoded) <= set(cases)
    tok.set_option(capi.TD_OPT_WS_FILL, fill)
    try:
        h = tok.clone()
    finally:
        tok.set_option(capi.TD_OPT_WS_FILL, -1)
    for name, (text, offs, want) in cases.items():
        got, c1, slack_ok, st1, st2, _ = device_call(h, text, offs, other)
        assert st1[0] == 0 and st2[0] == 0 and slack_ok
        same(got, want, (name, fill))
        assert c1.tolist() == [0, int(want[2].sum()), 0, 0, 0, 0, 0, 0], (name, fill, c1)
        same(h.nfc(text, offs), want, (name, fill, "host form"))
        if name in encoded:
            ids, toff, _, _, _, _ = h.encode_batch_nfc(text, offs)
            wi, wo = tok.encode_batch(want[0], want[1])
            assert np.array_equal(ids, wi) and np.array_equal(toff, wo), (name, fill)
            again, _, _, _, _, _ = device_call(h, text, offs, other)
            assert [np.asarray(x).tobytes() for x in again] == [np.asarray(x).tobytes() for x in got], (name, fill, "a repeat differs")


def test_counts_of_windows_proven_by_their_bytes(tok, side, cases):
    """counts[5] (opaque bytes) and counts[6] (the longest segment) are over the whole text: windows of bytes below 0xCC are copied without
    a look at the tables but hold opaque bytes (stray continuation bytes, 0xC0, 0xC1, two-byte leads cut short, also by a document's end),
    and ASCII in whole windows has segments of one code point."""
    for name, opaque, longest in (("ascii, whole windows", 0, 1), ("ascii, whole tiles", 0, 1), ("stray continuation bytes in whole windows", 15, 1),
                                  ("ill-formed below 0xCC", 8 * 40, 1), ("documents cut two-byte letters below 0xCC", 12, 1)):
        text, offs, want = cases[name]
        assert want[4].tolist() == [len(text), 0, 0, 0, 0, opaque, longest, 0], (name, want[4])
        for shift in (0, 7):
            got, _, _, st1, st2, _ = device_call(tok, text, offs, side, shift=shift)
            assert st1[0] == 0 and st2[0] == 0
            same(got, want, (name, shift))
        same(tok.nfc(text, offs), want, name)
        assert np.array_equal(tok.nfc(text, offs, want_text=False)[4], want[4]), name


@pytest.mark.parametrize("shift", range(16))
def test_the_checks_unrolled_loop(tok, side, shift):
    """td_nfc_check loads four windows a lane and round (g, g + step, g + 2 step, g + 3 step) while all four lie inside the text, which
    takes some hundreds of KB: dirty, out-of-order and in-order pieces and document boundaries around each of those seams and around the
    lane at the hand-over to the one-window loop, at every misalignment of the base."""
    from tokendagger_amd import capi
    n = 300007 + 16 * shift
    step, first, rounds = nt.check_loop_geometry(n, shift)
    assert rounds == 1 and 1 < first < step, "the text does not reach the unrolled loop and its hand-over"
    text, offs, seams = nt.check_loop_case(n, shift)
    assert len(seams) >= 6
    want = capi.nfc_host(text, offs)
    assert 0 < want[2].sum() < len(want[2]), "documents of both kinds"
    got, c1, slack_ok, st1, st2, _ = device_call(tok, text, offs, side, shift=shift)
    assert st1[0] == 0 and st2[0] == 0 and slack_ok, (st1, st2)
    same(got, want, shift)  # (flags: the check's)
    assert c1.tolist() == [0, int(want[2].sum()), 0, 0, 0, 0, 0, 0], c1
    if shift == 0:  # (the host forms upload to an aligned buffer)
        ids, toff, norm, noff, changed, counts = tok.encode_batch_nfc(text, offs, return_text=True)
        wi, wo = tok.encode_batch(want[0], want[1])
        assert np.array_equal(ids, wi) and np.array_equal(toff, wo)
        assert bytes(norm) == bytes(want[0]) and np.array_equal(noff, want[1]) and np.array_equal(counts, want[4])
        # the same text with its pieces out: proven by the unrolled loop, the original buffer is encoded
        clean = np.frombuffer(nt.filler(n), dtype=np.uint8).copy()
        ids, toff, norm, noff, changed, counts = tok.encode_batch_nfc(clean, offs, return_text=True)
        wi, wo = tok.encode_batch(clean, offs)
        assert np.array_equal(ids, wi) and np.array_equal(toff, wo) and bytes(norm) == bytes(clean) and not changed.any()
        assert counts.tolist() == [n, 0, 0, 0, 0, 0, 0, 0]


def test_the_checks_second_round(tok, side):
    """A text behind the 2048 workgroups' first sweep (32 MiB): lanes make a second round of four loads, others hand over after one."""
    from tokendagger_amd import capi
    n, shift = 57 * 2 ** 20 + 4321, 3
    step, first, rounds = nt.check_loop_geometry(n, shift)
    assert rounds == 2 and first < step
    text, offs, seams = nt.check_loop_case(n, shift)
    flags = capi.nfc_host(text, offs, want_text=False)[2]
    assert len(seams) >= 12 and 0 < flags.sum() < len(flags)
    got, c1, slack_ok, st1, _, _ = device_call(tok, text, offs, side, shift=shift, cap=0, check_only=True)
    assert st1[0] == 0 and slack_ok and np.array_equal(got[2], flags), (st1, got[2], flags)
    assert c1.tolist() == [0, int(flags.sum()), 0, 0, 0, 0, 0, 0], c1
