"""UTF-8 validation and repair on the GPU (td_utf8_check_device, td_utf8_device, td_utf8, td_encode_batch_utf8) against td_utf8_host.
Text, offsets, flags, first_bad, n_bad and counts must be EQUAL.  In the device buffer the text lies between guard bytes: `E2 82` in
front of it and `80 80 80` behind it, inside the allocation: a kernel that looked outside the text would consume a leading continuation
byte or complete a truncated tail, and the comparison would show it.  No case here makes the device fault: every error is one the
library reports by a status code."""
import numpy as np
import pytest

import helpers as H
import utf8_truth as ut

pytestmark = pytest.mark.gpu

FILL = 0x77
TILE = 4096
POLICIES = [ut.REPLACE, ut.IGNORE]


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
    """Built once, shared and left unchanged: name -> (text, offsets, {policy: td_utf8_host's answer})."""
    from tokendagger_amd import capi
    return {name: (text, offs, {p: capi.utf8_host(text, offs, p) for p in POLICIES}) for name, (text, offs) in ut.limit_cases(TILE).items()}


def device_call(tok, text, offs, stream, policy=ut.REPLACE, shift=0, cap=None, slack=9, n_bytes=None, check_only=False, first=True):
    """td_utf8_check_device, then td_utf8_device on a text whose base lies `shift` bytes off the 16-byte grid, between the guard bytes ->
    ((out, out_offsets, flags, first_bad, n_bad, counts) of the repair, (flags, first_bad, counts) of the check, slack untouched, the two
    statuses with their positions, the whole output buffer)."""
    import torch
    dev = torch.device("cuda", 0)
    text, offs = np.ascontiguousarray(text, dtype=np.uint8), np.ascontiguousarray(offs, dtype=np.int64)
    n_docs, n = len(offs) - 1, len(text) if n_bytes is None else n_bytes
    cap = 3 * len(text) if cap is None else cap
    front = np.full(16 + shift, 0x41, np.uint8)
    front[-2:] = (0xE2, 0x82)
    back = np.full(16, 0x41, np.uint8)
    back[:3] = 0x80
    with torch.cuda.stream(stream):
        raw = torch.from_numpy(np.concatenate([front, text, back])).to(dev)
        d_offs = torch.from_numpy(offs).to(dev)
        d_out = torch.full((cap + slack,), FILL, dtype=torch.uint8, device=dev)
        d_ooff = torch.full((n_docs + 1 + slack,), FILL, dtype=torch.int64, device=dev)
        d_f1, d_f2 = (torch.full((n_docs + slack,), FILL, dtype=torch.uint8, device=dev) for _ in range(2))
        d_b1, d_b2, d_nb = (torch.full((n_docs + slack,), FILL, dtype=torch.int64, device=dev) for _ in range(3))
        d_c1, d_c2 = (torch.full((8,), FILL, dtype=torch.int64, device=dev) for _ in range(2))
    s = stream.cuda_stream
    tok.utf8_check(raw.data_ptr() + 16 + shift, n, d_offs.data_ptr(), n_docs, d_f1.data_ptr(), d_b1.data_ptr() if first else 0, d_c1.data_ptr(), s)
    st1 = tok.device_status_pos(s)
    st2 = (0, 0)
    if not check_only:
        tok.utf8_device(raw.data_ptr() + 16 + shift, n, d_offs.data_ptr(), n_docs, policy, d_out.data_ptr(), cap, d_ooff.data_ptr(), d_f2.data_ptr(),
                        d_b2.data_ptr(), d_nb.data_ptr(), d_c2.data_ptr(), s)
        st2 = tok.device_status_pos(s)
    stream.synchronize()
    out, ooff = d_out.cpu().numpy(), d_ooff.cpu().numpy()
    f1, f2, b1, b2, nb = (x.cpu().numpy() for x in (d_f1, d_f2, d_b1, d_b2, d_nb))
    c1, c2 = d_c1.cpu().numpy(), d_c2.cpu().numpy()
    slack_ok = bool((out[cap:] == FILL).all() and (ooff[n_docs + 1:] == FILL).all() and all((x[n_docs:] == FILL).all() for x in (f1, f2, b1, b2, nb)))
    need = int(c2[0]) if st2[0] == 0 and not check_only else 0
    return ((out[:need] if need <= cap else out, ooff[:n_docs + 1], f2[:n_docs], b2[:n_docs], nb[:n_docs], c2), (f1[:n_docs], b1[:n_docs], c1),
            slack_ok, st1, st2, out)


def check_same(chk, want, what):
    f1, b1, c1 = chk
    assert np.array_equal(f1, want[2]), (what, "the check's flags", f1[:16], want[2][:16])
    assert np.array_equal(b1, want[3]), (what, "the check's first_bad", b1[:16], want[3][:16])
    assert c1.tolist() == [0, int(want[2].sum()), 0, 0, 0, 0, 0, 0], (what, c1)


def test_limit_cases_through_the_host_form(tok, cases):
    """Every limit case (tests/utf8_truth.py): every sequence length, truncated sequence and restricted second byte astride a window
    seam (16, 48), a tile seam (4096) and the next one (8192, the check's step seam at these sizes) at every split point; a document
    boundary at every position inside a sequence, alone and on those seams, with empty and one-byte documents there; documents of 0 to 3
    bytes; documents that begin with continuation bytes or end in a lead; no documents, empty text, documents at the text's end, bytes
    behind the last document; a tile of stray continuation bytes between clean tiles; clean tiles next to one bad byte; tiles of one
    sequence length; mixed scripts; noise."""
    assert len(cases) > 150
    for name, (text, offs, want) in cases.items():
        for policy in POLICIES:
            ut.same(tok.utf8(text, offs, policy), want[policy], (name, policy))
        _, _, flags, first, _, counts = tok.utf8(text, offs, check_only=True)  # (no output, offsets or n_bad asked for: the check)
        check_same((flags, first, counts), want[0], (name, "td_utf8 as the check"))
    text, offs, want = cases["a tile of strays"]
    assert want[ut.REPLACE][5][0] == len(text) + 2 * TILE and want[ut.IGNORE][5][0] == len(text) - TILE
    text, offs, want = cases["all ascii"]
    assert not want[0][2].any() and bytes(want[0][0]) == bytes(text)


@pytest.mark.parametrize("policy", POLICIES)
def test_check_and_device_forms(tok, side, cases, policy):
    from tokendagger_amd import capi
    for name, (text, offs, want) in cases.items():
        got, chk, slack_ok, st1, st2, _ = device_call(tok, text, offs, side, policy)
        assert st1[0] == capi.TD_OK, (name, st1)
        assert st2[0] == capi.TD_OK and slack_ok, (name, st2)
        ut.same(got, want[policy], (name, policy))
        check_same(chk, want[policy], name)


@pytest.mark.parametrize("shift", range(1, 16))
def test_text_off_the_16_byte_grid(tok, side, cases, shift):
    names = [n for n in cases if n.startswith("shorter than a window")] + [
        "noise, documents", "small documents", "mixed scripts, cut every 1000", "a tile of strays, documents", "all three, one cut",
        "clean tiles next to one bad byte, documents", f"four@{shift % 5}", "boundary in four@2, tile seam, empty documents", "empty", "no documents"]
    for name in names:
        text, offs, want = cases[name]
        policy = (shift + len(name)) % 2
        got, chk, slack_ok, st1, st2, _ = device_call(tok, text, offs, side, policy, shift=shift)
        assert st1[0] == 0 and st2[0] == 0 and slack_ok, (name, st1, st2)
        ut.same(got, want[policy], (name, shift))
        check_same(chk, want[policy], (name, shift))


def test_capacity_one_byte_short(tok, side, cases):
    from tokendagger_amd import capi
    text, offs, want = cases["noise, documents"]
    for policy in POLICIES:
        need = int(want[policy][5][0])
        got, _, slack_ok, _, st2, raw_out = device_call(tok, text, offs, side, policy, cap=need - 1)
        assert st2 == (capi.TD_E_CAPACITY, need) and slack_ok and (raw_out == FILL).all(), st2
        assert got[5][0] == need and (got[1] == FILL).all()
        got, _, slack_ok, _, st2, _ = device_call(tok, text, offs, side, policy, cap=need)
        assert st2[0] == capi.TD_OK and slack_ok
        ut.same(got, want[policy], "exact capacity")
        with pytest.raises(capi.TokenDaggerHipError) as e:
            tok.utf8(text, offs, policy, capacity=need - 1)
        assert e.value.code == capi.TD_E_CAPACITY and e.value.counts[0] == need
        ut.same(tok.utf8(text, offs, policy, capacity=need), want[policy], "host form, exact capacity")
        assert tok.utf8(text, offs, policy, want_text=False)[5][0] == need


def test_bad_offsets_raise_through_device_status(tok, side, cases):
    from tokendagger_amd import capi
    text, offs, want = cases["noise, documents"]
    dec = offs.copy()
    dec[3], dec[4] = offs[4], offs[3]
    assert dec[3] > dec[4]
    first = offs.copy()
    first[0] = 1
    for o, n_bytes, where_want in ((dec, None, 3), (first, None, 0), (offs, len(text) - 10, None)):
        if where_want is None:
            where_want = int(np.argmax(offs[1:] > len(text) - 10))
        got, chk, slack_ok, st1, st2, raw_out = device_call(tok, text, o, side, n_bytes=n_bytes)
        assert st1 == (capi.TD_E_INVALID, where_want) and st2 == (capi.TD_E_INVALID, where_want), (st1, st2, where_want)
        assert slack_ok and (raw_out == FILL).all() and (chk[2] == FILL).all() and (got[5] == FILL).all()
        assert all((x == FILL).all() for x in (got[1], got[2], got[3], got[4], chk[0], chk[1])), "an output was written although the offsets are bad"
        got, _, _, st1, st2, _ = device_call(tok, text, offs, side)  # (the error is cleared; the next good call)
        assert st1[0] == 0 and st2[0] == 0
        ut.same(got, want[0], "after an error")
    import torch
    t = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    p, s = t.data_ptr(), side.cuda_stream
    for call in (lambda: tok.utf8_check(p, 8, p, 1, p, p, p, 0),                                          # the null stream
                 lambda: tok.utf8_device(p, 8, p, 1, 0, p + 64, 64, p, 0, 0, 0, p, 0),
                 lambda: tok.utf8_device(p, 64, p, 1, 0, p + 32, 64, p, 0, 0, 0, p, s),                    # the output overlaps the text
                 lambda: tok.utf8_device(p, 8, p, 1, 2, p + 64, 64, p, 0, 0, 0, p, s),                     # no such policy
                 lambda: tok.utf8_check(p, 8, p + 4, 1, p, p, p, s),                                       # offsets off their alignment
                 lambda: tok.utf8(text, dec), lambda: tok.utf8(text, first), lambda: tok.utf8(text, offs, 7),
                 lambda: tok.encode_batch_utf8(text, dec), lambda: tok.encode_batch_utf8(text, offs, policy=3),
                 lambda: tok.encode_batch_utf8(text, offs, mode=capi.TD_MODE_ENCODE + 5)):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            call()
        assert e.value.code == capi.TD_E_INVALID


def test_null_first_bad(tok, side, cases):
    text, offs, want = cases["noise, documents"]
    _, chk, slack_ok, st1, _, _ = device_call(tok, text, offs, side, check_only=True, first=False)
    assert st1[0] == 0 and slack_ok and np.array_equal(chk[0], want[0][2]) and (chk[1] == FILL).all()
    assert chk[2].tolist() == [0, int(want[0][2].sum()), 0, 0, 0, 0, 0, 0]


def test_encode_batch_utf8(cases):
    """ids and token offsets equal td_encode_batch of the codec-repaired bytes on the same handle, for Llama-4 and one generic pattern; on
    clean text they equal td_encode_batch of the input itself."""
    from tokendagger_amd import capi
    import cases as C
    pat, mr, special = H.llama4()
    toks = [capi.HipTokenizer(pat, mr, special, device=0),
            capi.HipTokenizer(C.SUPPORTED_GENERIC_PATTERNS[0], {bytes([b]): b for b in range(256)}, {}, device=0)]
    for tok in toks:
        for name in ("noise, documents", "small documents", "mixed scripts, cut every 7", "a tile of strays, documents", "empty", "no documents",
                     "boundary in four@2, tile seam, empty documents", "documents at the text's end"):
            text, offs, want = cases[name]
            for policy in POLICIES:
                codec = ut.truth(text, offs, policy, ut.codec_walk)
                assert bytes(codec[0]) == bytes(want[policy][0])
                for mode in (capi.TD_MODE_ENCODE, capi.TD_MODE_ORDINARY):
                    ids, toff, fixed, foff, flags, first, nbad, counts = tok.encode_batch_utf8(text, offs, mode, policy, return_text=True)
                    wi, wo = tok.encode_batch(codec[0], codec[1], mode)
                    assert np.array_equal(ids, wi) and np.array_equal(toff, wo), (name, policy, mode)
                    ut.same((fixed, foff, flags, first, nbad, counts), want[policy], (name, policy))
                ids2, toff2, fixed2 = tok.encode_batch_utf8(text, offs, policy=policy)[:3]
                assert fixed2 is None and np.array_equal(ids2, wi) and np.array_equal(toff2, wo), name
        for name in ("all ascii", "mixed scripts", "all three", "all four"):
            text, offs, want = cases[name]
            assert not want[0][2].any()
            ids, toff, fixed, foff, flags, first, nbad, counts = tok.encode_batch_utf8(text, offs, return_text=True)
            wi, wo = tok.encode_batch(text, offs)
            assert np.array_equal(ids, wi) and np.array_equal(toff, wo) and bytes(fixed) == bytes(text) and np.array_equal(foff, offs)
            assert counts.tolist() == [len(text), 0, 0, 0, 0, 0, 0, 0] and not flags.any() and (first == -1).all() and not nbad.any()


@pytest.mark.parametrize("fill", [0x5A, 0xFF])
def test_clone_on_a_second_stream_and_poisoned_workspaces(tok, cases, fill):
    """The whole of it once more (every limit case through the check, the device form and the host form, the encode on some) on a clone
    whose workspace is filled with `fill` from its first allocation on, on a stream of its own: everything must EQUAL td_utf8_host's
    answer, and a second call repeats the first bit for bit."""
    from tokendagger_amd import capi
    import torch
    other = torch.cuda.Stream(device=torch.device("cuda", 0))
    encoded = ("noise, documents", "a tile of strays, documents", "small documents behind a tile", "mixed scripts, cut every 1000")
    tok.set_option(capi.TD_OPT_WS_FILL, fill)
    try:
        h = tok.clone()
    finally:
        tok.set_option(capi.TD_OPT_WS_FILL, -1)
    for name, (text, offs, want) in cases.items():
        policy = ut.REPLACE if fill == 0x5A else ut.IGNORE
        got, chk, slack_ok, st1, st2, _ = device_call(h, text, offs, other, policy)
        assert st1[0] == 0 and st2[0] == 0 and slack_ok
        ut.same(got, want[policy], (name, fill))
        check_same(chk, want[policy], (name, fill))
        ut.same(h.utf8(text, offs, policy), want[policy], (name, fill, "host form"))
        again, chk2, _, _, _, _ = device_call(h, text, offs, other, policy)
        assert [np.asarray(x).tobytes() for x in again + chk2] == [np.asarray(x).tobytes() for x in got + chk], (name, fill, "a repeat differs")
        if name in encoded:
            ids, toff = h.encode_batch_utf8(text, offs, policy=policy)[:2]
            wi, wo = tok.encode_batch(want[policy][0], want[policy][1])
            assert np.array_equal(ids, wi) and np.array_equal(toff, wo), (name, fill)


@pytest.mark.parametrize("shift", range(16))
def test_the_checks_multi_load_loop(tok, side, shift):
    """td_utf8_check loads four windows a lane and round (g, g + step, g + 2 step, g + 3 step) while all four have four bytes of the text on
    either side.  launch_utf8_check starts min(ceil((n + 16) / 16384), 2048) workgroups of 256 lanes, so a text below 32 MiB is one round
    whose four loads lie n / 4 apart: 300 KB here.  Behind each of the four loads EVERY piece of utf8_truth.PIECES (every sequence length,
    every truncated sequence, each restricted second byte, C0, F5, FF, stray continuation bytes) lies astride a window seam at EVERY
    split point (63 combinations, utf8_truth.check_loop_case), every other one with a document boundary on the seam, at every misalignment
    of the base."""
    from tokendagger_amd import capi
    n = 300007 + 16 * shift
    step, rounds = ut.check_loop_geometry(n, shift)
    assert rounds == 1
    text, offs, seams = ut.check_loop_case(n, shift)
    assert len(seams) == 4 and len(ut.COMBOS) == 63
    policy = shift % 2
    want = capi.utf8_host(text, offs, policy)
    assert 0 < want[2].sum() < len(want[2]), "documents of both kinds"
    got, chk, slack_ok, st1, st2, _ = device_call(tok, text, offs, side, policy, shift=shift)
    assert st1[0] == 0 and st2[0] == 0 and slack_ok, (st1, st2)
    ut.same(got, want, shift)
    check_same(chk, want, shift)


@pytest.mark.parametrize("shift", range(16))
def test_the_checks_multi_load_loop_on_dense_text(tok, side, shift):
    """The same on text without a single window of ASCII (two-, three- and four-byte sequences in every window): the four-load loop screens
    every window it loads, the case the validator is built for.  130 KB: 8 workgroups, step = 2048 windows, one round of four loads for
    the lanes up to window 1024; all 63 combinations behind each load, which also cut the characters they are written over."""
    from tokendagger_amd import capi
    n = 130003 + 16 * shift
    step, rounds = ut.check_loop_geometry(n, shift)
    assert step == 2048 and rounds == 1
    text, offs, seams = ut.check_loop_case(n, shift, ut.dense)
    assert len(seams) == 4
    g = (np.arange(n) + shift) // 16
    assert (np.bincount(g, weights=(text >= 0x80))[1:] > 0).all(), "a window of ASCII behind the first one (which may be one byte)"
    policy = (shift + 1) % 2
    want = capi.utf8_host(text, offs, policy)
    assert want[2].sum() > 0 and want[5][2] > 4 * 40
    got, chk, slack_ok, st1, st2, _ = device_call(tok, text, offs, side, policy, shift=shift)
    assert st1[0] == 0 and st2[0] == 0 and slack_ok, (st1, st2)
    ut.same(got, want, shift)
    check_same(chk, want, shift)
    # the text itself, nothing planted, one document: clean up to where n cuts it
    clean = np.frombuffer(ut.dense(n), dtype=np.uint8)
    one = np.asarray([0, n], dtype=np.int64)
    want = capi.utf8_host(clean, one, policy)
    assert want[4][0] <= 1
    got, chk, slack_ok, st1, st2, _ = device_call(tok, clean, one, side, policy, shift=shift)
    assert st1[0] == 0 and st2[0] == 0 and slack_ok
    ut.same(got, want, (shift, "clean"))
    check_same(chk, want, (shift, "clean"))


@pytest.mark.parametrize("shift", range(16))
def test_the_checks_second_round(tok, side, shift):
    """A text on which a lane makes TWO rounds of four loads: the grid is capped at 2048 workgroups, so step = 2048 * 256 windows = 8 MiB
    and the second round's last load lies 7 steps = 56 MiB behind the lane's first window: lane 256 (the first whose window has four
    bytes of the text in front of it) makes two rounds from 56 MiB + 4 KiB + 20 bytes on.  57 MiB, every piece at every split point
    behind every load of both rounds (utf8_truth.check_loop_case), at every misalignment of the base, the check alone."""
    from tokendagger_amd import capi
    n = 57 * 2 ** 20 + 4321
    step, rounds = ut.check_loop_geometry(n, shift)
    assert step == 2048 * 256 and rounds == 2
    text, offs, seams = ut.check_loop_case(n, shift)
    _, _, flags, first, _, _ = capi.utf8_host(text, offs, want_text=False)
    assert len(seams) >= 7 and 0 < flags.sum() < len(flags)
    _, chk, slack_ok, st1, _, _ = device_call(tok, text, offs, side, shift=shift, cap=0, check_only=True)
    assert st1[0] == 0 and slack_ok
    check_same(chk, (None, None, flags, first), "second round")
