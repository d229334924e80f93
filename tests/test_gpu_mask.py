"""Address masking on the GPU (td_mask_addresses_device, td_mask_addresses, Tokenizer.mask_addresses) against the rule in plain Python
(tests/mask_truth.py): output bytes, offsets, stats and totals must be EQUAL.  The outputs lie in buffers filled with 0x77 that are
longer than the call may write.  No case here makes the device fault: every error is one the library reports by a status code."""
import numpy as np
import pytest

import helpers as H
import mask_truth as mt

pytestmark = pytest.mark.gpu

FILL, SLACK = 0x77, 9
CASES = mt.seam_cases()


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
def want():
    """name -> the truth's answer, computed once a case and left unchanged"""
    memo = {}
    return lambda name: memo.setdefault(name, mt.mask(CASES[name][0], CASES[name][1], **CASES[name][2]))


class Call:
    """One td_mask_addresses_device call enqueued on `stream`, the text `shift` bytes off the 16-byte grid; result() waits and reads back."""

    def __init__(self, tok, stream, text, offs, kw, shift=0, cap=None, want_out=True, want_offs=True, want_totals=True, n_bytes=None):
        import torch
        dev = torch.device("cuda", 0)
        text, offs = np.frombuffer(bytes(text), dtype=np.uint8), np.asarray(offs, dtype=np.int64)
        self.n_docs, self.cap, self.stream = len(offs) - 1, 6 * len(text) if cap is None else cap, stream
        with torch.cuda.stream(stream):
            self.raw = torch.from_numpy(np.concatenate([np.full(16 + shift, 0x40, np.uint8), text, np.full(16, 0x40, np.uint8)])).to(dev)
            self.offs = torch.from_numpy(offs).to(dev)
            self.out = torch.full((self.cap + SLACK,), FILL, dtype=torch.uint8, device=dev)
            self.ooff = torch.full((self.n_docs + 1 + SLACK,), FILL, dtype=torch.int64, device=dev)
            self.stats = torch.full((self.n_docs * 6 + SLACK,), FILL, dtype=torch.int64, device=dev)
            self.totals = torch.full((6 + SLACK,), FILL, dtype=torch.int64, device=dev)
            self.counts = torch.full((8,), FILL, dtype=torch.int64, device=dev)
        tok.mask_addresses_device(self.raw.data_ptr() + 16 + shift, len(text) if n_bytes is None else n_bytes, self.offs.data_ptr(), self.n_docs,
                                  mt.make_rules(kw), self.out.data_ptr() if want_out else 0, self.cap if want_out else 0,
                                  self.ooff.data_ptr() if want_offs else 0, self.stats.data_ptr(), self.totals.data_ptr() if want_totals else 0,
                                  self.counts.data_ptr(), stream.cuda_stream)

    def result(self):
        """-> ((text, offsets, stats, totals), counts, the slack behind every output is untouched, the whole buffers)"""
        self.stream.synchronize()
        out, ooff, stats, totals = (x.cpu().numpy() for x in (self.out, self.ooff, self.stats, self.totals))
        n = self.n_docs
        slack = bool((out[self.cap:] == FILL).all() and (ooff[n + 1:] == FILL).all() and (stats[6 * n:] == FILL).all() and (totals[6:] == FILL).all())
        need = min(int(ooff[n]), self.cap) if ooff[n] >= 0 else 0
        return (out[:need], ooff[:n + 1], stats[:6 * n].reshape(n, 6), totals[:6]), self.counts.cpu().numpy(), slack, (out, ooff, stats, totals)


@pytest.mark.parametrize("name", list(CASES))
def test_seam_cases(tok, side, want, name):
    from tokendagger_amd import capi
    text, offs, kw = CASES[name]
    call = Call(tok, side, text, offs, kw)
    assert tok.device_status_pos(side.cuda_stream) == (capi.TD_OK, 0)
    got, counts, slack, (out, _, _, _) = call.result()
    mt.same(got, want(name), name)
    assert slack and counts.tolist() == [len(want(name)[0])] + [0] * 7 and (out[len(got[0]):] == FILL).all()
    if not kw:
        assert bytes(got[0]) == text and got[1].tolist() == list(offs)
    if "on every seam" in name:
        assert got[3][0] + got[3][1] == call.n_docs  # every planted address was found
    if name == "eight literals":
        assert all(lit in bytes(got[0]) for lit in kw["emails"] + kw["ips"])


@pytest.mark.parametrize("shift", range(16))
def test_every_misalignment_of_the_text(tok, side, want, shift):
    for name in ("the @ on every seam", "the lengths between empty documents"):
        got, _, slack, _ = Call(tok, side, *CASES[name], shift=shift).result()
        mt.same(got, want(name), (name, shift))
        assert slack


def test_stats_only(tok, side, want):
    name = "more than 256 tiles"
    call = Call(tok, side, *CASES[name], want_out=False, want_offs=False, want_totals=False)
    assert tok.device_status_pos(side.cuda_stream)[0] == 0
    _, counts, _, (out, ooff, stats, totals) = call.result()
    n = call.n_docs
    assert stats[:6 * n].reshape(n, 6).tolist() == want(name)[2] and counts[0] == len(want(name)[0])
    assert (out == FILL).all() and (ooff == FILL).all() and (totals == FILL).all() and (stats[6 * n:] == FILL).all()


def test_capacity_one_byte_short(tok, side, want):
    from tokendagger_amd import capi
    name = "literals of 32 bytes"
    need = len(want(name)[0])
    assert need > len(CASES[name][0])  # the output has grown
    call = Call(tok, side, *CASES[name], cap=need - 1)
    assert tok.device_status_pos(side.cuda_stream) == (capi.TD_E_CAPACITY, need)
    _, counts, _, (out, ooff, _, _) = call.result()
    assert counts[0] == need and (out == FILL).all() and (ooff == FILL).all()
    call = Call(tok, side, *CASES[name], cap=need)
    assert tok.device_status_pos(side.cuda_stream)[0] == capi.TD_OK
    mt.same(call.result()[0], want(name), "exactly enough")
    with pytest.raises(capi.TokenDaggerHipError) as e:
        tok.mask_addresses(CASES[name][0], CASES[name][1], mt.make_rules(CASES[name][2]), capacity=need - 1)
    assert e.value.code == capi.TD_E_CAPACITY and str(need) in str(e.value)


@pytest.mark.parametrize("offs, n_bytes, bad", [([0, 30, 20, 10, 40], 40, 1), ([1, 10, 40], 40, 0), ([0, 10, 50], 40, 1), ([0, -1, 40], 40, 0)])
def test_bad_offsets_write_nothing(tok, side, offs, n_bytes, bad):
    from tokendagger_amd import capi
    call = Call(tok, side, mt.prose(64, mt.SAMPLE), offs, mt.BOTH, cap=64, n_bytes=n_bytes)
    assert tok.device_status_pos(side.cuda_stream) == (capi.TD_E_INVALID, bad)
    _, counts, _, whole = call.result()
    assert (counts == FILL).all() and all((x == FILL).all() for x in whole)


def test_three_calls_on_one_handle_without_a_host_wait(tok, side, want):
    """the later calls' rules differ: nothing of an earlier call's marks, dirty words or sums may reach them"""
    name = "the last byte on every seam"
    text, offs, _ = CASES[name]
    first = Call(tok, side, text, offs, mt.BOTH)
    second = Call(tok, side, text, offs, {})
    third = Call(tok, side, *CASES["eight literals"][:2], dict(ips=(b"<ip>",)))
    assert tok.device_status_pos(side.cuda_stream)[0] == 0
    mt.same(first.result()[0], want(name), "first")
    mt.same(second.result()[0], mt.mask(text, offs), "second")
    mt.same(third.result()[0], mt.mask(*CASES["eight literals"][:2], ips=(b"<ip>",)), "third")
    assert bytes(second.result()[0][0]) == text


def test_mask_addresses_feeds_the_encode(tok, want):
    import tokendagger as tiktoken
    pat, mr, special = H.llama4()
    tk = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    name = "the lengths between empty documents"
    text, offs, kw = CASES[name]
    mk = tk.mask_addresses(text, np.asarray(offs, dtype=np.int64), emails=kw["emails"], ips=kw["ips"], keep_private_ips=False)
    mt.same((mk.text, mk.offsets, mk.stats, mk.totals), want(name), "Tokenizer.mask_addresses")
    assert np.array_equal(mk.emails, mk.stats[:, 0]) and np.array_equal(mk.out_bytes, np.diff(mk.offsets)) and mk.totals[1] > 0
    mt.same(tok.mask_addresses(text, offs, mt.make_rules(kw)), want(name), "td_mask_addresses")
    ids, toff = tk.encode_batch_to_numpy(mk.text, mk.offsets)
    e_ids, e_off = tk.encode_batch_to_numpy(np.frombuffer(want(name)[0], dtype=np.uint8), np.asarray(want(name)[1], dtype=np.int64))
    assert np.array_equal(ids, e_ids) and np.array_equal(toff, e_off) and len(ids) > 0
