"""Allowed special tokens cut out on the device (td_special.hip: scan, match, accept, mark, ids) on adversarial literal sets, bit
for bit.  Every case goes through td_encode_device_with_special and is compared three ways, ids and document offsets both:

  * with special_truth.expected_ids: tiktoken's rule stated twice in plain Python (the two statements must agree), the text between
    the cuts encoded by the plain-C port of oracle/ under the handle's split pattern;
  * with the host search (TD_OPT_DEVICE_SPECIALS = 0, segment_document in td_api_special.cpp);
  * from 1 MiB on, with td_encode_batch_with_special on its device route.

The sets (tests/special_truth.py gives each its reason): prefix chains the match has to climb, one literal per length 1 to 48, bytes
above 0x7F, literals of letters, digits and whitespace whose pieces are no whole tokens, aliases, 1-byte literals.  The placements:
the two-byte key across two lanes of the scan, every offset around a token tile border and a workgroup's pass, texts shorter than
a scan word, an unaligned text pointer, empty documents.  The configurations: the fused and the two-kernel tile loop, dedupe, the
long-piece fork, graph replay, a poisoned workspace, four pattern families.  The exits: candidate overflow (TD_E_SCRATCH and the
fall-back of the batch entry), a literal of 49 bytes, a generic pattern.  No case makes the device fault or wait."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import helpers as H
import special_truth as stt
from oracle import port
from tokendagger_amd import capi, vocab_io

pytestmark = pytest.mark.gpu

TD_E_PATTERN, TD_E_SCRATCH = 2, 6  # include/tokendagger_hip.h
AUTOGEN = r"[a-zA-Z]+|\s+|[0-9]+|[^\w\s]"  # a generic pattern (tests/test_gpu_determinism.py)
FAMILIES = {  # name -> (pattern, the port's variant)
    "llama4": (None, port.VARIANT_LLAMA4),
    "cl100k": (H.CL100K_PAT, port.VARIANT_CL100K),
    "gpt2": (H.GPT2_PAT, port.VARIANT_GPT2),
    "tekken": (H.TEKKEN_PAT, port.VARIANT_TEKKEN),
    "qwen2": (vocab_io.QWEN2_PAT_STR, port.VARIANT_QWEN2),  # (the truth tests/test_qwen2_pattern.py and test_gpu_determinism.py use)
}


@functools.lru_cache(maxsize=None)
def _ranks():
    pat, mr, _ = H.llama4()
    return pat, {b: r for b, r in mr.items() if r < 200000}


@functools.lru_cache(maxsize=None)
def _port(family: str = "llama4"):
    if not port.available():
        H.port_tokenizer()  # (builds it)
    return port.OracleTokenizer(_ranks()[1], FAMILIES[family][1])


def _handle(family: str = "llama4"):
    pat, ranks = _ranks()
    t = capi.HipTokenizer(FAMILIES[family][0] or pat, ranks, stt.vocabulary(), device=0)
    t.set_option(capi.TD_OPT_SMALL_PATH, 0)
    return t


@pytest.fixture(scope="module")
def tok():
    t = _handle()
    yield t
    t.close()


@functools.lru_cache(maxsize=None)
def _expected(call_index: int, family: str = "llama4"):
    """The truth of a call, computed once and shared."""
    c = stt.calls()[call_index] if call_index >= 0 else stt.config_call()
    return stt.expected_ids(c.text, c.offs, stt.literals(c.set_name), _port(family).encode)


def _stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream


class _Buffers:
    """A call's text at `shift` bytes behind a 16-byte boundary, its offsets, and outputs pre-filled with 0xFF bytes."""

    def __init__(self, text: bytes, offs, shift: int = 0):
        import torch
        self.n, self.nd = len(text), len(offs) - 1
        base = torch.zeros(self.n + shift + 16, dtype=torch.uint8, device="cuda")
        assert base.data_ptr() % 16 == 0
        if self.n:
            base[shift:shift + self.n] = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        self.base, self.text_ptr = base, base.data_ptr() + shift
        self.offs = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).cuda()
        self.cap = self.n + 1024
        self.ids = torch.empty(self.cap, dtype=torch.int32, device="cuda")
        self.toff = torch.empty(self.nd + 1, dtype=torch.int64, device="cuda")

    def run(self, tok, allowed, status=True):
        self.ids.fill_(-1)
        self.toff.fill_(-1)
        s = _stream()
        tok.encode_device_with_special(self.text_ptr, self.n, self.offs.data_ptr(), self.nd, allowed, self.ids.data_ptr(), self.cap,
                                       self.toff.data_ptr(), s)
        if status:
            tok.device_status(s)
        toff = self.toff.cpu().numpy()
        return self.ids[:max(int(toff[-1]), 0)].cpu().numpy(), toff


def _same(got, want, what):
    (gi, go), (wi, wo) = got, want
    assert np.array_equal(go, wo), f"{what}: document offsets differ, first at document {int(np.flatnonzero(np.asarray(go) != np.asarray(wo))[0]) if len(go) == len(wo) else '?'} (total {go[-1]} != {wo[-1]})"
    bad = np.flatnonzero(gi != wi)
    assert bad.size == 0, f"{what}: {bad.size} ids differ, first at token {int(bad[0])}: {gi[bad[0]:bad[0] + 4]} != {wi[bad[0]:bad[0] + 4]}"


def _three_ways(tok, c, want, what, buffers=None):
    """the device search against the truths; the host search against the truths; from 1 MiB on the batch entry's device route too"""
    allowed = stt.allowed_ids(c.set_name)
    b = buffers or _Buffers(c.text, c.offs, c.ptr_shift)
    _same(b.run(tok, allowed), want, f"{what}: the device search against the truths")
    tok.set_option(capi.TD_OPT_DEVICE_SPECIALS, 0)
    try:
        host = tok.encode_batch_with_special(c.text, c.offs, allowed)
    finally:
        tok.set_option(capi.TD_OPT_DEVICE_SPECIALS, 1)
    _same(host, want, f"{what}: the host search against the truths")
    if len(c.text) >= 1 << 20:
        _same(tok.encode_batch_with_special(c.text, c.offs, allowed), want, f"{what}: td_encode_batch_with_special on its device route")
    return b


# ---- the sets and the placements -------------------------------------------------------------------------------------------------------

def test_the_multi_id_literal_is_more_than_one_id():
    """... as ordinary text, so that td_special_ids meets had > 1 on its piece; the other pieces the sets rely on"""
    O = _port()
    assert len(O.encode(stt.MULTI_ID.encode())) > 1
    assert len(O.encode(b" wkkjqxzv")) > 1 and len(O.encode(stt.LETTERS48.encode())) > 1


@pytest.mark.parametrize("group", ["sets", "scan_words", "borders", "tiny", "pointer", "soups"])
def test_every_call_of_a_group_three_ways(tok, group):
    seen = 0
    for k, c in enumerate(stt.calls()):
        if c.group != group:
            continue
        _three_ways(tok, c, _expected(k), c.name)
        seen += 1
        if c.name == "words":
            assert tok.info(capi.TD_INFO_LONG_PIECES) > 0, "the literals inside pieces above 64 bytes and above 1 KiB made no long piece"
    assert seen >= 3


def test_a_text_above_one_mebibyte_on_both_entries(tok):
    """The batch entry searches on the device from 1 MiB on: the words set sprinkled over ordinary text, cut into documents."""
    L = [s.encode() for s in stt.SETS["words"][0]]
    docs = [stt.filler(9000 + 37 * k, seed=300 + k) + L[k % len(L)] + stt.filler(500, seed=k) + L[(k + 3) % len(L)] for k in range(112)]
    c = stt.Call("words over 1 MiB", "words", docs)
    assert len(c.text) >= 1 << 20
    want = stt.expected_ids(c.text, c.offs, stt.literals("words"), _port().encode)
    assert int((want[0] >= 200000).sum()) == 224
    _three_ways(tok, c, want, c.name)


# ---- the configurations ----------------------------------------------------------------------------------------------------------------

def _clone(tok, options, fill=-1):
    tok.set_option(capi.TD_OPT_WS_FILL, fill)
    try:
        t = tok.clone()
    finally:
        tok.set_option(capi.TD_OPT_WS_FILL, -1)
    for what, value in options.items():
        t.set_option(what, value)
    return t


@pytest.fixture(scope="module")
def config_buffers():
    c = stt.config_call()
    return c, _Buffers(c.text, c.offs)


def _configured(tok, config_buffers, options, what, fill=-1, calls=3):
    c, b = config_buffers
    want = _expected(-1)
    allowed = stt.allowed_ids(c.set_name)
    t = _clone(tok, options, fill)
    try:
        for rep in range(calls):  # (the first call of a handle has not seen long pieces yet: the fork engages behind it)
            _same(b.run(t, allowed), want, f"{what}, call {rep}")
            assert t.info(capi.TD_INFO_LONG_PIECES) >= 2048, "too few long pieces for the second stream to be taken"
        return t.info(capi.TD_INFO_WS_FILLED_BYTES)
    finally:
        t.close()


def test_the_configuration_case_three_ways(tok, config_buffers):
    c, b = config_buffers
    _three_ways(tok, c, _expected(-1), c.name, b)


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("dedupe", [0, 1])
@pytest.mark.parametrize("overlap", [0, 1])
def test_fused_dedupe_overlap(tok, config_buffers, fused, dedupe, overlap):
    _configured(tok, config_buffers, {capi.TD_OPT_FUSED: fused, capi.TD_OPT_DEDUPE: dedupe, capi.TD_OPT_OVERLAP: overlap},
                f"fused {fused}, dedupe {dedupe}, overlap {overlap}")


def test_direct_and_sparse_are_ignored_with_specials(tok, config_buffers):
    _configured(tok, config_buffers, {capi.TD_OPT_DIRECT: 1, capi.TD_OPT_SPARSE: 1}, "direct 1, sparse 1")
    _configured(tok, config_buffers, {capi.TD_OPT_DIRECT: 1, capi.TD_OPT_SPARSE: 1, capi.TD_OPT_FUSED: 0}, "direct 1, sparse 1, fused 0")


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_a_poisoned_workspace(tok, config_buffers, fill):
    assert _configured(tok, config_buffers, {}, f"fill 0x{fill:02X}", fill=fill) >= 8 * config_buffers[1].n


def test_graph_replay_with_changing_tables(tok, config_buffers):
    """Four identical calls (capture on the second), then two allowed sets of equal count and equal maxlen in turn: the graph's key is
    the same, only the table's contents differ."""
    c, b = config_buffers
    t = _clone(tok, {capi.TD_OPT_GRAPH: 1})
    try:
        for rep in range(4):
            _same(b.run(t, stt.allowed_ids("words")), _expected(-1), f"graph, words, call {rep}")
        O = _port().encode
        wants = {s: stt.expected_ids(c.text, c.offs, stt.literals(s), O) for s in ("graph_a", "graph_b")}
        assert int((wants["graph_a"][0] >= 200000).sum()) > 20 and not np.array_equal(wants["graph_a"][0], wants["graph_b"][0])
        for rep in range(6):
            s = ("graph_a", "graph_b")[rep & 1]
            _same(b.run(t, stt.allowed_ids(s)), wants[s], f"graph, {s}, call {rep}")
    finally:
        t.close()


@pytest.mark.parametrize("family", ["cl100k", "gpt2", "tekken", "qwen2"])
def test_pattern_families(family, config_buffers):
    """The same vocabulary under another split pattern: the literals' pieces fall differently, the truth comes from the port's variant."""
    c, b = config_buffers
    t = _handle(family)
    try:
        want = _expected(-1, family)
        _three_ways(t, c, want, f"{family}: {c.name}", b)
        for k, cc in enumerate(stt.calls()):
            if cc.name in ("words", "nonascii", "lens", "chain"):
                _three_ways(t, cc, _expected(k, family), f"{family}: {cc.name}")
    finally:
        t.close()


# ---- the exits: status returns, none of them faults or waits -----------------------------------------------------------------------------

def test_candidate_overflow_is_a_status_and_the_handle_goes_on():
    """A fresh handle, the 1-byte literal '|' and 256 KiB of it: n candidates against a list of n / 32 + 4096 (grown by an eighth by
    the handle's allocator: about 14 000).  Every write of the kernels stays inside min(count, capacity); the status is TD_E_SCRATCH."""
    t = _handle()
    try:
        n = 256 << 10
        b = _Buffers(b"|" * n, [0, n])
        allowed = stt.allowed_ids("one_byte")
        b.run(t, allowed, status=False)
        with pytest.raises(capi.TokenDaggerHipError) as e:
            t.device_status(_stream())
        assert e.value.code == TD_E_SCRATCH
        # the next call on the same handle is right
        k = [i for i, c in enumerate(stt.calls()) if c.name == "one_byte"][0]
        c = stt.calls()[k]
        _same(_Buffers(c.text, c.offs).run(t, allowed), _expected(k), "one_byte behind the overflow")
        # the batch entry falls back to the host search: 128 KiB of candidates (more than the list of 1 MiB holds: n / 32 + 4096 and
        # an eighth are about 41 500), then words with one more every 16 bytes
        text = b"|" * (128 << 10) + b"|the of and it. " * (56 << 10)
        assert len(text) == 1 << 20
        offs = np.asarray([0, 5, len(text) // 2 + 1, len(text)], dtype=np.int64)
        want = stt.expected_ids(text, offs, stt.literals("one_byte"), _port().encode)
        assert int((want[0] >= 200000).sum()) == (128 << 10) + (56 << 10)
        _same(t.encode_batch_with_special(text, offs, allowed), want, "1 MiB of candidates through td_encode_batch_with_special")
        _same(_Buffers(c.text, c.offs).run(t, allowed), _expected(k), "one_byte behind the fall-back")
    finally:
        t.close()


def test_a_literal_of_49_bytes_is_refused_by_the_device_entry(tok):
    text = b"x" + stt.TOO_LONG.encode() + b"y[INST]" + stt.TOO_LONG.encode()[:48] + b"z"
    offs = np.asarray([0, len(text)], dtype=np.int64)
    allowed = stt.allowed_ids("too_long")
    b = _Buffers(text, offs)
    b.ids.fill_(-1)
    b.toff.fill_(-1)
    with pytest.raises(capi.TokenDaggerHipError) as e:
        tok.encode_device_with_special(b.text_ptr, b.n, b.offs.data_ptr(), b.nd, allowed, b.ids.data_ptr(), b.cap, b.toff.data_ptr(), _stream())
    assert e.value.code == capi.TD_E_INVALID and "49 bytes long" in str(e.value) and "at most 48 bytes" in str(e.value)
    tok.device_status(_stream())
    assert bool((b.ids == -1).all().item()) and bool((b.toff == -1).all().item()), "the refused call wrote its outputs"
    want = stt.expected_ids(text, offs, stt.literals("too_long"), _port().encode)
    assert int((want[0] >= 200000).sum()) == 2
    _same(tok.encode_batch_with_special(text, offs, allowed), want, "the batch entry with a 49-byte literal")
    # the handle still searches on the device
    k = [i for i, c in enumerate(stt.calls()) if c.name == "alias"][0]
    c = stt.calls()[k]
    _same(_Buffers(c.text, c.offs).run(tok, stt.allowed_ids("alias")), _expected(k), "alias behind the refusal")


def test_a_generic_pattern_is_refused_by_the_device_entry():
    _, ranks = _ranks()
    t = capi.HipTokenizer(AUTOGEN, ranks, stt.vocabulary(), device=0)
    try:
        b = _Buffers(b"a[INST]b", [0, 8])
        with pytest.raises(capi.TokenDaggerHipError) as e:
            b.run(t, stt.allowed_ids("words"))
        assert e.value.code == TD_E_PATTERN and "td_encode_batch_with_special" in str(e.value)
    finally:
        t.close()
