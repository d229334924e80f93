"""Every encode repeats bit for bit, whatever the workspace held before it.

The step's kernels run on memory the allocator returned as it was: every word of it is either reset per call (td_prepare_mark) or
written before it is read ("Who writes the workspace first").  TD_OPT_WS_FILL makes a word nobody wrote read as a chosen
byte, at allocation and in front of every step, so that a read of unwritten memory gives a wrong answer HERE, every time, instead of
once in sixty runs somewhere else.  What is compared, everywhere: ids and document offsets against the compiled reference
(CoreBPE::encode, the reference's src/tiktoken/tiktoken.cpp:169-234, through oracle/_ref), bit for bit; the other pattern families
against the checker their own GPU tests use; the row, label, count, match and decode operations against their tests/*_truth.py.

Device-form calls write into outputs pre-filled with 0xFF bytes that lie inside larger tensors, 64 guard elements on either side,
which must stay untouched.  TD_OPT_SMALL_PATH is 0 unless a test says otherwise.  No case here makes the device fault or wait."""
from __future__ import annotations

import functools
import os
import random

import numpy as np
import pytest

import helpers as H
import td_corpus
from oracle import port, ref
from tokendagger_amd import capi, vocab_io

pytestmark = pytest.mark.gpu

GUARD = 64
FILLS = (0x00, 0xFF, 0xA5)
REPEATS = 5
REF_THREADS = min(16, os.cpu_count() or 1)
AUTOGEN = r"[a-zA-Z]+|\s+|[0-9]+|[^\w\s]"  # the reference tests' own pattern (tests/autogenned_test.py:66): a generic one
SWEEP_LENGTHS = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 4097)
CJK = "的一是不了人我在有他这为之大来以个中上们"

# name -> options set on a fresh clone (in this order).  TD_OPT_OVERLAP is 1 by default: "sparse0" turns it off so that the dense
# sequence runs in line there and on its second stream in "sparse0_overlap".
CONFIGS = {
    "default": {},
    "sparse1": {capi.TD_OPT_SPARSE: 1},
    "sparse0": {capi.TD_OPT_SPARSE: 0, capi.TD_OPT_OVERLAP: 0},
    "sparse0_overlap": {capi.TD_OPT_SPARSE: 0, capi.TD_OPT_OVERLAP: 1},
    "direct": {capi.TD_OPT_DIRECT: 1},
    "fused0": {capi.TD_OPT_FUSED: 0},
    "pack_split0": {capi.TD_OPT_PACK_SPLIT: 0},
    "dedupe0": {capi.TD_OPT_DEDUPE: 0},
    "giant_coop_1024": {capi.TD_OPT_GIANT_COOP_MIN: 1024},
    "graph": {capi.TD_OPT_GRAPH: 1},
    "ordinary": {},
}


# ---- inputs: built once, shared, left unchanged ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _seed_batches():
    """The document batches 0 and 1 of tests/test_gpu_char_seeds.py, drawn as they are drawn there -> [(runs, docs)] * 2."""
    rng = random.Random(17)
    out = []
    for _ in range(2):
        runs = H.char_seed_runs(rng, 1500)
        docs = []
        for i, r in enumerate(runs):
            sep = rng.choice(["", " ", "\n", "。", ", ", "x" * rng.randint(0, 5)])
            docs.append((r + sep).encode("utf-8") if i + 1 < len(runs) else r.encode("utf-8"))
        out.append((runs, docs))
    return out


def _long_sweep() -> bytes:
    """English filler around single pieces at the lengths where the step changes its path: the 64-byte window, the 256-byte halo, the
    1 KiB giant pieces, more than a tile; a letter piece and a digit run of 20 000 bytes; a piece across tiles; deferred tiles."""
    filler = td_corpus.english(160 << 10, seed=2)[0].tobytes()
    parts, at = [], 0

    def fill(n):
        nonlocal at
        parts.append(filler[at:at + n] + b" ")
        at += n
    for k, n in enumerate(SWEEP_LENGTHS):
        fill(5000)
        parts.append(bytes([97 + k]) * n + b" ")
    for k, n in enumerate(SWEEP_LENGTHS):
        fill(5000)
        parts.append((CJK[k] * n).encode("utf-8") + b" ")
    for big in (b"q" * 20000, b"7" * 20000, b"z" * 30000 + b"\n" * 9000, b"a.b.c.d." * 4000):
        fill(9000)
        parts.append(big + b" ")
    fill(8000)
    return b"".join(parts)


@functools.lru_cache(maxsize=None)
def _inputs():
    """name -> (text uint8[n], document offsets int64[n_docs + 1]); each well under 2 MiB."""
    out = {}
    docs = [d for _, ds in _seed_batches() for d in ds]
    text, offs = H.pack_docs(docs)
    out["seed_runs"] = (np.frombuffer(text, dtype=np.uint8), offs)
    sweep = _long_sweep()
    out["long_sweep"] = (np.frombuffer(sweep, dtype=np.uint8), np.asarray([0, len(sweep) // 3, len(sweep)], dtype=np.int64))
    for name, gen in (("mixed", td_corpus.mixed), ("english", td_corpus.english), ("code", td_corpus.code)):
        x, o = gen(1 << 20, seed=7)
        out[name] = (np.ascontiguousarray(x), np.asarray(o, dtype=np.int64))
    base = td_corpus.english(64 << 10, seed=11)[0]
    out["cut_docs"] = (np.ascontiguousarray(base[:40000]), np.arange(0, 40001, dtype=np.int64))  # one-byte documents
    out["cut_docs_empty"] = (np.ascontiguousarray(base[:20000]),
                             np.asarray([0, 0, 0, 5, 5, 8192, 8192, 8192 + 128, 20000, 20000], dtype=np.int64))
    for name, (x, o) in out.items():
        assert len(x) < (2 << 20) and o[0] == 0 and o[-1] == len(x), name
    return out


def _need_ref():
    assert ref.available(), "oracle/_ref/libtdref.so is missing: build it where /root/reference exists (oracle/build_ref.sh)"


@functools.lru_cache(maxsize=None)
def _reference(name: str, mode: int = capi.TD_MODE_ENCODE):
    """-> (ids int32, offsets int64) of the compiled reference: encode, or encode_ordinary document by document."""
    _need_ref()
    R = H.ref_tokenizer()
    x, o = _inputs()[name]
    if mode == capi.TD_MODE_ENCODE:
        _, ids, offs = R.encode_batch(x, o, n_threads=REF_THREADS, want_tokens=True)
        return ids.copy(), offs
    raw = x.tobytes()
    per = [R.encode_ordinary(raw[o[d]:o[d + 1]]) for d in range(len(o) - 1)]
    offs = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64)
    return (np.concatenate(per) if per else np.zeros(0, np.int32)).astype(np.int32), offs


# ---- the device form on guarded, 0xFF-filled outputs ------------------------------------------------------------------------------------

class _DeviceCase:
    """One input uploaded once, its reference beside it, and the guarded outputs of td_encode_device."""

    def __init__(self, x, o, want_ids, want_offs):
        import torch
        self.dev = torch.device("cuda", 0)
        self.n, self.n_docs, self.total = len(x), len(o) - 1, len(want_ids)
        self.cap = self.n + 64  # (at most one id per byte)
        self.d_text = torch.from_numpy(np.array(x, dtype=np.uint8)).to(self.dev)  # (a copy: the input may be read-only)
        self.d_offs = torch.from_numpy(np.ascontiguousarray(o, dtype=np.int64)).to(self.dev)
        self.want_ids = torch.from_numpy(np.ascontiguousarray(want_ids, dtype=np.int32)).to(self.dev)
        self.want_offs = torch.from_numpy(np.ascontiguousarray(want_offs, dtype=np.int64)).to(self.dev)
        self.ids = torch.empty(self.cap + 2 * GUARD, dtype=torch.int32, device=self.dev)
        self.offs = torch.empty(self.n_docs + 1 + 2 * GUARD, dtype=torch.int64, device=self.dev)

    def launch(self, tok, stream: int, mode: int = capi.TD_MODE_ENCODE):
        """(on the torch stream that is current: the fills of the outputs are ordered in front of the call)"""
        self.ids.fill_(-1)   # 0xFF bytes
        self.offs.fill_(-1)
        tok.encode_device(self.d_text.data_ptr(), self.n, self.d_offs.data_ptr(), self.n_docs, self.ids.data_ptr() + 4 * GUARD, self.cap,
                          self.offs.data_ptr() + 8 * GUARD, stream, mode=mode)

    def check(self, what):
        import torch
        g = GUARD
        guards = bool(((self.ids[:g] == -1).all() & (self.ids[g + self.cap:] == -1).all() & (self.offs[:g] == -1).all() &
                       (self.offs[g + self.n_docs + 1:] == -1).all()).item())
        assert guards, f"{what}: the guard elements around the outputs were written"
        got_offs = self.offs[g:g + self.n_docs + 1]
        if not torch.equal(got_offs, self.want_offs):
            bad = torch.nonzero(got_offs != self.want_offs)[:1].cpu().numpy().reshape(-1)
            d = int(bad[0])
            raise AssertionError(f"{what}: document offsets differ from the reference, first at document {d}: "
                                 f"{int(got_offs[d].item())} != {int(self.want_offs[d].item())} (total {int(got_offs[-1].item())} != {self.total})")
        got_ids = self.ids[g:g + self.total]
        if not torch.equal(got_ids, self.want_ids):
            bad = torch.nonzero(got_ids != self.want_ids).cpu().numpy().reshape(-1)
            raise AssertionError(f"{what}: {len(bad)} ids differ from the reference, first at token {int(bad[0])}")


@functools.lru_cache(maxsize=None)
def _device_case(name: str, mode: int = capi.TD_MODE_ENCODE) -> _DeviceCase:
    x, o = _inputs()[name]
    return _DeviceCase(x, o, *_reference(name, mode))


def _stream() -> int:
    import torch
    return torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream


@pytest.fixture(scope="module")
def base():
    """The Llama-4 handle every test clones (td_clone copies the options): the one-launch small path off, no fill."""
    pat, mr, special = H.llama4()
    t = capi.HipTokenizer(pat, mr, special, device=0)
    t.set_option(capi.TD_OPT_SMALL_PATH, 0)
    yield t
    t.close()


def _clone(base, fill: int = -1, options=None):
    base.set_option(capi.TD_OPT_WS_FILL, fill)  # (the clone is filled from its first allocation on)
    try:
        t = base.clone()
    finally:
        base.set_option(capi.TD_OPT_WS_FILL, -1)
    for what, value in (options or {}).items():
        t.set_option(what, value)
    return t


def _filled(t) -> int:
    return t.info(capi.TD_INFO_WS_FILLED_BYTES)


# ---- poisoned steps ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("config", list(CONFIGS))
def test_poisoned_steps_equal_the_reference(base, config):
    """Every input under one configuration, under each fill byte, five times in a row on one handle: every repeat equals the reference
    and has filled the workspace in front of its step (stage and stage2 alone are 2 x 4160 x 4 bytes per 4096 bytes of text)."""
    mode = capi.TD_MODE_ORDINARY if config == "ordinary" else capi.TD_MODE_ENCODE
    s = _stream()
    for fill in FILLS:
        t = _clone(base, fill, CONFIGS[config])
        try:
            assert _filled(t) > 0, "the clone's first allocation was not filled"
            for name in _inputs():
                c = _device_case(name, mode)
                for rep in range(REPEATS):
                    before = _filled(t)
                    c.launch(t, s, mode)
                    t.device_status(s)  # (reads the counters: the next call may choose the sparse sequence / the second stream by them)
                    c.check(f"{config}, fill 0x{fill:02X}, {name}, repeat {rep}")
                    grown = _filled(t) - before
                    assert grown >= 8 * c.n, f"{config}, fill 0x{fill:02X}, {name}, repeat {rep}: only {grown} bytes filled for {c.n} bytes of text"
                if name == "seed_runs" and config == "sparse0_overlap":
                    assert t.info(capi.TD_INFO_LONG_PIECES) >= 2048, "too few long pieces for the second stream to run"
                    assert t.info(capi.TD_INFO_SPARSE) == 0
                if config == "sparse1":
                    assert t.info(capi.TD_INFO_SPARSE) == 1
        finally:
            t.close()


# ---- what the last call left, fill off -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("config", ["default", "sparse1", "sparse0"])
def test_a_call_on_the_workspace_another_input_left_equals_the_reference(base, config):
    """One handle, no fill: mixed, then seed_runs, then long_sweep, then english, each on what its predecessor left behind."""
    s = _stream()
    t = _clone(base, -1, CONFIGS[config])
    try:
        for name in ("mixed", "seed_runs", "long_sweep", "english"):
            c = _device_case(name)
            c.launch(t, s)
            t.device_status(s)
            c.check(f"{config}: {name} behind the previous input")
        assert _filled(t) == 0
    finally:
        t.close()


# ---- the first call of a fresh handle ----------------------------------------------------------------------------------------------------

def test_first_host_call_of_fifty_fresh_handles(base):
    """The call that once gave 15 ids too many ("What's weak" 2): td_encode_batch of the seeded runs as the FIRST call
    of a handle, here on 50 fresh clones with the fill rotating over the three bytes."""
    x, o = _inputs()["seed_runs"]
    want_ids, want_offs = _reference("seed_runs")
    for k in range(50):
        fill = FILLS[k % 3]
        t = _clone(base, fill)
        try:
            ids, offs = t.encode_batch(x, o)
            assert np.array_equal(offs, want_offs), f"clone {k}, fill 0x{fill:02X}: document offsets differ from the reference ({offs[-1]} != {want_offs[-1]} ids)"
            bad = np.flatnonzero(ids != want_ids)
            assert bad.size == 0, f"clone {k}, fill 0x{fill:02X}: ids differ from the reference, first at token {int(bad[0])}"
            assert _filled(t) >= 8 * len(x)
        finally:
            t.close()


def test_first_single_calls_of_fifty_fresh_handles_with_the_small_path(base):
    """The same with TD_OPT_SMALL_PATH 1: the first 40 runs one by one through encode() (the one-launch kernel hands a piece above
    64 bytes back to the general path)."""
    _need_ref()
    R = H.ref_tokenizer()
    runs = [r.encode("utf-8") for r in _seed_batches()[0][0][:40]]
    want = [R.encode(b) for b in runs]
    for k in range(50):
        fill = FILLS[k % 3]
        t = _clone(base, fill, {capi.TD_OPT_SMALL_PATH: 1})
        try:
            for i, b in enumerate(runs):
                assert np.array_equal(t.encode(b), want[i]), f"clone {k}, fill 0x{fill:02X}: run {i} differs from the reference"
        finally:
            t.close()


# ---- two clones, two streams ---------------------------------------------------------------------------------------------------------------

def test_two_poisoned_clones_on_two_streams(base):
    import torch
    dev = torch.device("cuda", 0)
    a, b = _clone(base, 0xFF), _clone(base, 0xA5)
    ca, cb = _device_case("mixed"), _device_case("seed_runs")
    sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    try:
        for rnd in range(10):
            with torch.cuda.stream(sa):
                ca.launch(a, sa.cuda_stream)
            with torch.cuda.stream(sb):
                cb.launch(b, sb.cuda_stream)
            a.device_status(sa.cuda_stream)
            b.device_status(sb.cuda_stream)
            ca.check(f"mixed on the first clone, round {rnd}")
            cb.check(f"seed_runs on the second clone, round {rnd}")
    finally:
        torch.cuda.synchronize(dev)
        a.close()
        b.close()


# ---- the other pattern families under the launch configurations -------------------------------------------------------------------------

def _family_text():
    """The documents of `mixed` that end inside its first 256 KiB, then long_sweep's."""
    x, o = _inputs()["mixed"]
    o = o[o <= (256 << 10)]
    sx, so = _inputs()["long_sweep"]
    text = np.concatenate([x[:o[-1]], sx])
    return text, np.concatenate([o, so[1:] + o[-1]]).astype(np.int64)


FAMILIES = {  # name -> (pattern, the checker its own GPU test uses)
    "tekken": (H.TEKKEN_PAT, lambda mr, sp: H.port_tokenizer_tekken()),
    "cl100k": (H.CL100K_PAT, lambda mr, sp: H.port_tokenizer_cl100k()),
    "cl100k_current": (vocab_io.CL100K_PAT_STR_CURRENT, lambda mr, sp: port.OracleTokenizer(mr, port.VARIANT_CL100K_EOS)),
    "qwen2": (vocab_io.QWEN2_PAT_STR, lambda mr, sp: port.OracleTokenizer(mr, port.VARIANT_QWEN2)),
    "gpt2": (H.GPT2_PAT, lambda mr, sp: H.port_tokenizer_gpt2()),
    "generic": (AUTOGEN, None),  # the compiled reference with that very pattern
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_pattern_families_poisoned_under_the_launch_configurations(family):
    _need_ref()
    _, mr, special = H.llama4()
    pat, checker = FAMILIES[family]
    text, offs = _family_text()
    if checker is None:
        _, want_ids, want_offs = ref.RefTokenizer(pat, mr, special).encode_batch(text, offs, n_threads=REF_THREADS, want_tokens=True)
    else:
        want_ids, want_offs = checker(mr, special).encode_batch(text.tobytes(), offs)
    c = _DeviceCase(text, offs, want_ids, want_offs)
    s = _stream()
    t0 = capi.HipTokenizer(pat, mr, special, device=0)
    t0.set_option(capi.TD_OPT_SMALL_PATH, 0)
    try:
        # (a generic pattern has one launch sequence: the library turns the fused loop, direct placement and the sparse sequence off for it)
        for config in (("default",) if family == "generic" else ("default", "sparse1", "direct", "fused0")):
            t = _clone(t0, 0xFF, CONFIGS[config])
            try:
                for rep in range(3):
                    before = _filled(t)
                    c.launch(t, s)
                    t.device_status(s)
                    c.check(f"{family}, {config}, repeat {rep}")
                    assert _filled(t) - before >= 8 * c.n
            finally:
                t.close()
    finally:
        t0.close()


# ---- the other operations on buffers filled at their allocation ------------------------------------------------------------------------
# Each takes a case of its truth module at one of two sizes, runs the host form (whose every device buffer the handle allocates) and
# compares every output with the truth.

BOS, EOS, PAD = 200000, 200001, -5


def _same(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        if g is None or w is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and np.array_equal(g, w), (what, k)


def _ids_case(big: bool, seed: int):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 400 if big else 40, 300 if big else 25)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return rng.integers(0, 200000, int(offs[-1])).astype(np.int32), offs


def _op_concat_rows(t, big, what):
    import rows_truth as rt
    ids, offs = _ids_case(big, 1)
    S = 128 if big else 7
    _same(t.make_rows(ids, offs, capi.rows_spec(S, rt.CONCAT, BOS, EOS, PAD, False), positions=True, aux=True),
          rt.rows_numpy(ids, offs, S, rt.CONCAT, BOS, EOS, PAD, False), what)


def _op_pack_rows(t, big, what):
    import pack_truth as pt
    ids, offs = _ids_case(big, 2)
    S = 512 if big else 19
    _same(t.pack_rows(ids, offs, capi.pack_spec(S, BOS, EOS, PAD, False), positions=True, lengths=True, docs=True),
          pt.pack_runs(ids, offs, S, BOS, EOS, PAD, False), what)


def _op_window_rows(t, big, what):
    import windows_truth as wt
    ids, offs = _ids_case(big, 3)
    S, overlap = (128, 32) if big else (9, 2)
    _same(t.window_rows(ids, offs, capi.windows_spec(S, BOS, EOS, PAD), overlap, positions=True, lengths=True, docs=True, starts=True),
          wt.windows_numpy(ids, offs, S, overlap, BOS, EOS, PAD), what)


def _op_span_labels(t, big, what):
    import labels_truth as lt
    ids, offs, open, close, tc = lt.random_case(np.random.default_rng(4), max_docs=300 if big else 12)
    _same(t.span_labels(ids, offs, capi.labels_spec(open, close, -100, tc), mask=True, trained_offsets=True),
          lt.labels_numpy(ids, offs, open, close, -100, tc), what)


@functools.lru_cache(maxsize=None)
def _id_lengths():
    import offsets_truth as OT
    _, mr, special = H.llama4()
    lengths = OT.id_lengths(OT.id_bytes(mr, special))
    pool = []
    for k in range(1, 13):
        pool += np.flatnonzero(lengths == k)[:3].tolist()
    return lengths, np.asarray(pool, dtype=np.int32)


def _op_range_labels(t, big, what):
    import ranges_truth as rt
    lengths, pool = _id_lengths()
    ids, offs, ro, rg = rt.random_case(np.random.default_rng(5), lengths, pool, max_docs=300 if big else 12)
    _same(t.range_labels(ids, offs, (ro, rg), capi.range_spec("overlap", -100), mask=True, trained_offsets=True),
          rt.ranges_numpy(ids, offs, ro, rg, lengths, "overlap", -100, None), what)


def _op_select(t, big, what):
    import select_truth as st
    ids, labels, offs, sel, mn, mx = st.random_case(np.random.default_rng(6), max_docs=300 if big else 30)
    _same(t.select_docs(ids, offs, sel, capi.select_spec(mn, mx), labels=labels, docs=True),
          st.select_numpy(ids, offs, sel, mn, mx, labels=labels), what)


def _op_token_counts(t, big, what):
    import counts_truth as ct
    if big:
        ids, offs, groups, n_bins, n_groups = ct.border_documents()
    else:
        ids, offs = _ids_case(False, 7)
        ids, groups, n_bins, n_groups = ids % 320 - 10, (np.arange(len(offs) - 1) % 3).astype(np.int32), 300, 3  # (negative and too large values too)
    got = t.token_counts(ids, offs, groups, capi.counts_spec(n_bins, n_groups))
    _same(got, ct.counts_numpy(ids, n_bins, offs, groups, n_groups), what)


def _op_ngram_matches(t, big, what):
    import ngram_truth as nt
    rng = np.random.default_rng(8)
    c = nt.sparse(rng) if big else nt.dense(rng, total=700, n_docs=9)
    with t.ngram_set(c["seqs"]) as nset:
        got = t.ngram_matches(nset, c["ids"], c["offs"], labels=c["ids"], pattern_counts=True)
    nt.same(got, nt.matches_numpy(c["seqs"], c["ids"], c["offs"], labels=c["ids"]), what)


@functools.lru_cache(maxsize=None)
def _decode_vocab():
    import decode_rows_truth as dt
    _, mr, _ = H.llama4()
    return dt.Vocab({r: b for b, r in mr.items()})


def _token_ids(big: bool):
    """Ids of real tokens: the reference's ids of the first 24 (2) documents of `code`."""
    ids, offs = _reference("code")
    offs = offs[:25 if big else 3]
    assert len(offs) > 2 and offs[-1] > (40000 if big else 1000)
    return ids[:offs[-1]], offs


def _op_decode_rows(t, big, what):
    import decode_rows_truth as dt
    ids, offs = _token_ids(big)
    want = dt.decode_numpy(ids, _decode_vocab(), tok_offsets=offs)
    got = t.decode_rows(ids, capi.decode_spec(0, (), ()), tok_offsets=offs)
    assert got[0] == want[0], what
    _same(got[1:4], want[1:4], what)


def _op_token_starts(t, big, what):
    import offsets_truth as OT
    ids, offs = _token_ids(big)
    assert np.array_equal(t.token_starts(ids, offs, capi.TD_UNIT_BYTES), OT.covered_byte_starts(ids, offs, _id_lengths()[0])), what


def _op_decode_device(t, big, what):
    import torch
    import decode_rows_truth as dt
    ids, _ = _token_ids(big)
    want = dt.decode_numpy(ids, _decode_vocab(), tok_offsets=np.asarray([0, len(ids)], dtype=np.int64))[0]
    dev = torch.device("cuda", 0)
    d_ids = torch.from_numpy(np.ascontiguousarray(ids)).to(dev)
    out = torch.full((len(want) + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    nb = torch.full((1 + 2 * GUARD,), -1, dtype=torch.int64, device=dev)
    s = _stream()
    t.decode_device(d_ids.data_ptr(), len(ids), out.data_ptr() + GUARD, len(want), nb.data_ptr() + 8 * GUARD, s)
    t.device_status(s)
    o, n = out.cpu().numpy(), nb.cpu().numpy()
    assert int(n[GUARD]) == len(want) and o[GUARD:GUARD + len(want)].tobytes() == want, what
    assert (o[:GUARD] == 0xFF).all() and (o[GUARD + len(want):] == 0xFF).all() and (n[:GUARD] == -1).all() and (n[GUARD + 1:] == -1).all(), what


OPERATIONS = {"concat_rows": _op_concat_rows, "pack_rows": _op_pack_rows, "window_rows": _op_window_rows, "span_labels": _op_span_labels,
              "range_labels": _op_range_labels, "select": _op_select, "token_counts": _op_token_counts, "ngram_matches": _op_ngram_matches,
              "decode_rows": _op_decode_rows, "token_starts": _op_token_starts, "decode_device": _op_decode_device}


@pytest.mark.parametrize("op", list(OPERATIONS))
def test_other_operations_on_buffers_filled_at_birth(base, op):
    """As the FIRST call of a fresh clone under fill 0xFF and under 0x00, then once more behind a call of another size."""
    run = OPERATIONS[op]
    for fill in (0xFF, 0x00):
        t = _clone(base, fill)
        try:
            birth = _filled(t)
            run(t, False, f"{op}, fill 0x{fill:02X}, first call")
            assert _filled(t) > birth, f"{op}: none of its buffers went through the filled allocation"
            run(t, True, f"{op}, fill 0x{fill:02X}, the larger case")
            run(t, False, f"{op}, fill 0x{fill:02X}, behind the larger case")
        finally:
            t.close()


# ---- the switch itself ----------------------------------------------------------------------------------------------------------------------

def test_the_switch(base):
    s = _stream()
    c = _device_case("cut_docs_empty")
    for bad in (-2, 256, 1 << 20):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            base.set_option(capi.TD_OPT_WS_FILL, bad)
        assert e.value.code == capi.TD_E_INVALID
    off = _clone(base, -1)
    on = _clone(base, 0xA5)
    child = on.clone()  # (inherits the byte)
    try:
        assert _filled(off) == 0
        c.launch(off, s)
        off.device_status(s)
        c.check("fill off")
        assert _filled(off) == 0, "fill off: the counter moved"
        for name, t in (("the clone", on), ("the clone's clone", child)):
            birth = _filled(t)
            assert birth >= 256, f"{name}: its control block was not filled at birth"
            c.launch(t, s)
            t.device_status(s)
            c.check(name)
            first = _filled(t) - birth
            c.launch(t, s)
            t.device_status(s)
            second = _filled(t) - birth - first
            # the first call allocates (filled once at birth) and fills in front of its step; the second only the latter
            assert first > second >= 8 * c.n, (name, first, second)
        on.set_option(capi.TD_OPT_WS_FILL, -1)
        before = _filled(on)
        c.launch(on, s)
        on.device_status(s)
        c.check("switched off again")
        assert _filled(on) == before
    finally:
        for t in (off, on, child):
            t.close()
    # the environment's twin, read by td_create: the handle's own first allocation is filled
    pat, mr, special = H.llama4()
    old = os.environ.get("TD_WS_FILL")
    os.environ["TD_WS_FILL"] = "165"
    try:
        t = capi.HipTokenizer(pat, mr, special, device=0)
    finally:
        if old is None:
            del os.environ["TD_WS_FILL"]
        else:
            os.environ["TD_WS_FILL"] = old
    try:
        assert _filled(t) >= 256
        t.set_option(capi.TD_OPT_SMALL_PATH, 0)
        c.launch(t, s)
        t.device_status(s)
        c.check("TD_WS_FILL=165")
    finally:
        t.close()
