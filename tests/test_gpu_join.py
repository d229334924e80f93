"""Field joins on the GPU (td_join_fields, td_join_fields_device, td_encode_batch_join, the Python methods) against the truth of
tests/join_truth.py.  All comparisons are exact.  No case here makes the device fault: every error is one the library reports by
a status code."""
import ctypes

import numpy as np
import pytest

import helpers as H
import join_truth as jt
import labeled_rows_truth as lr

pytestmark = pytest.mark.gpu

BOS, EOS, SEP, PAD = 200000, 200001, 7, 3  # Llama-4 <|begin_of_text|>, <|end_of_text|>; an ordinary id; any int32
TILE = 4096                # output slots a workgroup writes per tile
CHUNK, PASS = 1024, 1024   # examples per chunk of the scan, chunks per pass of the chunk scan
LDS_DOCS = 4352            # offsets of a tile's examples kept in LDS
LIT_POOL = list(range(1, 900)) + [BOS, EOS]
NAMES = ("ids", "labels", "types", "offsets", "examples", "field_len", "counts")


@pytest.fixture(scope="module")
def tok():
    from tokendagger_amd import capi
    pat, mr, special = H.llama4()
    return capi.HipTokenizer(pat, mr, special, device=0)


def _check(tok, ids, offs, join, truth=jt.join_numpy, t=None, labels=True, types=True, examples=True, field_len=True):
    t = t if t is not None else truth(ids, offs, join)
    g = tok.join_fields(ids, offs, jt.capi_spec(join), labels=labels, types=types, examples=examples, field_len=field_len)
    want = dict(zip(NAMES, (True, labels, types, True, examples, field_len, True)))
    assert np.array_equal(g[6], t[6]), (g[6], t[6])
    for name, a, b in zip(NAMES, g, t):
        if not want[name]:
            assert a is None, name
        else:
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), name
    return t


def _case(rng, L, join, hi=200000):
    """ids and offsets for the field lengths L[n_ex, K], laid out the way `join` reads them."""
    L = np.asarray(L, np.int64).reshape(-1, len(join["fields"]))
    lengths = (L.T if join["field_major"] else L).reshape(-1)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return rng.integers(0, hi, int(offs[-1])).astype(np.int32), offs


def _sft(max_total=-1, shrink="order", field_major=False, completion_rank=2):
    return jt.make_join([jt.field([BOS], rank=1, keep_tail=True, type=0), jt.field([SEP], rank=completion_rank, train=True, type=1)],
                        tail=[EOS], tail_type=1, train_tail=True, max_total=max_total, shrink=shrink, field_major=field_major)


def test_small_cases_against_brute_force(tok):
    rng = np.random.default_rng(5)
    for it in range(64):
        ids, offs, join = jt.random_case(rng, K=(1 if it % 16 == 0 else 8 if it % 16 == 1 else None), lit_pool=LIT_POOL)
        _check(tok, ids, offs, join, truth=jt.join_brute, labels=bool(it & 1), types=bool(it & 2), examples=bool(it & 4), field_len=bool(it & 8))


def test_scan_borders(tok):
    rng = np.random.default_rng(6)
    for n_ex in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        for shrink in ("order", "longest"):
            join = _sft(9, shrink, completion_rank=0)  # bodies of at most 6 ids; a completion above that is dropped
            ids, offs = _case(rng, rng.integers(0, 9, (n_ex, 2)), join)
            t = _check(tok, ids, offs, join)
            assert n_ex < 2 or (t[6][0] > 0 and t[6][2] > 0 and t[6][3] > 0)
    # the last example alone is kept
    join = jt.make_join([jt.field(max_len=-1)], max_total=0)
    ids, offs = _case(rng, np.concatenate([rng.integers(1, 4, 3000), [0]]), join)
    t = _check(tok, ids, offs, join)
    assert t[6].tolist() == [1, 0, 3000, 0] and t[4].tolist() == [3000]


def test_more_examples_than_one_pass_of_the_chunk_scan(tok):
    rng = np.random.default_rng(7)
    n_ex = CHUNK * PASS + 5
    join = jt.make_join([jt.field(train=True)], max_total=1)  # one-id fields; the two-id ones do not fit and nothing may be cut
    ids, offs = _case(rng, rng.integers(0, 3, n_ex), join)
    t = _check(tok, ids, offs, join, types=False, field_len=False)
    assert t[6][0] > 600000 and t[6][2] > 300000 and t[6][1] > 300000


def _lengths_at_borders():
    """Field lengths [n, 2] for the join _sft (BOS body_0 SEP body_1 EOS): examples of 4095, 4096, 4097 and 9000 slots, then
    examples whose first slot (BOS), body_0's first id, body_0's end (SEP) and the tail each lie 1, 2 and 3 slots before a tile
    border (a filler example in front of each)."""
    rows, at = [], 0
    for n in (4095, 4096, 4097, 9000):
        rows.append([n - 3 - 40, 40])
        at += n
    a, b = 5, 6  # the placed example: BOS at 0, body_0 at 1, SEP at 1 + a, body_1 behind it, EOS at 2 + a + b
    for mark in (0, 1, 1 + a, 2 + a + b):
        for before in (1, 2, 3):
            filler = (TILE - before - mark - at) % TILE
            filler += TILE if filler < 3 else 0  # (an example has its three literals)
            rows.append([filler - 3, 0])
            at += filler
            assert (at + mark) % TILE == TILE - before
            rows.append([a, b])
            at += 3 + a + b
    return np.array(rows, np.int64)


def test_tile_borders_and_alignments(tok):
    rng = np.random.default_rng(8)
    L = _lengths_at_borders()
    for field_major in (False, True):
        join = _sft(field_major=field_major)
        ids, offs = _case(rng, L, join)
        t = _check(tok, ids, offs, join)
        assert np.diff(t[3])[:4].tolist() == [4095, 4096, 4097, 9000]
    # the same examples cut at the front of the prompt and the end of the completion: the sources move, the borders too
    for shrink in ("order", "longest"):
        join = _sft(4000, shrink)
        ids, offs = _case(rng, L, join)
        t = _check(tok, ids, offs, join)
        assert t[6][3] >= 4
    # every residue mod 4 of a body's source against its destination: field-major, the first example's lengths move field 0's
    # sources by s0, field 1's by s1 and every destination by s0 + s1
    tail = L[4:]
    for s0 in range(4):
        for s1 in range(4):
            join = _sft(field_major=True)
            ids, offs = _case(rng, np.concatenate([[[s0, s1]], tail]), join)
            _check(tok, ids, offs, join, types=bool(s0 & 1), field_len=False)


def test_runs_of_empty_examples(tok):
    rng = np.random.default_rng(9)
    plain = jt.make_join([jt.field(train=True, type=4)])
    two = jt.make_join([jt.field(rank=1), jt.field(train=True, type=1)], max_total=5000)
    # more kept empty examples between two non-empty ones than LDS holds, just as many, fewer; all inside one tile, and across tiles
    for empties, a, b in ((5000, 10, 10), (4000, 3, 5), (5000, 5000, 4097), (LDS_DOCS - 1, 1, 1), (LDS_DOCS, 1, 1), (LDS_DOCS + 1, 1, 1)):
        ids, offs = _case(rng, [a] + [0] * empties + [b], plain)
        t = _check(tok, ids, offs, plain)
        assert t[6].tolist() == [empties + 2, a + b, 0, 0]
        ids, offs = _case(rng, [[a, 1]] + [[0, 0]] * empties + [[1, b]], two)
        t = _check(tok, ids, offs, two)
        assert t[6][0] == empties + 2 and t[6][2] == 0
    ids, offs = _case(rng, [0] * 3000 + [7] + [0] * 6000 + [4096, 1] + [0] * 5000, plain)  # empty runs at both ends and in between
    _check(tok, ids, offs, plain)
    t = _check(tok, np.zeros(0, np.int32), np.zeros(5, np.int64), two)  # two examples, all empty
    assert t[6].tolist() == [2, 0, 0, 0] and t[3].tolist() == [0, 0, 0]
    t = _check(tok, np.zeros(0, np.int32), np.zeros(1, np.int64), two)  # no documents
    assert t[6].tolist() == [0, 0, 0, 0] and t[3].tolist() == [0]


def test_field_counts(tok, golden):
    ids, offs = golden["enc"], golden["enc_offsets"]
    # K = 1 without literals is the selection with the identity list
    join = jt.make_join([jt.field(train=True)])
    g = tok.join_fields(ids, offs, jt.capi_spec(join))
    s = tok.select_docs(ids, offs, None, labels=ids)
    assert np.array_equal(g[0], s[0]) and np.array_equal(g[1], s[1]) and np.array_equal(g[3], s[2]) and np.array_equal(g[4], s[3])
    assert np.array_equal(g[0], ids) and np.array_equal(g[3], offs) and g[6].tolist() == [len(offs) - 1, len(ids), 0, 0]
    # K = 8, all 17 literal places full
    rng = np.random.default_rng(10)
    lit = lambda: rng.choice(LIT_POOL, 16).tolist()
    for shrink in ("order", "longest"):
        fs = [jt.field(lit(), rank=int(rng.integers(0, 3)), type=f, keep_tail=bool(f & 1), train=bool(f & 2), train_before=bool(f & 4)) for f in range(8)]
        join = jt.make_join(fs, lit(), tail_type=9, train_tail=True, max_total=17 * 16 + 200, shrink=shrink, field_major=shrink == "longest")
        ids8, offs8 = _case(rng, rng.integers(0, 80, (300, 8)), join)
        t = _check(tok, ids8, offs8, join)
        assert t[6][0] > 0 and t[6][3] > 0
        assert (np.diff(t[3]) >= 17 * 16).all()


@pytest.mark.parametrize("K", (2, 3))
def test_golden_ids(tok, golden, K):
    ids, offs = golden["enc"], golden["enc_offsets"]
    n_ex = (len(offs) - 1) // K
    offs = offs[:n_ex * K + 1]
    ids = ids[:offs[-1]]
    assert n_ex > CHUNK and len(ids) > 50 * TILE
    fs = [jt.field([BOS], rank=1, keep_tail=True), jt.field([SEP], rank=1, type=1)][:K - 1] + [jt.field([SEP], rank=0, train=True, type=2)]
    med = int(np.median(np.diff(jt.join_numpy(ids, offs, jt.make_join(fs, [EOS]))[3])))
    for shrink in ("order", "longest"):
        for field_major in (False, True):
            join = jt.make_join(fs, [EOS], tail_type=2, train_tail=True, max_total=med, shrink=shrink, field_major=field_major)
            t = _check(tok, ids, offs, join)
            assert t[6][0] > 0 and t[6][2] > 0 and t[6][3] > 0  # kept, dropped and truncated are all there
            assert t[6][0] - t[6][3] > 0 and np.diff(t[3]).max() == med


def test_composition_with_the_labeled_row_layouts(tok, golden):
    from tokendagger_amd import capi
    ids, offs = golden["enc"], golden["enc_offsets"]
    n_ex = (len(offs) - 1) // 2
    offs = offs[:2 * n_ex + 1]
    join = _sft(300)
    t = jt.join_numpy(ids, offs, join)
    j_ids, j_lab, _, j_offs, _, _, _ = tok.join_fields(ids, offs, jt.capi_spec(join))
    S = 128
    kw = dict(bos=False, eos=False, pad_value=-100)
    lab = capi.rows_labels(0, 0, -100, -100, -100)
    got = tok.make_rows_labeled(j_ids, j_lab, j_offs, capi.rows_spec(S, capi.TD_ROWS_PAD, -1, -1, PAD), lab)
    assert np.array_equal(got[0], lr.id_rows("pad", t[0], t[3], S, pad=PAD)[0])
    assert np.array_equal(got[-1], lr.label_rows("pad", t[1], t[3], S, **kw))
    got = tok.pack_rows_labeled(j_ids, j_lab, j_offs, capi.pack_spec(S, -1, -1, PAD), lab)
    assert np.array_equal(got[0], lr.id_rows("bestfit", t[0], t[3], S, pad=PAD)[0])
    assert np.array_equal(got[-1], lr.label_rows("bestfit", t[1], t[3], S, **kw))
    got = tok.window_rows_labeled(j_ids, j_lab, j_offs, capi.windows_spec(S, -1, -1, PAD), lab, 16)
    assert np.array_equal(got[0], lr.id_rows("windows", t[0], t[3], S, pad=PAD, overlap=16)[0])
    assert np.array_equal(got[-1], lr.label_rows("windows", t[1], t[3], S, overlap=16, **kw))


def _device_call(tok, ids, offs, join, cap, n_tokens=None, fill=77, stream=None, want=(True, True, True, True), spec=None):
    import torch
    dev = torch.device("cuda", 0)
    K = len(join["fields"])
    n_docs = len(offs) - 1
    n_ex = n_docs // K
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream(dev)):
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        d_ids, d_offs = up(ids, np.int32), up(offs, np.int64)
        full = lambda n, dt: torch.full((max(n, 1),), fill, dtype=dt, device=dev)
        bufs = {"ids": full(cap, torch.int32), "labels": full(cap, torch.int32), "types": full(cap, torch.int32),
                "offsets": full(n_ex + 1, torch.int64), "examples": full(n_ex, torch.int64), "field_len": full(n_ex * K, torch.int32)}
        counts = torch.full((4,), fill, dtype=torch.int64, device=dev)
    s = (stream if stream is not None else torch.cuda.current_stream(dev)).cuda_stream
    p = lambda name, on: bufs[name].data_ptr() if on else 0
    tok.join_fields_device(d_ids.data_ptr() if len(ids) else 0, len(ids) if n_tokens is None else n_tokens, d_offs.data_ptr(), n_docs,
                           spec if spec is not None else jt.capi_spec(join), bufs["ids"].data_ptr(), cap, bufs["offsets"].data_ptr(),
                           counts.data_ptr(), p("labels", want[0]), p("types", want[1]), p("examples", want[2]), p("field_len", want[3]), s)
    return bufs, counts, s, (d_ids, d_offs)


def _untouched(bufs, fill=77):
    return all((b == fill).all().item() for b in bufs.values())


def _golden_pairs(golden, n=60000):
    ids, offs = golden["enc"][:n], golden["enc_offsets"]
    offs = offs[:int(np.searchsorted(offs, n, side="right"))]
    offs = offs[:(len(offs) - 1) // 2 * 2 + 1].astype(np.int64)
    return ids[:offs[-1]], offs


def test_device_form_on_a_side_stream_and_on_poisoned_workspaces(tok, golden):
    import torch
    from tokendagger_amd import capi
    ids, offs = _golden_pairs(golden)
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    for join, want in ((_sft(250, "longest"), (True, True, True, True)), (_sft(250, "order", completion_rank=0), (True, False, False, True)),
                       (_sft(), (False, True, True, False))):
        t = jt.join_numpy(ids, offs, join)
        E, T = int(t[6][0]), int(t[6][1])
        sizes = {"ids": T, "labels": T if want[0] else 0, "types": T if want[1] else 0, "offsets": E + 1, "examples": E if want[2] else 0,
                 "field_len": 2 * E if want[3] else 0}
        ref = dict(zip(NAMES, t))
        runs = []
        for fill in (-1, 0x5A, 0xFF):  # a handle of its own each: its workspace is filled from its first allocation on
            tok.set_option(capi.TD_OPT_WS_FILL, fill)
            try:
                h = tok.clone()
            finally:
                tok.set_option(capi.TD_OPT_WS_FILL, -1)
            bufs, counts, s, keep = _device_call(h, ids, offs, join, T + 5, stream=side, want=want)
            h.device_status(s)
            assert np.array_equal(counts.cpu().numpy(), t[6])
            got = {k: b.cpu().numpy() for k, b in bufs.items()}
            for k, n in sizes.items():
                assert n == 0 or np.array_equal(got[k][:n], ref[k].reshape(-1)), (fill, k)
                assert (got[k][n:] == 77).all(), (fill, k)
            runs.append({k: got[k].tobytes() for k in got} | {"counts": counts.cpu().numpy().tobytes()})
            h.close()
        assert runs[0] == runs[1] == runs[2]


def test_errors_host_and_device(tok, golden):
    from tokendagger_amd import capi
    ids, offs = _golden_pairs(golden, 50000)
    n_docs = len(offs) - 1
    join = _sft(200)
    sp = jt.capi_spec(join)
    t = jt.join_numpy(ids, offs, join)
    T = int(t[6][1])

    def good_call_follows():  # the next good call on the same handle
        bufs, counts, stream, _ = _device_call(tok, ids, offs, join, T)
        tok.device_status(stream)
        assert np.array_equal(counts.cpu().numpy(), t[6]) and np.array_equal(bufs["ids"].cpu().numpy()[:T], t[0])
        assert np.array_equal(bufs["labels"].cpu().numpy()[:T], t[1]) and np.array_equal(bufs["types"].cpu().numpy()[:T], t[2])

    # capacity one below T
    with pytest.raises(capi.TokenDaggerHipError) as ei:
        tok.join_fields(ids, offs, sp, ids_capacity=T - 1)
    assert ei.value.code == capi.TD_E_CAPACITY and ei.value.counts[1] == T
    bufs, counts, stream, _ = _device_call(tok, ids, offs, join, T - 1)
    rc, where = tok.device_status_pos(stream)
    assert rc == capi.TD_E_CAPACITY and where == T
    assert counts.cpu().tolist()[1] == T and _untouched(bufs)
    tok.device_status(stream)  # (cleared)
    good_call_follows()
    # offsets: a decreasing pair inside a document, and n_tokens below the last offset: the position is the example
    d = 1 + int(np.flatnonzero(np.diff(offs[1:]) > 0)[0])  # document d is not empty
    dec = offs.copy()
    dec[d], dec[d + 1] = offs[d + 1], offs[d]              # documents d - 1 and d + 1 grow, d decreases
    bufs, counts, stream, _ = _device_call(tok, ids, dec, join, 2 * len(ids) + 3 * n_docs)
    rc, where = tok.device_status_pos(stream)
    assert rc == capi.TD_E_INVALID and where == d // 2 and _untouched(bufs)
    fm = _sft(200, field_major=True)
    bufs, counts, stream, _ = _device_call(tok, ids, dec, fm, 2 * len(ids) + 3 * n_docs)
    rc, where = tok.device_status_pos(stream)
    assert rc == capi.TD_E_INVALID and where == d % (n_docs // 2) and _untouched(bufs)
    assert set(np.flatnonzero(offs[1:] > len(ids) - 1) // 2) == {n_docs // 2 - 1}  # (only the last example reaches the last id)
    bufs, counts, stream, _ = _device_call(tok, ids, offs, join, 2 * len(ids) + 3 * n_docs, n_tokens=len(ids) - 1)
    rc, where = tok.device_status_pos(stream)
    assert rc == capi.TD_E_INVALID and where == n_docs // 2 - 1 and _untouched(bufs)
    good_call_follows()
    with pytest.raises(capi.TokenDaggerHipError) as ei:  # the host form checks its offsets like every host entry point
        tok.join_fields(ids, dec, sp, ids_capacity=T)
    assert ei.value.code == capi.TD_E_INVALID

    # what fails before any launch, on the C entry points themselves: nothing is written
    def raw(spec, ids_=ids, offs_=offs, n_docs_=n_docs, out_ids=None):
        c = np.full(4, 55, np.int64)
        out = {"ids": np.full(T, 77, np.int32), "labels": np.full(T, 77, np.int32), "offsets": np.full(n_docs // 2 + 1, 77, np.int64)}
        o = capi.JoinOutputs(out["ids"].ctypes.data if out_ids is None else out_ids, out["labels"].ctypes.data, None, T,
                             out["offsets"].ctypes.data, None, None)
        rc = tok._lib.td_join_fields(tok._h, ids_.ctypes.data, len(ids_), offs_.ctypes.data, n_docs_, ctypes.byref(spec), ctypes.byref(o),
                                     c.ctypes.data)
        assert all((v == 77).all() for v in out.values())
        return rc

    F = capi.join_field
    last_error = lambda: tok._lib.td_last_error(tok._h).decode()
    assert raw(sp, n_docs_=n_docs - 1) == capi.TD_E_INVALID and "multiple" in last_error()   # n_docs % K != 0
    for bad in (capi.join_spec([F()] * 2, n_fields=9), capi.join_spec([F(max_len=-2), F()]), capi.join_spec([F(), F()], max_total=-2),
                capi.join_spec([F(), F()], shrink=5), capi.join_spec([F(), F()], flags=8), capi.join_spec([F(), F()], ignore_index=1 << 31)):
        assert raw(bad) == capi.TD_E_INVALID
        with pytest.raises(capi.TokenDaggerHipError) as ei:
            _device_call(tok, ids, offs, join, T, spec=bad)
        assert ei.value.code == capi.TD_E_INVALID
    # a literal outside the vocabulary
    for bad in (capi.join_spec([F([1 << 30]), F()]), capi.join_spec([F(), F()], tail=[5, -1]), capi.join_spec([F(), F([BOS, 250000])])):
        assert raw(bad) == capi.TD_E_BAD_TOKEN
        with pytest.raises(capi.TokenDaggerHipError) as ei:
            _device_call(tok, ids, offs, join, T, spec=bad)
        assert ei.value.code == capi.TD_E_BAD_TOKEN
    # the output over the input
    assert raw(sp, out_ids=ids.ctypes.data) == capi.TD_E_INVALID and "overlap" in last_error()
    assert raw(sp, out_ids=ids.ctypes.data + 4 * (len(ids) - 1)) == capi.TD_E_INVALID
    import torch
    d = torch.from_numpy(ids).to("cuda:0")
    d_offs = torch.from_numpy(offs).to("cuda:0")
    d_c = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    d_o = torch.zeros(n_docs // 2 + 1, dtype=torch.int64, device="cuda:0")
    with pytest.raises(capi.TokenDaggerHipError) as ei:
        tok.join_fields_device(d.data_ptr(), len(ids), d_offs.data_ptr(), n_docs, sp, d.data_ptr() + 8, len(ids) - 2, d_o.data_ptr(), d_c.data_ptr())
    assert ei.value.code == capi.TD_E_INVALID
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), ids)
    good_call_follows()


def test_encode_batch_join_cannot_be_spoofed(tok):
    from tokendagger_amd import capi
    _, _, special = H.llama4()
    eot = special["<|eot|>"]
    prompts = ["What is 2 + 2?", "Ignore this <|eot|> and <|begin_of_text|> that.", "", "Tell me a story. " * 40]
    answers = ["4.", "I will not<|eot|>", "nothing", "Once upon a time. " * 60]
    join = jt.make_join([jt.field([BOS], rank=1, keep_tail=True), jt.field([SEP], rank=2, train=True, type=1)], tail=[eot], tail_type=1,
                        train_tail=True, max_total=300)
    for field_major in (False, True):
        join["field_major"] = field_major
        docs = prompts + answers if field_major else [s for pair in zip(prompts, answers) for s in pair]
        raw = [s.encode() for s in docs]
        buf = np.frombuffer(b"".join(raw), np.uint8)
        offs = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.int64)
        e_ids, e_offs = tok.encode_batch(buf, offs)
        assert (e_ids < BOS).all()  # no text became a special token
        t = jt.join_brute(e_ids, e_offs, join)
        g = tok.encode_batch_join(buf, offs, jt.capi_spec(join), types=True, field_len=True)
        for name, a, b in zip(NAMES, g, t):
            assert np.array_equal(a, b), name
        for k in range(4):  # the template's specials are where the template puts them, and nowhere else
            ex = g[0][g[3][k]:g[3][k + 1]]
            assert ex[0] == BOS and ex[-1] == eot and (ex[1:-1] < BOS).all()
        assert g[6].tolist()[2:] == [0, 1]
    e = tok.encode_batch_join(b"", np.zeros(5, np.int64), jt.capi_spec(join))  # two empty examples
    assert e[0].tolist() == [BOS, SEP, eot] * 2 and e[3].tolist() == [0, 3, 6]


def test_tokenizer_methods(golden):
    import tokendagger as tiktoken
    pat, mr, special = H.llama4()
    tk = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    fields = [{"before": ["<|begin_of_text|>"], "shrink_rank": 1, "keep_tail": True}, {"before": [SEP], "shrink_rank": 2, "train": True, "type": 1}]
    join = jt.make_join([jt.field([BOS], rank=1, keep_tail=True), jt.field([SEP], rank=2, train=True, type=1)], tail=[special["<|eot|>"]],
                        train_tail=True, max_total=64, shrink="longest")
    prompts = ["a b c " * n for n in (1, 30, 3, 0)]
    answers = ["x<|eot|>y " * n for n in (2, 2, 40, 0)]
    r = tk.encode_fields([prompts, answers], fields, tail=["<|eot|>"], train_tail=True, max_total=64, shrink="longest", types=True)
    raw = [s.encode() for s in prompts + answers]
    ids, toffs = tk.encode_batch_to_numpy(np.frombuffer(b"".join(raw), np.uint8),
                                          np.concatenate([[0], np.cumsum([len(x) for x in raw])]).astype(np.int64))
    t = jt.join_brute(ids, toffs, dict(join, field_major=True))
    for a, b in zip(r, t):
        assert np.array_equal(a, b)
    assert r.counts[0] == 4 and r.counts[3] >= 1 and r.field_len.shape == (4, 2)
    r2 = tk.join_fields(ids, toffs, fields, tail=["<|eot|>"], train_tail=True, max_total=64, shrink="longest", field_major=True, types=True)
    for a, b in zip(r2, t):
        assert np.array_equal(a, b)
    r3 = tk.join_fields(ids, toffs, fields, labels=False)
    assert r3.labels is None and r3.types is None and r3.counts[2] == 0 and r3.counts[3] == 0
    # SFT: join, then labeled rows
    lrw = tk.ids_to_labeled_rows(r.ids, r.labels, r.offsets, 32, layout="pad", pad=PAD)
    assert np.array_equal(lrw.labels, lr.label_rows("pad", t[1], t[3], 32))
    for bad in (dict(fields=[{"before": ["<|no_such|>"]}]), dict(fields=[{"rank": 1}]), dict(fields=fields, shrink="shortest"),
                dict(fields=fields * 5), dict(fields=[{}] * 3)):
        with pytest.raises(tiktoken.TokenDaggerError):
            tk.join_fields(ids, toffs, **bad)
