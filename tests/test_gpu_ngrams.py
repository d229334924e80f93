"""N-gram matches on the GPU (td_ngrams.hip) against tests/ngram_truth.py: every comparison is bit for bit, of cover, labels,
doc_stats, pattern_counts and counts.  The contract is the section "n-gram matches" of include/tokendagger_hip.h; every error is a
status code, no case makes the device fault."""
import numpy as np
import pytest

import helpers as H
import ngram_truth as nt

pytestmark = pytest.mark.gpu

TILE = nt.TILE
FILL = -7777  # the guard elements around every output of the device form
GUARD = 64


@pytest.fixture(scope="module")
def tok():
    from tokendagger_amd import capi
    pat, mr, special = H.llama4()
    return capi.HipTokenizer(pat, mr, special, device=0)


@pytest.fixture(scope="module")
def cases():
    """Built once, shared and left unchanged: name -> (case, truth with labels = the ids)."""
    return {name: (c, nt.matches_numpy(c["seqs"], c["ids"], c["offs"], labels=c["ids"])) for name, c in nt.limit_cases().items()}


def _host(tok, c, want, what="", **kw):
    with tok.ngram_set(c["seqs"]) as nset:
        got = tok.ngram_matches(nset, c["ids"], c["offs"], labels=c["ids"], pattern_counts=True, **kw)
    nt.same(got, want, what)
    return got


def _device_setup(tok, nset, c, n_pats, cover=True, labels=True, doc_stats=True, pattern_counts=True, accumulate=False, preset=None,
                  ignore=-100, n_tokens=None, offs=None, shift=0):
    """Everything td_ngram_matches_device needs, uploaded and synchronised; every output lies inside a larger FILL-filled tensor.
    -> (call(tok, stream), result() -> (the five outputs | None, guards untouched)).  labels start as a copy of the ids."""
    import torch
    from tokendagger_amd import capi
    dev = torch.device("cuda", 0)
    ids = np.ascontiguousarray(c["ids"], dtype=np.int32)
    o = np.ascontiguousarray(c["offs"] if offs is None else offs, dtype=np.int64)
    n_docs, total = len(o) - 1, len(ids)
    d_ids = torch.from_numpy(np.concatenate([np.full(shift, 12345, dtype=np.int32), ids])).to(dev)
    d_offs = torch.from_numpy(o).to(dev)

    def guarded(n, dtype, init=None):
        t = torch.full((n + 2 * GUARD,), FILL if dtype != torch.uint8 else 0xAB, dtype=dtype, device=dev)
        if init is not None:
            t[GUARD:GUARD + n] = torch.from_numpy(np.ascontiguousarray(init).reshape(-1)).to(dev)
        return t
    d_cover = guarded(total, torch.uint8) if cover else None
    d_labels = guarded(total, torch.int32, ids) if labels else None
    d_stats = guarded(2 * n_docs, torch.int64) if doc_stats else None
    d_pc = guarded(n_pats, torch.int64, preset) if pattern_counts else None
    d_counts = guarded(4, torch.int64)
    spec = capi.ngram_spec(ignore, accumulate=accumulate)
    torch.cuda.synchronize()

    def ptr(t, size):
        return t.data_ptr() + GUARD * size if t is not None else 0

    def call(handle, stream):
        rc = handle.ngram_matches_device(nset, d_ids.data_ptr() + 4 * shift if total else 0, total if n_tokens is None else n_tokens,
                                         d_offs.data_ptr(), n_docs, spec, ptr(d_cover, 1), ptr(d_labels, 4), ptr(d_stats, 8), ptr(d_pc, 8),
                                         ptr(d_counts, 8), stream)
        assert rc is None  # (nothing comes back but through device_status)

    def result():
        guards, out = True, []
        for t, n, fill in ((d_cover, total, 0xAB), (d_labels, total, FILL), (d_stats, 2 * n_docs, FILL), (d_pc, n_pats, FILL), (d_counts, 4, FILL)):
            if t is None:
                out.append(None)
                continue
            a = t.cpu().numpy()
            guards = guards and bool((a[:GUARD] == fill).all() and (a[GUARD + n:] == fill).all())
            out.append(a[GUARD:GUARD + n].copy())
        if out[2] is not None:
            out[2] = out[2].reshape(n_docs, 2)
        return tuple(out), guards
    return call, result


def _device_ok(tok, c, want, what="", **kw):
    import torch
    with tok.ngram_set(c["seqs"]) as nset:
        call, result = _device_setup(tok, nset, c, len(c["seqs"]), **kw)
        stream = torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream
        call(tok, stream)
        tok.device_status(stream)
        got, guards = result()
    assert guards, what
    nt.same(got, want, what)
    return got


def test_limit_cases_host_and_device_forms(tok, cases):
    for name, (c, want) in cases.items():
        _host(tok, c, want, name)
        _device_ok(tok, c, want, name)
    assert cases["dense"][1][4][0] > 5000 and cases["sparse"][1][4][0] > 30  # dense and sparse matches
    assert cases["no_docs"][1][4].tolist() == [0, 0, 0, 0]


def test_a_64_id_pattern_at_every_split_of_a_tile_border(tok):
    rng = np.random.default_rng(51)
    for split in range(0, 65):
        c = nt.tile_split(rng, split)
        want = nt.matches_numpy(c["seqs"], c["ids"], c["offs"], labels=c["ids"])
        assert want[4].tolist() == [1, 64, 1, 0]
        _host(tok, c, want, split)


def test_eight_lengths_and_set_info(tok, cases):
    c, want = cases["eight_lengths"]
    with tok.ngram_set(c["seqs"]) as nset:
        info = nset.info
        assert info["patterns"] == 24 and info["distinct"] == 24 and info["lengths"] == 8 and info["max_len"] == 64
        assert info["slots"] == 64 and info["device_bytes"] > 0 and 0 <= info["max_probe"] < 64
    c, want = cases["repeats"]
    with tok.ngram_set(c["seqs"]) as nset:
        assert nset.info["patterns"] == 7 and nset.info["distinct"] == 3
    assert want[3][[2, 4, 5, 6]].tolist() == [0, 0, 0, 0] and want[3][[0, 1, 3]].min() >= 1  # a repeated sequence counts under its lowest index


def test_outputs_are_optional(tok, cases):
    c, want = cases["dense"]
    only_labels = _device_ok(tok, c, want, "labels without cover", cover=False, doc_stats=False, pattern_counts=False)
    assert only_labels[0] is None and only_labels[2] is None and only_labels[3] is None
    _device_ok(tok, c, want, "cover without labels", labels=False)
    only_counts = _device_ok(tok, c, want, "only counts", cover=False, labels=False, doc_stats=False, pattern_counts=False)
    assert np.array_equal(only_counts[4], want[4])
    want5 = nt.matches_numpy(c["seqs"], c["ids"], c["offs"], labels=c["ids"], ignore=-5)
    _device_ok(tok, c, want5, "another ignore_index", ignore=-5)
    with tok.ngram_set(c["seqs"]) as nset:
        got = tok.ngram_matches(nset, c["ids"], c["offs"], cover=False, doc_stats=False)
        assert got[0] is None and got[2] is None and got[3] is None and np.array_equal(got[4], want[4])


@pytest.mark.parametrize("shift", [1, 3])
def test_ids_off_the_16_byte_grid(tok, cases, shift):
    c, want = cases["sparse"]
    _device_ok(tok, c, want, shift, shift=shift)


def test_accumulate_over_two_calls(tok, cases):
    c, want = cases["dense"]
    preset = np.full(len(c["seqs"]), 2**32 - 5, dtype=np.int64)  # the sum carries into the upper word
    got = _device_ok(tok, c, (want[0], want[1], want[2], want[3] + (2**32 - 5), want[4]), "onto a preset", accumulate=True, preset=preset)
    _device_ok(tok, c, (want[0], want[1], want[2], 2 * want[3] + (2**32 - 5), want[4]), "twice", accumulate=True, preset=got[3])
    from tokendagger_amd import capi
    with tok.ngram_set(c["seqs"]) as nset:
        acc = want[3].copy()
        got = tok.ngram_matches(nset, c["ids"], c["offs"], capi.ngram_spec(accumulate=True), pattern_counts=acc)
        assert got[3] is acc and np.array_equal(acc, 2 * want[3]) and np.array_equal(got[2], want[2])  # doc_stats is never accumulated


def test_two_hundred_thousand_patterns(tok):
    rng = np.random.default_rng(61)
    n_pats, k = 200000, 13
    flat = rng.integers(0, 1000, size=n_pats * k).astype(np.int32)
    seqs = flat.reshape(n_pats, k)
    total = 3 * TILE + 12
    ids = nt.junk(rng, total)
    for p, q in zip(rng.integers(0, n_pats, size=150), rng.integers(0, total - k, size=150)):
        ids[q:q + k] = seqs[p]
    c = dict(seqs=seqs, ids=ids, offs=nt.random_offsets(rng, total, 20))
    want = nt.matches_numpy(seqs, ids, c["offs"], labels=ids)
    assert want[4][0] >= 100
    with tok.ngram_set(flat, np.arange(n_pats + 1, dtype=np.int64) * k) as nset:
        info = nset.info
        assert info["distinct"] == n_pats and info["slots"] == 1 << 19 and info["max_probe"] > 1  # lookups walk further than one slot
        nt.same(tok.ngram_matches(nset, ids, c["offs"], labels=ids, pattern_counts=True), want)


@pytest.mark.parametrize("bits", [1, 4, 0])
def test_tag_bits_change_nothing(tok, bits):
    """tests/test_ngram_model.py shows on the CPU that these inputs meet tag matches whose ids differ at 1 to 4 bits."""
    from tokendagger_amd import capi
    c = nt.forced_collisions(np.random.default_rng(31))
    want = nt.matches_numpy(c["seqs"], c["ids"], c["offs"], labels=c["ids"])
    tok.set_option(capi.TD_OPT_NGRAM_TAG_BITS, bits)
    try:
        _host(tok, c, want, bits)
        _device_ok(tok, c, want, bits)
    finally:
        tok.set_option(capi.TD_OPT_NGRAM_TAG_BITS, 0)
    for bad in (-1, 32, 1 << 20):
        with pytest.raises(capi.TokenDaggerHipError):
            tok.set_option(capi.TD_OPT_NGRAM_TAG_BITS, bad)


def test_two_clones_share_one_set_on_two_streams(tok, cases):
    import torch
    dev = torch.device("cuda", 0)
    c, want = cases["dense"]
    c2, want2 = cases["sparse"]
    both = dict(seqs=c["seqs"] + c2["seqs"])
    a, b = tok.clone(), tok.clone()
    try:
        with tok.ngram_set(both["seqs"]) as nset:
            n = len(both["seqs"])
            w1 = nt.matches_numpy(both["seqs"], c["ids"], c["offs"], labels=c["ids"])
            w2 = nt.matches_numpy(both["seqs"], c2["ids"], c2["offs"], labels=c2["ids"])
            call1, res1 = _device_setup(a, nset, c, n)
            call2, res2 = _device_setup(b, nset, c2, n)
            s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
            for _ in range(3):
                call1(a, s1.cuda_stream)
                call2(b, s2.cuda_stream)
            a.device_status(s1.cuda_stream)
            b.device_status(s2.cuda_stream)
            torch.cuda.synchronize()
            (g1, ok1), (g2, ok2) = res1(), res2()
            assert ok1 and ok2
            nt.same(g1, w1, "first clone")  # (three calls in place: the labels were covered by the first, the ids are what is read)
            nt.same(g2, w2, "second clone")
    finally:
        a.close()
        b.close()


def test_device_form_does_not_wait_and_bad_offsets_are_status_codes(tok, cases):
    import torch
    from tokendagger_amd import capi
    dev = torch.device("cuda", 0)
    c, want = cases["document_edges"]
    down = c["offs"].copy()
    down[4], down[7] = down[3] - 50, down[6] - 1  # documents 3 and 6 decrease
    with tok.ngram_set(c["seqs"]) as nset:
        n = len(c["seqs"])
        # nothing synchronises.  Buffers first; then long work on the side stream in front of the call; when the call has returned, the
        # work in front of it has not finished, so the call waited for nothing on its stream and read nothing back
        call, result = _device_setup(tok, nset, c, n, offs=down)
        side = torch.cuda.Stream(device=dev)
        x = torch.randn(4096, 4096, device=dev)
        y = x @ x  # (the first product loads its library: before anything is timed against it)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            z = x
            for _ in range(40):
                z = z @ x * 1e-3
            front = torch.cuda.Event()
            front.record(side)
        call(tok, side.cuda_stream)
        behind = torch.cuda.Event()
        behind.record(side)
        assert not front.query() and not behind.query() and not side.query(), "td_ngram_matches_device waited for its stream"
        rc, where = tok.device_status_pos(side.cuda_stream)  # (this one synchronises)
        assert behind.query() and rc == capi.TD_E_INVALID and where == 3  # the lowest bad document
        torch.cuda.synchronize()
        got, guards = result()
        assert guards
        assert (got[0] == 0xAB).all() and np.array_equal(got[1], c["ids"]) and (got[2] == FILL).all() and (got[3] == FILL).all() and \
            (got[4] == FILL).all(), "bad offsets: nothing is written"
        assert tok.device_status_pos(side.cuda_stream)[0] == capi.TD_OK  # cleared
        for o, n_tok, doc in ((np.concatenate([[1], c["offs"][1:]]), None, 0), (c["offs"], len(c["ids"]) - 5, len(c["offs"]) - 2),
                              (np.concatenate([[0, -3], c["offs"][2:]]), None, 0)):
            call, result = _device_setup(tok, nset, c, n, offs=o, n_tokens=n_tok)
            stream = torch.cuda.current_stream(dev).cuda_stream
            call(tok, stream)
            rc, where = tok.device_status_pos(stream)
            got, guards = result()
            assert rc == capi.TD_E_INVALID and where == doc and guards and (got[4] == FILL).all() and (got[0] == 0xAB).all(), (doc, where)
        # and the next good call on the same handle
        call, result = _device_setup(tok, nset, c, n)
        stream = torch.cuda.current_stream(dev).cuda_stream
        call(tok, stream)
        tok.device_status(stream)
        got, guards = result()
        assert guards
        nt.same(got, want)
        # host form: the offsets are checked before any launch
        with pytest.raises(capi.TokenDaggerHipError) as e:
            tok.ngram_matches(nset, c["ids"], down)
        assert e.value.code == capi.TD_E_INVALID and "non-decreasing" in str(e.value)


def test_spec_and_set_errors_come_before_any_launch(tok, cases):
    from tokendagger_amd import capi
    c, want = cases["sparse"]
    for seqs, word in (([[]], "length"), ([list(range(65))], "length"), ([[1] * k for k in range(1, 10)], "8 distinct"), ([[3, -1]], "negative"),
                       ([], "n_pats")):
        with pytest.raises(capi.TokenDaggerHipError) as e:
            tok.ngram_set(seqs)
        assert e.value.code == capi.TD_E_INVALID and word in str(e.value), (seqs, str(e.value))
    with tok.ngram_set(c["seqs"]) as nset:
        for spec, word in ((capi.NgramSpec(-100, 2), "flags"), (capi.NgramSpec(2**31, 0), "int32"), (capi.NgramSpec(-2**31 - 1, 1), "int32")):
            with pytest.raises(capi.TokenDaggerHipError) as e:
                tok.ngram_matches(nset, c["ids"], c["offs"], spec)
            assert e.value.code == capi.TD_E_INVALID and word in str(e.value)
            with pytest.raises(capi.TokenDaggerHipError) as e:
                tok.ngram_matches_device(nset, 0, 0, 8, 0, spec, 0, 0, 0, 0, 8, 0)  # (the spec is looked at before any pointer)
            assert e.value.code == capi.TD_E_INVALID and word in str(e.value)
        nt.same(tok.ngram_matches(nset, c["ids"], c["offs"], labels=c["ids"], pattern_counts=True), want)


def test_fused_equals_encode_then_match(tok, golden):
    n_docs = 300
    doc_offs = golden["offsets"][:n_docs + 1].astype(np.int64)
    text = golden["text"][:int(doc_offs[-1])]
    ids, offs = tok.encode_batch(text, doc_offs)
    rng = np.random.default_rng(71)
    starts = rng.integers(0, len(ids) - 13, size=400)
    seqs = [ids[q:q + 13].tolist() for q in starts] + [ids[q:q + 4].tolist() for q in starts[:50]]
    with tok.ngram_set(seqs) as nset:
        want = tok.ngram_matches(nset, ids, offs, pattern_counts=True)
        nt.same(want, nt.matches_numpy(seqs, ids, offs))
        ds, pc, counts, total = tok.encode_batch_ngram_matches(text, doc_offs, nset, pattern_counts=True)
        assert total == len(ids) and counts[0] >= 400
        nt.same((None, None, ds, pc, counts), want)
        ds, pc, counts, total = tok.encode_batch_ngram_matches(text, doc_offs, nset, doc_stats=False)
        assert ds is None and pc is None and np.array_equal(counts, want[4])
        e = tok.encode_batch_ngram_matches(b"", np.zeros(4, np.int64), nset)
        assert not e[0].any() and not e[2].any() and e[3] == 0


def test_tokenizer_methods_and_the_decontamination_recipe(cases):
    import tokendagger as tiktoken
    pat, mr, special = H.llama4()
    tk = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    rng = np.random.default_rng(81)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)

    def words(n):  # random six-letter words: no eight ids in a row are shared by chance
        return " ".join(bytes(rng.choice(letters, size=6)).decode() for _ in range(n))
    docs = [words(40) for _ in range(20)]
    sources, quoting = [0, 1, 2, 3, 4], {10: 0, 11: 3, 12: 4}
    for d, src in quoting.items():
        docs[d] = words(15) + " " + docs[src] + " " + words(15)
    data = [d.encode() for d in docs]
    text = np.frombuffer(b"".join(data), dtype=np.uint8)
    doc_offs = np.concatenate([[0], np.cumsum([len(b) for b in data])]).astype(np.int64)
    ids, offs = tk.encode_batch_to_numpy(text, doc_offs, ordinary=True)
    with tk.ngram_set_from_texts([docs[s] for s in sources], 8) as nset:
        assert nset.info["lengths"] == 1 and nset.info["max_len"] == 8 and nset.info["distinct"] == nset.info["patterns"]
        r = tk.ids_to_ngram_matches(ids, offs, nset, labels=ids, pattern_counts=True)
        hit = np.flatnonzero(r.doc_stats[:, 0] > 0)
        assert hit.tolist() == sorted(sources + list(quoting)), hit
        assert r.counts[2] == len(hit) and r.cover.sum() == r.counts[1] == r.doc_stats[:, 1].sum()
        assert np.array_equal(r.labels == -100, r.cover == 1) and np.array_equal(r.labels[r.cover == 0], ids[r.cover == 0])
        assert r.pattern_counts.sum() == r.counts[0]
        for s in sources:  # a source document is covered whole
            assert r.doc_stats[s, 1] == offs[s + 1] - offs[s]
        keep = np.flatnonzero(r.doc_stats[:, 0] == 0)  # the decontamination: the keep list of select_docs
        kept_ids, kept_offs = tk.select_docs(ids, offs, keep)[:2]
        assert len(kept_offs) - 1 == 12 and tk.ids_to_ngram_matches(kept_ids, kept_offs, nset).counts.tolist() == [0, 0, 0, 0]
        e, total = tk.encode_batch_to_ngram_matches(text, doc_offs, nset, ordinary=True)
        assert total == len(ids) and np.array_equal(e.doc_stats, r.doc_stats) and np.array_equal(e.counts, r.counts) and e.cover is None
    with tk.ngram_set_from_texts([docs[0]], 8, stride=8) as coarse:
        assert 0 < coarse.info["patterns"] <= (offs[1] - offs[0]) // 8
    c, want = cases["nested"]
    with tk.ngram_set(c["seqs"]) as nset:
        r = tk.ids_to_ngram_matches(c["ids"], c["offs"], nset, cover=False)
        assert r.cover is None and np.array_equal(r.counts, want[4])
    for bad in ([[]], []):
        with pytest.raises(tiktoken.TokenDaggerError):
            tk.ngram_set(bad)
    with pytest.raises(tiktoken.TokenDaggerError):
        tk.ngram_set_from_texts(["a b"], 13)
