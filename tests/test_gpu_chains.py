"""Chains of device calls on ONE handle with no host wait between them.

Every td_*_device entry point is asynchronous on the caller's stream, and INTEGRATION.md tells callers to hand one call's device outputs
to the next call.  What makes that safe is shared by all of them (td_api.cpp): a call on another stream than the handle's previous call
waits for that call's event (order_before / order_after); a workspace buffer that has to grow is parked until the next synchronisation
point, not freed (ensure's graveyard); the control block's error is taken with atomicCAS(err, 0, code), so the first error wins and
stays until td_device_status reads it; MinHash's parameter table, the head words every operation zeroes, and the n-gram set are reused
from call to call.  The tests of the single operations make one call and then read the status, which synchronises.  Here:

  1. the text chain      utf8_device (replace) -> nfc_device -> text_stats_device (all groups) -> encode_device, each on the previous
                         call's device text and device offsets, one stream, one status read at the end;
  2. the token chain     select_docs_device -> span_labels_device -> make_rows_labeled_device -> token_counts_device -> minhash_device ->
                         ngram_matches_device -> token_starts_device -> decode_rows_device, everything on the selected ids and offsets
                         that never left the device; twice on the same handle without a status read, the second time with another
                         MinHash seed (the table is rebuilt in stream order behind a call that may still read the old one);
  3. alternating streams fourteen calls with disjoint, uploaded inputs, call i on stream i % 3, the test adds no ordering of its own:
                         an entry point that did not order itself behind the previous call would share its scratch with a running kernel;
  4. workspace growth    small, large, small for encode, nfc, text_stats, minhash and pack_rows on a fresh clone under TD_OPT_WS_FILL,
                         TD_INFO_WS_FILLED_BYTES rising across every large call; then the same on two alternating streams;
  5. an unread error     the chains of 1 and 2 with one call (or two) in the middle made bad by its offsets: the status at the end is the
                         FIRST bad call's, its outputs still hold the fill, every other call equals its truth, the second status is TD_OK.

Every expected value is built on the CPU before anything is launched: stage N's truth is the suite's truth of stage N - 1's truth
(td_utf8_host / td_nfc_host, the contract's executable statements the device tests of those passes compare with, and here compared with
tests/utf8_truth.py and tests/nfc_truth.py first; textstats_truth; the oracle's ids; select_, labels_, rows_, labeled_rows_, counts_,
minhash_, ngram_, offsets_, decode_rows_ and pack_truth).  Sizes and capacities are the truth's, exactly.  Outputs are filled with 0xA7
bytes between 16 guard elements; everything is compared with equality, nothing with a tolerance.

What this does NOT show: whether a later call really overlaps an earlier one cannot be proven from the host, nobody has measured it, and
no assertion here depends on it: the results must be right whether or not calls overlap.  The counter of 4 proves that buffers were
replaced between the calls, not that the replaced buffer was still being read.  For td_minhash_device the only buffer that depends on
the call is the (a_j, b_j) table, whose size is num_perm's: its "large" call has 128 permutations against the small calls' 16.

Left out of the chains of 1, 2 and 5: td_pack_rows_device and td_pack_rows_labeled_device.  They read a table back and wait for the
stream themselves (include/tokendagger_hip.h), which is a host wait in the middle of a chain; 2 takes td_make_rows_labeled_device.  In 4
td_pack_rows_device takes part as the issue of growth asks: the wait is the library's own, the test adds none.

No case here makes the device fault: every bad input is one the library reports by a status code."""
from __future__ import annotations

import numpy as np
import pytest

import chain_cases as cc
import helpers as H

pytestmark = pytest.mark.gpu

BOS, EOS, PAD = 200000, 200001, -5  # Llama-4 <|begin_of_text|>, <|end_of_text|>
S = 128                       # rows split documents
K, PERM, BANDS, ROWS = 5, 128, 16, 8
N_BINS, N_GROUPS = 50000, 3
UT_PIECES = ("noise, documents", "small documents", "mixed scripts, cut every 1000", "a tile of strays, documents",
             "boundary in four@2, tile seam, empty documents")
NT_PIECES = ("nfd of mixed, documents", "ill-formed", "truncated then continuation", "begins with a mark", "marks 33", "triples")


@pytest.fixture(scope="module")
def tok():
    from tokendagger_amd import capi
    pat, mr, special = H.llama4()
    t = capi.HipTokenizer(pat, mr, special, device=0)
    yield t
    t.close()


@pytest.fixture(scope="module")
def streams():
    import torch
    return [torch.cuda.Stream(device=cc.dev()) for _ in range(3)]


def _sync():
    import torch
    torch.cuda.synchronize()


# ---- the truths: built once, shared, left unchanged ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def text_case(golden):
    """About 256 KiB: pieces of the UTF-8 and NFC limit cases and the golden documents of at most 20 000 bytes from the first on, empty
    documents at both ends."""
    from tokendagger_amd import capi
    import nfc_truth as nt
    import textstats_truth as tt
    import utf8_truth as ut
    u, n = ut.limit_cases(4096), nt.limit_cases(4096)
    docs = [b"", b""]
    for name in UT_PIECES:
        docs += ut.docs_of(*u[name])
    for name in NT_PIECES:
        docs += nt.docs_of(*n[name])
    g, go = golden["text"].tobytes(), golden["offsets"]
    total, taken = sum(len(d) for d in docs), 0
    for d in range(len(go) - 1):
        if total >= 256 * 1024:
            break
        if 0 < go[d + 1] - go[d] <= 20000:
            docs.append(g[go[d]:go[d + 1]])
            total += len(docs[-1])
            taken += 1
    docs += [b"", b""]
    assert taken >= 200 and 256 * 1024 <= total < 300 * 1024
    text, offs = nt.batch(docs)
    n_docs = len(docs)
    c = dict(text=text, offs=offs, n_docs=n_docs)
    c["utf8"] = capi.utf8_host(text, offs, capi.TD_UTF8_REPLACE)
    ut.same(c["utf8"], ut.truth(text, offs, ut.REPLACE, by=ut.codec_walk), "the chain's input, repaired")
    assert c["utf8"][2].sum() >= 10 and c["utf8"][5][0] != len(text), "no document is ill-formed: the repair rewrites nothing"
    c["nfc"] = capi.nfc_host(c["utf8"][0], c["utf8"][1])
    nt.same(c["nfc"], nt.truth(c["utf8"][0], c["utf8"][1]), "the chain's input, normalised")
    assert c["nfc"][3].sum() >= 5, "no document changes under NFC"
    ntext, noffs = c["nfc"][0], c["nfc"][1]
    c["stats"] = tt.truth(ntext, noffs)
    ids, toffs = H.port_tokenizer().encode_batch(ntext.tobytes(), noffs)
    c["enc"] = (np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(toffs, dtype=np.int64))
    assert len(c["enc"][0]) > 50000
    # documents that are not empty, for the bad offsets of 5
    full = np.flatnonzero((np.diff(c["utf8"][1]) > 0) & (np.diff(noffs) > 0))
    c["bad_docs"] = (int(full[len(full) // 3]), int(full[2 * len(full) // 3]))
    return c


@pytest.fixture(scope="module")
def voc():
    import decode_rows_truth as dt
    import offsets_truth as OT
    _, mr, special = H.llama4()
    return dt.Vocab({r: b for b, r in mr.items()}), OT.id_lengths(OT.id_bytes(mr, special))


@pytest.fixture(scope="module")
def token_case(golden, voc):
    """400 golden documents of at most 4000 ids, the first 250 and the 150 longest; a selection that reorders, drops and filters by length;
    every later stage's truth."""
    import counts_truth as ct
    import decode_rows_truth as dt
    import labeled_rows_truth as lr
    import labels_truth as lt
    import minhash_truth as mt
    import ngram_truth as ngt
    import offsets_truth as OT
    import rows_truth as rt
    import select_truth as st
    ids, offs = golden["enc"].astype(np.int32), golden["enc_offsets"].astype(np.int64)
    L = np.diff(offs)
    fit = np.flatnonzero(L <= 4000)
    longest = fit[np.argsort(-L[fit], kind="stable")[:150]]
    pick = np.sort(np.concatenate([np.setdiff1d(fit, longest)[:250], longest]))
    assert len(pick) == 400
    ids0 = np.concatenate([ids[offs[d]:offs[d + 1]] for d in pick])
    offs0 = np.concatenate([[0], np.cumsum(np.diff(offs)[pick])]).astype(np.int64)
    rng = np.random.default_rng(31)
    sel = rng.permutation(400)[:330].astype(np.int64)
    mn, mx = 3, 2500
    c = dict(ids0=ids0, offs0=offs0, sel=sel, mn=mn, mx=mx)
    c["select"] = w = st.select_numpy(ids0, offs0, sel, mn, mx)
    sids, soffs = w[0], w[2]
    kept, T = int(w[4][0]), int(w[4][1])
    assert kept >= 200 and w[4][2] > 0 and w[4][3] > 0 and T > 30000 and len(soffs) == kept + 1
    c.update(sids=sids, soffs=soffs, kept=kept, T=T)
    f = np.argsort(-np.bincount(sids))[:6].tolist()
    c["open"], c["close"] = [[f[1]], [f[2], f[4]]], [f[0], f[3]]
    c["labels"] = lt.labels_numpy(sids, soffs, c["open"], c["close"], -100, True)
    assert c["labels"][3][0] > 1000 and c["labels"][3][1] > 100
    c["rows"] = rt.rows_numpy(sids, soffs, S, rt.CONCAT, BOS, EOS, PAD, False)
    c["row_labels"] = lr.label_rows("concat", c["labels"][0], soffs, S, bos=True, eos=True, bos_value=-1, eos_value=-2, pad_value=-3)
    assert c["rows"][3][0] > 200 and (np.diff(soffs) > S).sum() > 30
    c["groups"] = (np.arange(kept) % N_GROUPS).astype(np.int32)
    c["counts"] = ct.counts_numpy(sids, N_BINS, soffs, c["groups"], N_GROUPS)
    assert c["counts"][1][0] > 0 and c["counts"][1][2] > 0
    c["minhash"] = {seed: mt.minhash_numpy(sids, soffs, K, PERM, seed, BANDS, ROWS) for seed in (1, 2)}
    assert not np.array_equal(c["minhash"][1][0], c["minhash"][2][0])
    seqs = [sids[q:q + k].tolist() for k, q in zip((2, 3, 5, 8, 2, 3, 13, 5, 1, 2), rng.integers(0, T - 20, 10))]
    c["seqs"] = seqs
    c["ngram"] = ngt.matches_numpy(seqs, sids, soffs, labels=sids)
    assert c["ngram"][4][0] >= 10
    c["starts"] = OT.covered_byte_starts(sids, soffs, voc[1])
    c["decode"] = dt.decode_numpy(sids, voc[0], tok_offsets=soffs)
    d = int(np.flatnonzero(np.diff(soffs) > 0)[kept // 2])
    c["bad_doc"] = d
    c["above"] = int(np.searchsorted(soffs, T - 10, side="right")) - 1  # the first document that ends above n_tokens = T - 10
    assert 0 < c["above"] < kept
    return c


@pytest.fixture(scope="module")
def nset(tok, token_case):
    s = tok.ngram_set(token_case["seqs"])
    yield s
    _sync()
    s.close()


# ---- the chains ------------------------------------------------------------------------------------------------------------------------

def text_chain(c, bad=(), keep=None):
    """-> the four operations.  bad: names of the calls whose offsets decrease (at c["bad_docs"][0] for nfc, [1] for text_stats); the calls
    behind a bad one read uploaded copies of the truth of the stage they need, not the bad call's outputs."""
    from tokendagger_amd import capi
    import textstats_truth as tt
    keep = keep if keep is not None else []
    n_docs = c["n_docs"]
    t, p_text = cc.up(c["text"], np.uint8, front=16 + 5, back=16, pad=0x41)  # (off the 16-byte grid)
    assert p_text % 16 == 5
    t2, p_offs = cc.up(c["offs"], np.int64)
    keep += [t, t2]
    u8 = cc.Utf8(p_text, len(c["text"]), p_offs, n_docs, capi.TD_UTF8_REPLACE, c["utf8"])
    n1, n2 = len(c["utf8"][0]), len(c["nfc"][0])
    nfc_offs = u8.ptr("offsets")
    if "nfc" in bad:
        t, nfc_offs = cc.up(cc.swapped(c["utf8"][1], c["bad_docs"][0]), np.int64)
        keep.append(t)
    nfc = cc.Nfc(u8.ptr("text"), n1, nfc_offs, n_docs, c["nfc"])
    p_ntext, p_noffs = nfc.ptr("text"), nfc.ptr("offsets")
    if bad:
        t, p_ntext = cc.up(c["nfc"][0], np.uint8, front=16, back=16, pad=0x41)
        t2, p_noffs = cc.up(c["nfc"][1], np.int64)
        keep += [t, t2]
    ts_offs = p_noffs
    if "text_stats" in bad:
        t, ts_offs = cc.up(cc.swapped(c["nfc"][1], c["bad_docs"][1]), np.int64)
        keep.append(t)
    ts = cc.TextStats(p_ntext, n2, ts_offs, n_docs, tt.LOCAL | tt.RUNS, c["stats"])
    enc = cc.Encode(p_ntext, n2, p_noffs, n_docs, c["enc"])
    return [u8, nfc, ts, enc]


def token_chain(c, nset, seed=1, bad=(), keep=None):
    """-> the eight operations.  bad: "minhash" (n_tokens ten below the offsets' end: position c["above"]), "ngram" (offsets that decrease at
    c["bad_doc"], uploaded)."""
    keep = keep if keep is not None else []
    t, p_ids0 = cc.up(c["ids0"], np.int32)
    t2, p_offs0 = cc.up(c["offs0"], np.int64)
    keep += [t, t2]
    sel = cc.Select(p_ids0, len(c["ids0"]), p_offs0, len(c["offs0"]) - 1, c["sel"], c["mn"], c["mx"], c["select"])
    T, kept = c["T"], c["kept"]
    on = (sel.ptr("ids"), T, sel.ptr("offsets"), kept)  # the selected ids and offsets, where select_docs_device leaves them
    lab = cc.SpanLabels(*on, c["open"], c["close"], c["labels"])
    rows = cc.RowsLabeled(*on, lab.ptr("labels"), S, BOS, EOS, PAD, c["rows"], c["row_labels"])
    cnt = cc.Counts(*on, c["groups"], N_BINS, N_GROUPS, c["counts"])
    mh = cc.Minhash(sel.ptr("ids"), T - 10 if "minhash" in bad else T, sel.ptr("offsets"), kept, K, PERM, seed, BANDS, ROWS, c["minhash"][seed])
    ng_offs = sel.ptr("offsets")
    if "ngram" in bad:
        t, ng_offs = cc.up(cc.swapped(c["soffs"], c["bad_doc"]), np.int64)
        keep.append(t)
    ng = cc.Ngram(nset, len(c["seqs"]), sel.ptr("ids"), T, ng_offs, kept, c["sids"], c["ngram"])
    starts = cc.TokenStarts(*on, c["starts"])
    dec = cc.DecodeRows(*on, c["decode"])
    return [sel, lab, rows, cnt, mh, ng, starts, dec]


BAD_NAME = {"nfc": "nfc_device", "text_stats": "text_stats_device", "minhash": "minhash_device", "ngram": "ngram_matches_device"}


def run(tok, ops, stream_of):
    """The calls alone, back to back: call i on stream_of(i).  Nothing else touches the device or waits."""
    for i, op in enumerate(ops):
        op.launch(tok, stream_of(i).cuda_stream)


def check(ops, what, bad=()):
    names = {BAD_NAME[b] for b in bad}
    for i, op in enumerate(ops):
        op.check((what, i), written=op.name not in names)


# ---- 1 and 2 ---------------------------------------------------------------------------------------------------------------------------

def test_text_chain_on_one_stream(tok, streams, text_case):
    from tokendagger_amd import capi
    ops = text_chain(text_case)
    _sync()
    run(tok, ops, lambda i: streams[0])
    assert tok.device_status_pos(streams[0].cuda_stream)[0] == capi.TD_OK
    check(ops, "text chain")


def test_token_chain_twice_on_one_stream_with_two_minhash_seeds(tok, streams, token_case, nset):
    from tokendagger_amd import capi
    first, second = token_chain(token_case, nset, seed=1), token_chain(token_case, nset, seed=2)
    _sync()
    run(tok, first + second, lambda i: streams[1])
    assert tok.device_status_pos(streams[1].cuda_stream)[0] == capi.TD_OK
    check(first, "token chain, seed 1")
    check(second, "token chain, seed 2")


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big_cases(golden):
    """The large inputs of 3 and 4: textstats_truth.big_case() (1.2 MiB), about 1 MiB of golden text with its reference ids, 1 MiB of
    mixed-script NFD text, the first 320 000 golden ids."""
    from tokendagger_amd import capi
    import minhash_truth as mt
    import nfc_truth as nt
    import pack_truth as pt
    import textstats_truth as tt
    c = {}
    text, offs = tt.big_case()
    text = np.frombuffer(text, dtype=np.uint8)
    c["stats"] = (text, offs, {g: tt.truth(text, offs, g) for g in (tt.RUNS, tt.LOCAL | tt.RUNS)})
    go, eo = golden["offsets"], golden["enc_offsets"]
    nd = int(np.argmax(go >= 1 << 20))  # whole documents up to the first boundary at or above 1 MiB
    assert (1 << 20) <= go[nd] < 1200 * 1024
    c["encode"] = (golden["text"][:go[nd]], go[:nd + 1].astype(np.int64), (golden["enc"][:eo[nd]].astype(np.int32), eo[:nd + 1].astype(np.int64)))
    raw = nt.mixed(1 << 20, "NFD")
    ntext = np.frombuffer(raw, dtype=np.uint8)
    noffs = np.concatenate([np.arange(0, len(raw), 3001), [len(raw)]]).astype(np.int64)
    c["nfc"] = (ntext, noffs, capi.nfc_host(ntext, noffs))
    assert c["nfc"][2][3].sum() > 100
    md = int(np.argmax(eo >= 300000))
    ids, toffs = golden["enc"][:eo[md]].astype(np.int32), eo[:md + 1].astype(np.int64)
    assert 300000 <= len(ids) < 350000 and md > 100
    c["ids"] = (ids, toffs)
    c["minhash"] = mt.minhash_numpy(ids, toffs, K, PERM, 3, 0, 0)
    c["pack"] = pt.pack_runs(ids, toffs, 512, BOS, EOS, PAD, False)
    return c


def _small(golden, lo, n):
    """n golden documents from lo on: (text, offsets, (ids, token offsets))"""
    go, eo = golden["offsets"], golden["enc_offsets"]
    return (golden["text"][go[lo]:go[lo + n]], (go[lo:lo + n + 1] - go[lo]).astype(np.int64),
            (golden["enc"][eo[lo]:eo[lo + n]].astype(np.int32), (eo[lo:lo + n + 1] - eo[lo]).astype(np.int64)))


def test_independent_calls_on_alternating_streams(tok, streams, text_case, token_case, big_cases, nset):
    """Fourteen calls whose inputs and outputs are disjoint and uploaded before the first call; call i goes to stream i % 3 and the test
    orders nothing.  The largest first, so that the small ones behind it are issued while it plausibly still runs; and the small call
    of the same family directly behind each large one, on the next stream: those two share the family's scratch, not only the control
    block (text_stats 1.2 MiB / 256 KiB, encode 1 MiB / 256 KiB, the two rewrites, which share one tile frame)."""
    from tokendagger_amd import capi
    import textstats_truth as tt
    c, k, keep = text_case, token_case, []

    def up(a, dt, **kw):
        t, p = cc.up(a, dt, **kw)
        keep.append(t)
        return p
    btext, boffs, bwant = big_cases["stats"]
    etext, eoffs, ewant = big_cases["encode"]
    sids, soffs, T, kept = up(k["sids"], np.int32), up(k["soffs"], np.int64), k["T"], k["kept"]
    n_docs = c["n_docs"]
    u8_text, u8_offs = up(c["utf8"][0], np.uint8, front=16 + 3, back=16, pad=0x41), up(c["utf8"][1], np.int64)
    nf_text, nf_offs = up(c["nfc"][0], np.uint8, front=16 + 9, back=16, pad=0x41), up(c["nfc"][1], np.int64)
    stats_runs = tt.truth(c["nfc"][0], c["nfc"][1], tt.RUNS)
    ops = [
        cc.TextStats(up(btext, np.uint8, front=16 + 7, back=16, pad=0x61), len(btext), up(boffs, np.int64), len(boffs) - 1, tt.RUNS, bwant[tt.RUNS]),
        cc.TextStats(nf_text, len(c["nfc"][0]), nf_offs, n_docs, tt.RUNS, stats_runs),
        cc.Encode(up(etext, np.uint8), len(etext), up(eoffs, np.int64), len(eoffs) - 1, ewant),
        cc.Encode(nf_text, len(c["nfc"][0]), nf_offs, n_docs, c["enc"]),
        cc.Nfc(u8_text, len(c["utf8"][0]), u8_offs, n_docs, c["nfc"]),
        cc.Utf8(up(c["text"], np.uint8, front=16 + 1, back=16, pad=0x41), len(c["text"]), up(c["offs"], np.int64), n_docs, capi.TD_UTF8_REPLACE, c["utf8"]),
        cc.RowsLabeled(sids, T, soffs, kept, up(k["labels"][0], np.int32), S, BOS, EOS, PAD, k["rows"], k["row_labels"]),
        cc.Select(up(k["ids0"], np.int32), len(k["ids0"]), up(k["offs0"], np.int64), len(k["offs0"]) - 1, k["sel"], k["mn"], k["mx"], k["select"]),
        cc.SpanLabels(sids, T, soffs, kept, k["open"], k["close"], k["labels"]),
        cc.Counts(sids, T, soffs, kept, k["groups"], N_BINS, N_GROUPS, k["counts"]),
        cc.Ngram(nset, len(k["seqs"]), sids, T, soffs, kept, k["sids"], k["ngram"]),
        cc.Minhash(sids, T, soffs, kept, K, PERM, 2, BANDS, ROWS, k["minhash"][2]),
        cc.DecodeRows(sids, T, soffs, kept, k["decode"]),
        cc.TokenStarts(sids, T, soffs, kept, k["starts"]),
    ]
    assert len(ops) >= 12 and len({op.name for op in ops}) == 12
    _sync()
    run(tok, ops, lambda i: streams[i % 3])
    for s in streams:
        s.synchronize()
    assert [tok.device_status_pos(s.cuda_stream)[0] for s in streams] == [capi.TD_OK] * 3
    check(ops, "alternating streams")


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------

def _growth_ops(golden, big, keep):
    """-> [(operation, is the large one)] * 15: small, large, small for each of the five families, inputs uploaded."""
    from tokendagger_amd import capi
    import minhash_truth as mt
    import nfc_truth as nt
    import pack_truth as pt
    import textstats_truth as tt

    def up(a, dt, **kw):
        t, p = cc.up(a, dt, **kw)
        keep.append(t)
        return p
    ALL = tt.LOCAL | tt.RUNS
    out = []
    smalls = [_small(golden, lo, 30) for lo in (40, 300)]
    assert all(200 < len(s[0]) < 4000 and len(s[2][0]) > 50 for s in smalls)
    etext, eoffs, ewant = big["encode"]
    for text, offs, want in (smalls[0], (etext, eoffs, ewant), smalls[1]):
        out.append((cc.Encode(up(text, np.uint8), len(text), up(offs, np.int64), len(offs) - 1, want), len(text) > 4000))
    nsmall = [nt.batch([nt.mixed(300 + 7 * i, "NFD"), b"", nt.mixed(90, "NFC")]) for i in range(2)]
    for text, offs, want in ((*nsmall[0], None), big["nfc"], (*nsmall[1], None)):
        want = want if want is not None else capi.nfc_host(text, offs)
        out.append((cc.Nfc(up(text, np.uint8, front=16, back=16, pad=0x41), len(text), up(offs, np.int64), len(offs) - 1, want), len(text) > 4000))
    btext, boffs, bwant = big["stats"]
    for text, offs, want in ((smalls[0][0], smalls[0][1], None), (btext, boffs, bwant[ALL]), (smalls[1][0], smalls[1][1], None)):
        want = want if want is not None else tt.truth(text, offs)
        out.append((cc.TextStats(up(text, np.uint8, front=16, back=16, pad=0x61), len(text), up(offs, np.int64), len(offs) - 1, ALL, want), len(text) > 4000))
    ids, toffs = big["ids"]
    for i, perm, w in ((0, 16, None), (None, PERM, big["minhash"]), (1, 16, None)):
        x, o = (ids, toffs) if i is None else smalls[i][2]
        w = w if w is not None else mt.minhash_numpy(x, o, K, perm, 3, 0, 0)
        out.append((cc.Minhash(up(x, np.int32), len(x), up(o, np.int64), len(o) - 1, K, perm, 3, 0, 0, w), i is None))
    for i, w in ((0, None), (None, big["pack"]), (1, None)):
        x, o = (ids, toffs) if i is None else smalls[i][2]
        w = w if w is not None else pt.pack_runs(x, o, 512, BOS, EOS, PAD, False)
        out.append((cc.PackRows(up(x, np.int32), len(x), up(o, np.int64), len(o) - 1, 512, BOS, EOS, PAD, w), i is None))
    assert len(out) == 15 and sum(large for _, large in out) == 5
    return out


@pytest.mark.parametrize("n_streams", [1, 2])
def test_workspace_growth_behind_a_call(tok, streams, golden, big_cases, n_streams):
    """A fresh clone whose every allocation is filled with 0xA5: each large call makes ensure replace buffers the small call in front of it
    was given (TD_INFO_WS_FILLED_BYTES rises across it), and the small call behind it runs on the new ones.  No host contact of the
    test's between the calls; with two streams the calls alternate."""
    from tokendagger_amd import capi
    tok.set_option(capi.TD_OPT_WS_FILL, 0xA5)
    try:
        t = tok.clone()
    finally:
        tok.set_option(capi.TD_OPT_WS_FILL, -1)
    try:
        keep = []
        ops = _growth_ops(golden, big_cases, keep)
        _sync()
        for i, (op, large) in enumerate(ops):
            before = t.info(capi.TD_INFO_WS_FILLED_BYTES)
            op.launch(t, streams[i % n_streams].cuda_stream)
            grown = t.info(capi.TD_INFO_WS_FILLED_BYTES) - before
            assert not large or grown > 0, f"call {i} ({op.name}): the large call replaced no buffer"
        for s in streams[:n_streams]:
            s.synchronize()
        assert [t.device_status_pos(s.cuda_stream)[0] for s in streams[:n_streams]] == [capi.TD_OK] * n_streams
        check([op for op, _ in ops], f"growth, {n_streams} stream(s)")
    finally:
        _sync()
        t.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------

def _error_chain(tok, streams, ops, first_bad, bad, want_pos, other_stream, again):
    """ops with the calls named in `bad` made bad; the calls behind the first bad one go to another stream if asked.  One status read at the
    end: the first bad call's code and position; then TD_OK; then `again`, one more good call."""
    from tokendagger_amd import capi
    at = [op.name for op in ops].index(BAD_NAME[first_bad])
    _sync()
    run(tok, ops, lambda i: streams[1] if other_stream and i > at else streams[0])
    last = streams[1] if other_stream else streams[0]
    assert tok.device_status_pos(last.cuda_stream) == (capi.TD_E_INVALID, want_pos)
    streams[0].synchronize()
    check(ops, ("error chain", bad, other_stream), bad=bad)
    assert tok.device_status_pos(last.cuda_stream)[0] == capi.TD_OK, "the error was not cleared by the read"
    assert tok.device_status_pos(streams[0].cuda_stream)[0] == capi.TD_OK
    again.launch(tok, last.cuda_stream)
    assert tok.device_status_pos(last.cuda_stream)[0] == capi.TD_OK
    again.check("the good call behind the error")


@pytest.mark.parametrize("other_stream", [False, True])
@pytest.mark.parametrize("bad", [("nfc",), ("text_stats",), ("nfc", "text_stats")])
def test_text_chain_keeps_the_first_unread_error(tok, streams, text_case, bad, other_stream):
    c, keep = text_case, []
    ops = text_chain(c, bad=bad, keep=keep)
    t, p = cc.up(c["nfc"][0], np.uint8, front=16, back=16, pad=0x41)
    t2, p2 = cc.up(c["nfc"][1], np.int64)
    keep += [t, t2]
    again = cc.Encode(p, len(c["nfc"][0]), p2, c["n_docs"], c["enc"])
    _error_chain(tok, streams, ops, bad[0], bad, c["bad_docs"][0 if bad[0] == "nfc" else 1], other_stream, again)


@pytest.mark.parametrize("other_stream", [False, True])
@pytest.mark.parametrize("bad", [("minhash",), ("minhash", "ngram")])
def test_token_chain_keeps_the_first_unread_error(tok, streams, token_case, nset, bad, other_stream):
    c, keep = token_case, []
    ops = token_chain(c, nset, seed=1, bad=bad, keep=keep)
    t, p = cc.up(c["sids"], np.int32)
    t2, p2 = cc.up(c["soffs"], np.int64)
    keep += [t, t2]
    again = cc.Minhash(p, c["T"], p2, c["kept"], K, PERM, 2, BANDS, ROWS, c["minhash"][2])
    _error_chain(tok, streams, ops, "minhash", bad, c["above"], other_stream, again)
