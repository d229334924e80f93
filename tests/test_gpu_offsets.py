"""Per-token start offsets on the GPU (td_token_starts*, td_encode_batch_with_starts, td_encode_device_with_starts, the Python
methods), through the C ABI, against the brute-force truth of tests/offsets_truth.py."""
import numpy as np
import pytest

import helpers as H
import offsets_truth as OT
import td_corpus

pytestmark = pytest.mark.gpu

AUTOGEN = r"[a-zA-Z]+|\s+|[0-9]+|[^\w\s]"  # the reference tests' own pattern: skips '_' and 'é'


@pytest.fixture(scope="module")
def vocab():
    pat, mr, special = H.llama4()
    table = OT.id_bytes(mr, special)
    return pat, mr, special, table, OT.id_lengths(table)


@pytest.fixture(scope="module")
def tok(vocab):
    from tokendagger_amd import capi
    return capi.HipTokenizer(vocab[0], vocab[1], vocab[2], device=0)


def _check_covered(t, text, offs, lengths, expect_ids=None, expect_offs=None):
    """Both units through the host entry against the covered truth; ids against td_encode_batch (or the given ones);
    td_token_starts on the same ids."""
    from tokendagger_amd import capi
    ids, toffs, sb = t.encode_batch_with_starts(text, offs, unit=capi.TD_UNIT_BYTES)
    if expect_ids is None:
        expect_ids, expect_offs = t.encode_batch(text, offs)
    assert np.array_equal(toffs, expect_offs) and np.array_equal(ids, expect_ids)
    truth_b = OT.covered_byte_starts(ids, toffs, lengths)
    assert np.array_equal(sb, truth_b)
    _, _, sc = t.encode_batch_with_starts(text, offs, unit=capi.TD_UNIT_CHARS)
    truth_c = OT.char_starts(text, offs, toffs, truth_b)
    assert np.array_equal(sc, truth_c)
    assert np.array_equal(t.token_starts(ids, toffs, capi.TD_UNIT_BYTES), truth_b)
    assert np.array_equal(t.token_starts(ids, toffs, capi.TD_UNIT_CHARS), truth_c)
    return ids, toffs, sb, sc


@pytest.mark.parametrize("fixture,pat", [("golden", None), ("tekken_golden", H.TEKKEN_PAT), ("cl100k_golden", H.CL100K_PAT),
                                         ("gpt2_golden", H.GPT2_PAT)])
def test_golden_patterns_both_units(request, golden, vocab, fixture, pat):
    from tokendagger_amd import capi
    g = request.getfixturevalue(fixture)  # (the other patterns' goldens are over the documents of llama4_golden.npz)
    t = capi.HipTokenizer(pat or vocab[0], vocab[1], vocab[2], device=0)
    _check_covered(t, golden["text"], golden["offsets"], vocab[4], g["enc"], g["enc_offsets"])
    t.close()


def test_code_files_and_qwen2(tok, vocab):
    from tokendagger_amd import capi, vocab_io
    g = np.load(H.ROOT / "tests" / "golden" / "code_corpus.npz", allow_pickle=False)
    _check_covered(tok, g["text"], g["offsets"], vocab[4], g["enc"], g["enc_offsets"])
    t = capi.HipTokenizer(vocab_io.QWEN2_PAT_STR, vocab[1], vocab[2], device=0)
    x, o = td_corpus.mixed(4 << 20, seed=5)
    _check_covered(t, x, o, vocab[4])
    t.close()


@pytest.mark.parametrize("kind", ["english", "mixed"])
def test_64_mib(tok, vocab, kind):
    x, o = getattr(td_corpus, kind)(64 << 20, seed=11)
    _check_covered(tok, x, o, vocab[4])


def _autogen_docs():
    rng = np.random.default_rng(3)
    words = ["snake_case", "é", "_", "__init__", "naïve", "café", "x", "42", "!", " ", "\n", "émigré", "_é_", "中文", "\U0001F600"]
    docs = ["_leading gap", "middle_gap here", "trailing gap_", "___", "", "é", "", "plain text 1 2 3"]
    for n in (100, 5000, 20000):  # documents over many 4 KiB tiles and 4096-id chunks
        docs.append("".join(words[i] + (" " if i % 3 else "") for i in rng.integers(0, len(words), n)))
    return [d.encode("utf-8") for d in docs]


def _generic_truth(docs, ids, toffs, lengths):
    out = []
    for d, doc in enumerate(docs):
        st, en = OT.split_arrays(AUTOGEN, doc)
        out.append(OT.generic_byte_starts(st, en, ids[toffs[d]:toffs[d + 1]], lengths, len(doc)))
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def test_autogen_gaps_host_and_device(vocab):
    import torch
    from tokendagger_amd import capi
    t = capi.HipTokenizer(AUTOGEN, vocab[1], vocab[2], device=0)
    docs = _autogen_docs()
    text, offs = H.pack_docs(docs)
    ids, toffs, sb = t.encode_batch_with_starts(text, offs, unit=capi.TD_UNIT_BYTES)
    eids, eoffs = t.encode_batch(text, offs)
    assert np.array_equal(ids, eids) and np.array_equal(toffs, eoffs)
    truth = _generic_truth(docs, ids, toffs, vocab[4])
    assert not np.array_equal(truth, OT.covered_byte_starts(ids, toffs, vocab[4])), "the documents must skip text"
    assert np.array_equal(sb, truth)
    _, _, sc = t.encode_batch_with_starts(text, offs, unit=capi.TD_UNIT_CHARS)
    assert np.array_equal(sc, OT.char_starts(text, offs, toffs, truth))
    # the device entry equals the host entry
    n = len(text)
    d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    d_offs = torch.from_numpy(np.asarray(offs, dtype=np.int64)).cuda()
    for unit, want in ((capi.TD_UNIT_BYTES, sb), (capi.TD_UNIT_CHARS, sc)):
        d_tok = torch.empty(n, dtype=torch.int32, device="cuda")
        d_toff = torch.empty(len(offs), dtype=torch.int64, device="cuda")
        d_st = torch.empty(n, dtype=torch.int64, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        t.encode_device_with_starts(d_text.data_ptr(), n, d_offs.data_ptr(), len(offs) - 1, d_tok.data_ptr(), n, d_toff.data_ptr(),
                                    d_st.data_ptr(), unit, s)
        t.device_status(s)
        k = int(d_toff[-1])
        assert np.array_equal(d_toff.cpu().numpy(), toffs)
        assert np.array_equal(d_tok[:k].cpu().numpy(), ids)
        assert np.array_equal(d_st[:k].cpu().numpy(), want)
    t.close()


def test_autogen_64_mib_single_document(vocab):
    from tokendagger_amd import capi
    t = capi.HipTokenizer(AUTOGEN, vocab[1], vocab[2], device=0)
    x, _ = td_corpus.code(64 << 20, seed=2)
    doc = x.tobytes()
    offs = np.asarray([0, len(doc)], dtype=np.int64)
    ids, toffs, sb = t.encode_batch_with_starts(doc, offs, unit=capi.TD_UNIT_BYTES)
    eids, _ = t.encode_batch(doc, offs)
    assert np.array_equal(ids, eids)
    truth = OT.generic_byte_starts(*OT.split_arrays(AUTOGEN, doc), ids, vocab[4], len(doc))
    assert np.array_equal(sb, truth)
    _, _, sc = t.encode_batch_with_starts(doc, offs, unit=capi.TD_UNIT_CHARS)
    assert np.array_equal(sc, OT.char_starts(doc, offs, toffs, truth))
    t.close()


def test_allowed_specials_host_entry(tok, vocab):
    from tokendagger_amd import capi
    special = vocab[2]
    names = sorted(special)[:3]
    docs = [f"{names[0]}hello é{names[1]} world{names[0]}", "no specials here", "", f"中文{names[2]}\U0001F600 x",
            names[1] * 3]
    docs = [d.encode("utf-8") for d in docs]
    text, offs = H.pack_docs(docs)
    eids, eoffs = tok.encode_batch_with_special_strs(text, offs, names)
    ids, toffs, sb = tok.encode_batch_with_starts(text, offs, allowed=names, unit=capi.TD_UNIT_BYTES)
    assert np.array_equal(ids, eids) and np.array_equal(toffs, eoffs)
    assert any(int(i) in special.values() for i in ids)
    truth = OT.covered_byte_starts(ids, toffs, vocab[4])
    assert np.array_equal(sb, truth)
    _, _, sc = tok.encode_batch_with_starts(text, offs, allowed=names, unit=capi.TD_UNIT_CHARS)
    assert np.array_equal(sc, OT.char_starts(text, offs, toffs, truth))
    # a generic pattern that skips text, behind special tokens
    t = capi.HipTokenizer(AUTOGEN, vocab[1], vocab[2], device=0)
    docs = [f"a_b{names[0]}_c d_{names[1]}é_", "x_y"]
    docs = [d.encode("utf-8") for d in docs]
    text, offs = H.pack_docs(docs)
    ids, toffs, sb = t.encode_batch_with_starts(text, offs, allowed=names, unit=capi.TD_UNIT_BYTES)
    eids, _ = t.encode_batch_with_special_strs(text, offs, names)
    assert np.array_equal(ids, eids)
    table = vocab[3]
    for d, doc in enumerate(docs):  # every token's bytes stand at its start, in order
        prev = -1
        for k in range(toffs[d], toffs[d + 1]):
            b = table[ids[k]]
            assert doc[sb[k]:sb[k] + len(b)] == b and sb[k] > prev
            prev = sb[k]
    _, _, sc = t.encode_batch_with_starts(text, offs, allowed=names, unit=capi.TD_UNIT_CHARS)
    assert np.array_equal(sc, OT.char_starts(text, offs, toffs, sb))
    t.close()


def test_token_starts_errors_and_device_form(tok, vocab):
    import torch
    from tokendagger_amd import capi
    bad = np.asarray([1, 2, 10 ** 8, 5, -1], dtype=np.int32)
    with pytest.raises(capi.TokenDaggerHipError) as e:
        tok.token_starts(bad)
    assert e.value.code == capi.TD_E_BAD_TOKEN and "index 2" in str(e.value)
    with pytest.raises(capi.TokenDaggerHipError) as e:
        tok.token_starts(np.asarray([1, 2, 3], dtype=np.int32), np.asarray([0, 5], dtype=np.int64), n_tokens=3)
    assert e.value.code == capi.TD_E_CAPACITY
    assert list(tok.token_starts(np.asarray([1, 2, 3], dtype=np.int32))) == [0, 1, 2]
    s = torch.cuda.current_stream().cuda_stream
    d_ids = torch.from_numpy(bad).cuda()
    d_to = torch.tensor([0, 5], dtype=torch.int64, device="cuda")
    d_out = torch.empty(5, dtype=torch.int64, device="cuda")
    tok.token_starts_device(d_ids.data_ptr(), 5, d_to.data_ptr(), 1, d_out.data_ptr(), capi.TD_UNIT_BYTES, s)
    with pytest.raises(capi.TokenDaggerHipError) as e:
        tok.device_status(s)
    assert e.value.code == capi.TD_E_BAD_TOKEN and "index 2" in str(e.value)
    d_to = torch.tensor([0, 9], dtype=torch.int64, device="cuda")
    good = torch.tensor([1, 2, 3, 4, 5], dtype=torch.int32, device="cuda")
    tok.token_starts_device(good.data_ptr(), 5, d_to.data_ptr(), 1, d_out.data_ptr(), capi.TD_UNIT_BYTES, s)
    with pytest.raises(capi.TokenDaggerHipError) as e:
        tok.device_status(s)
    assert e.value.code == capi.TD_E_CAPACITY
    # the device form on a real batch
    x, o = td_corpus.english(2 << 20, seed=4)
    ids, toffs = tok.encode_batch(x, o)
    d_ids = torch.from_numpy(ids.copy()).cuda()
    d_to = torch.from_numpy(toffs.copy()).cuda()
    d_out = torch.empty(len(ids), dtype=torch.int64, device="cuda")
    for unit in (capi.TD_UNIT_BYTES, capi.TD_UNIT_CHARS):
        tok.token_starts_device(d_ids.data_ptr(), len(ids), d_to.data_ptr(), len(toffs) - 1, d_out.data_ptr(), unit, s)
        tok.device_status(s)
        assert np.array_equal(d_out.cpu().numpy(), tok.token_starts(ids, toffs, unit))


def test_clone_handle(tok, vocab):
    from tokendagger_amd import capi
    c = tok.clone()
    x, o = td_corpus.mixed(1 << 20, seed=8)
    a = tok.encode_batch_with_starts(x, o, unit=capi.TD_UNIT_CHARS)
    b = c.encode_batch_with_starts(x, o, unit=capi.TD_UNIT_CHARS)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    c.close()


def test_python_methods(vocab):
    import tokendagger as tiktoken
    pat, mr, special, table, _ = vocab
    enc = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    eot = sorted(special)[0]
    for s in ["Hello, world! 你好世界 \U0001F30D\U0001F600 naïve café", "中文文本和emoji \U0001F468‍\U0001F469 mixed",
              "", "plain", f"a{eot}b 中"]:
        ids, starts = enc.encode_with_offsets(s, allowed_special="all")
        assert ids == enc.encode(s, allowed_special="all")
        tb = enc.decode_tokens_bytes(ids)
        b_starts = np.concatenate([[0], np.cumsum([len(b) for b in tb])])[:-1] if ids else []
        data = s.encode("utf-8")
        for k in range(len(ids)):
            on_boundary = (data[b_starts[k]] & 0xC0) != 0x80
            end_ok = k + 1 == len(ids) or (data[b_starts[k + 1]] & 0xC0) != 0x80
            if on_boundary and end_ok:
                end = starts[k + 1] if k + 1 < len(ids) else len(s)
                assert s[starts[k]:end] == tb[k].decode("utf-8"), (s, k)
        assert starts == OT.decode_offsets_rule(tb) if ids else starts == []
        text, offs = enc.decode_with_offsets(ids)
        assert text == s and offs == OT.decode_offsets_rule(tb)
        bids, bstarts = enc.encode_with_offsets(data, allowed_special="all")
        assert bids == ids and list(bstarts) == [int(v) for v in b_starts]
    with pytest.raises(ValueError):
        enc.encode_with_offsets(f"x{eot}", disallowed_special="all")  # the same check as encode
    # a token that splits a 4-byte character: decode_with_offsets points at the character
    emoji = "\U0001F600".encode("utf-8")
    parts = [mr[bytes([c])] for c in emoji if bytes([c]) in mr]
    if len(parts) == 4:
        _, offs = enc.decode_with_offsets([mr[b"a"]] + parts)
        assert offs == OT.decode_offsets_rule([b"a"] + [bytes([c]) for c in emoji])
    x, o = td_corpus.english(1 << 20, seed=1)
    ids, toffs, st = enc.encode_batch_to_numpy_with_offsets(x, o, unit="bytes")
    eids, eoffs = enc.encode_batch_to_numpy(x, o)
    assert np.array_equal(ids, eids) and np.array_equal(toffs, eoffs)
    assert np.array_equal(st, OT.covered_byte_starts(ids, toffs, OT.id_lengths(table)))
