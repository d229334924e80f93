"""Bag models on the GPU (td_bag_classify_device, td_bag_classify, Tokenizer.classify) against the rule in plain Python
(tests/bag_truth.py): stats, totals and hidden must be EQUAL, the probabilities within the tolerance derived there, best equal wherever
the reference decides it.  The outputs lie in buffers filled with 0x77 that are longer than the call may write."""
import numpy as np
import pytest

import bag_truth as bt
import helpers as H

pytestmark = pytest.mark.gpu

FILL, SLACK = 0x77, 9
MODELS, CASES = bt.models(), bt.seam_cases()


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
def model(tok):
    """name -> the model on the device, made once"""
    from tokendagger_amd import capi
    memo = {}

    def get(name):
        if name not in memo:
            m = MODELS[name]
            memo[name] = tok.bag_model(capi.BagSpec(m["words"], m["input"], m["output"], bucket=m["bucket"], minn=m["minn"], maxn=m["maxn"],
                                                    word_ngrams=m["word_ngrams"], loss=m["loss"], label_counts=m["counts"]))
        return memo[name]
    return get


@pytest.fixture(scope="module")
def truth():
    memo = {}

    def get(name):
        if name not in memo:
            text, offs, mname, eos = CASES[name]
            memo[name] = bt.classify(MODELS[mname], text, offs, eos)
        return memo[name]
    return get


def call(tok, stream, bm, text, offs, eos, shift=0, want=True, n_bytes=None):
    """One td_bag_classify_device call on `stream`, the text `shift` bytes off the 16-byte grid -> (the results, the slack behind every
    output is untouched, the whole buffers)"""
    import torch
    dev = torch.device("cuda", 0)
    text, offs = np.frombuffer(bytes(text), dtype=np.uint8), np.asarray(offs, dtype=np.int64)
    n, L, dim = len(offs) - 1, bm.n_labels, bm.dim
    sizes = {"best": (n, torch.int32), "best_prob": (n, torch.float32), "probs": (n * L, torch.float32), "hidden": (n * dim, torch.float32),
             "stats": (4 * n, torch.int64), "totals": (4, torch.int64)}
    with torch.cuda.stream(stream):
        raw = torch.from_numpy(np.concatenate([np.full(16 + shift, 0x74, np.uint8), text, np.full(16, 0x65, np.uint8)])).to(dev)
        d_offs = torch.from_numpy(offs).to(dev)
        bufs = {k: torch.full(((m + SLACK) * dt.itemsize,), FILL, dtype=torch.uint8, device=dev).view(dt) for k, (m, dt) in sizes.items()}
    ptr = lambda k: bufs[k].data_ptr() if want or k in ("best", "best_prob", "stats") else 0  # noqa: E731
    tok.bag_classify_device(bm, raw.data_ptr() + 16 + shift, len(text) if n_bytes is None else n_bytes, d_offs.data_ptr(), n, 1 if eos else 0,
                            ptr("best"), ptr("best_prob"), ptr("probs"), ptr("hidden"), ptr("stats"), ptr("totals"), stream.cuda_stream)
    stream.synchronize()
    whole = {k: v.cpu().numpy() for k, v in bufs.items()}
    slack = all((whole[k][m:].view(np.uint8) == FILL).all() for k, (m, _) in sizes.items())
    got = {k: whole[k][:m] for k, (m, _) in sizes.items()}
    got["probs"], got["hidden"], got["stats"] = got["probs"].reshape(n, L), got["hidden"].reshape(n, dim), got["stats"].reshape(n, 4)
    return got, slack, whole


# every case, off the 16-byte grid by 0, 1 and 15 bytes
@pytest.mark.parametrize("name, shift", [(n, s) for n in CASES for s in (0, 1, 15)])
def test_seam_cases(tok, side, model, truth, name, shift):
    from tokendagger_amd import capi
    text, offs, mname, eos = CASES[name]
    got, slack, _ = call(tok, side, model(mname), text, offs, eos, shift)
    assert tok.device_status_pos(side.cuda_stream) == (capi.TD_OK, 0)
    bt.same(got, truth(name), (name, shift))
    assert slack


def test_two_calls_give_the_same_bits(tok, side, model):
    name = "a document of many chunks"
    text, offs, mname, eos = CASES[name]
    first, second = (call(tok, side, model(mname), text, offs, eos, 5)[2] for _ in range(2))
    assert all(np.array_equal(first[k].view(np.uint8), second[k].view(np.uint8)) for k in first)


def test_without_probs_hidden_and_totals(tok, side, model, truth):
    name = "fewer tokens than N"
    text, offs, mname, eos = CASES[name]
    got, _, whole = call(tok, side, model(mname), text, offs, eos, want=False)
    assert np.array_equal(got["stats"], truth(name)["stats"])
    assert all((whole[k].view(np.uint8) == FILL).all() for k in ("probs", "hidden", "totals"))


@pytest.mark.parametrize("offs, n_bytes, bad", [([0, 30, 20, 10, 40], 40, 1), ([1, 10, 40], 40, 0), ([0, 10, 50], 40, 1), ([0, -1, 40], 40, 0)])
def test_bad_offsets_write_nothing(tok, side, model, offs, n_bytes, bad):
    from tokendagger_amd import capi
    whole = call(tok, side, model("one"), b"the " * 16, offs, True, n_bytes=n_bytes)[2]
    assert tok.device_status_pos(side.cuda_stream) == (capi.TD_E_INVALID, bad)
    assert all((x.view(np.uint8) == FILL).all() for x in whole.values())


def test_the_host_buffer_call_and_the_tokenizer(tok, truth):
    import tokendagger as tiktoken
    name = "a literal </s>, a word"
    text, offs, mname, eos = CASES[name]
    m = MODELS[mname]
    pat, mr, special = H.llama4()
    tk = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    labels = ["__label__%d" % i for i in range(m["n_labels"])]
    with tk.bag_model(m["words"], m["input"], m["output"], bucket=m["bucket"], minn=m["minn"], maxn=m["maxn"], word_ngrams=m["word_ngrams"],
                      loss="hs", label_counts=m["counts"], labels=labels) as bm:
        assert bm.info["eos_index"] == m["index"][bt.EOS] and bm.info["tree_depth"] == max(len(p) for p, _ in bt.tree(m["counts"]))
        res = tk.classify(text, np.asarray(offs, dtype=np.int64), bm, probs=True, hidden=True)
    want = truth(name)
    bt.same({k: getattr(res, k) for k in ("best", "best_prob", "probs", "hidden", "stats", "totals")}, want, "Tokenizer.classify")
    assert res.features.tolist() == want["stats"][:, 2].tolist()
    assert res.mask(labels[int(res.best[0])], 0.0).tolist() == [True] and not res.mask(int(res.best[0]), 2.0).any()
