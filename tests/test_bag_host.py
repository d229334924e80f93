"""td_bag_classify_host, the rule's executable statement, against the rule in plain Python (tests/bag_truth.py) on the seam cases the GPU
test uses; every create error with its position, which writes nothing; the tree against hand-written ones."""
import numpy as np
import pytest

import bag_truth as bt

MODELS, CASES = bt.models(), bt.seam_cases()
TRUTH = {}


def truth(name):
    if name not in TRUTH:
        text, offs, model, eos = CASES[name]
        TRUTH[name] = bt.classify(MODELS[model], text, offs, eos)
    return TRUTH[name]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build_hip()
    from tokendagger_amd import capi
    return capi


def spec_of(capi, m, **over):
    kw = dict(bucket=m["bucket"], minn=m["minn"], maxn=m["maxn"], word_ngrams=m["word_ngrams"], loss=m["loss"], label_counts=m["counts"])
    kw.update(over)
    return capi.BagSpec(m["words"], m["input"], m["output"], **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_seam_cases(capi, name):
    text, offs, model, eos = CASES[name]
    bt.same(capi.bag_classify_host(spec_of(capi, MODELS[model]), text, offs, capi.TD_BAG_EOS if eos else 0), truth(name), name)


def test_best_is_decided_in_nine_documents_of_ten():
    sure = np.concatenate([truth(n)["sure"] for n in CASES])
    print("largest relative tolerance:", max(float(truth(n)["rel"].max()) for n in CASES))
    assert sure.mean() >= 0.9


W3 = [b"a", b"b", b"c"]
BAD = {  # name -> (words, the parameters changed, the position reported)
    "an empty word": ([b"a", b"", b"c"], {}, 1),
    "a word with a delimiter": ([b"a", b"b", b"c\x00d"], {}, 2),
    "a duplicate: the second one": ([b"a", b"b", b"c", b"b", b"a"], {}, 3),
    "the lowest of two faults": ([b"a", b"a", b""], {}, 1),
    "dim 513": (W3, {"dim": 513}, -1),
    "no label": (W3, {"n_labels": 0}, -1),
    "4097 labels": (W3, {"n_labels": 4097}, -1),
    "one label under hs": (W3, {"n_labels": 1, "loss": 2}, -1),
    "minn above maxn": (W3, {"minn": 3, "maxn": 2}, -1),
    "minn 0 with maxn 2": (W3, {"minn": 0, "maxn": 2}, -1),
    "maxn 9": (W3, {"minn": 1, "maxn": 9}, -1),
    "word_ngrams 0": (W3, {"word_ngrams": 0}, -1),
    "word_ngrams 6": (W3, {"word_ngrams": 6}, -1),
    "a negative bucket": (W3, {"bucket": -1}, -1),
    "bucket 0 with bigrams": (W3, {"bucket": 0, "word_ngrams": 2}, -1),
    "bucket 0 with character n-grams": (W3, {"bucket": 0, "minn": 1, "maxn": 1}, -1),
    "an unknown loss": (W3, {"loss": 3}, -1),
    "counts that increase": (W3, {"n_labels": 3, "loss": 2, "counts": [5, 6, 1]}, -1),
}


@pytest.mark.parametrize("name", list(BAD))
def test_model_errors_name_the_word_and_write_nothing(capi, name):
    words, over, pos = BAD[name]
    m = bt.make_model(0, words, 2, 3, bt.SOFTMAX, 5)
    over = dict(over)
    counts = over.pop("counts", None)
    spec = capi.BagSpec(words, m["input"], np.zeros((8, 2), np.float32), bucket=5, label_counts=counts)
    for k, v in over.items():
        setattr(spec.params, k, v)
    text, offs = np.frombuffer(b"a b c", dtype=np.uint8), np.array([0, 5], dtype=np.int64)
    outs = [np.full(8, 0x77, np.uint8).view(t) for t in (np.int32, np.float32)] + [np.full(64, 0x77, np.uint8) for _ in range(4)]
    got = capi.ctypes.c_int64(7)
    rc = capi.load_library().td_bag_classify_host(*spec.args(), text.ctypes.data, offs.ctypes.data, 1, 1, *(x.ctypes.data for x in outs), capi.ctypes.byref(got))
    assert (rc, got.value) == (capi.TD_E_INVALID, pos)
    assert all((x.view(np.uint8) == 0x77).all() for x in outs)


def test_a_word_above_1024_bytes_is_accepted_and_never_matches(capi):
    m = bt.make_model(9, [b"a", b"x" * 1025], 4, 2, bt.SOFTMAX, 3, word_ngrams=2)
    text = b"a " + b"x" * 1025 + b" a"
    bt.same(capi.bag_classify_host(spec_of(capi, m), text, [0, len(text)]), bt.classify(m, text, [0, len(text)]), "a long word")


HAND = {  # counts -> per label (path, code), leaf to root, written out by hand from fastText's buildTree
    (5, 3, 1, 1): [([2], [1]), ([1, 2], [1, 0]), ([0, 1, 2], [1, 0, 0]), ([0, 1, 2], [0, 0, 0])],
    (2, 2, 2, 2): [([1, 2], [1, 1]), ([1, 2], [0, 1]), ([0, 2], [1, 0]), ([0, 2], [0, 0])],
}


@pytest.mark.parametrize("counts", list(HAND))
def test_the_tree_against_a_hand_written_one(capi, counts):
    """dim = the tree's three nodes, the output layer 20 * identity, one word whose row is +-1 along a label's path: that label gets
    all the probability exactly when the library's tree is the hand-written one"""
    assert [(list(p), [int(c) for c in code]) for p, code in bt.tree(list(counts))] == HAND[counts]
    for label, (path, code) in enumerate(HAND[counts]):
        row = np.zeros((1, 3), np.float32)
        for k, c in zip(path, code):
            row[0, k] = 1 if c else -1
        spec = capi.BagSpec([b"w"], row, 20 * np.eye(3, dtype=np.float32), bucket=0, loss=capi.TD_BAG_HS, label_counts=list(counts))
        got = capi.bag_classify_host(spec, b"w", [0, 1], 0)
        assert got["best"][0] == label and got["best_prob"][0] > 0.999, (counts, label, got["probs"])


@pytest.mark.parametrize("rows, cols, counts", [(3 + 4, 2, None), (3 + 5, 3, None), (3 + 5, 2, [3, 2, 1])])
def test_shapes_that_do_not_fit_one_another_are_refused_before_the_library(capi, rows, cols, counts):
    with pytest.raises(ValueError):
        capi.BagSpec(W3, np.zeros((rows, 2), np.float32), np.zeros((3, cols), np.float32), bucket=5,
                     loss=capi.TD_BAG_HS if counts else capi.TD_BAG_SOFTMAX, label_counts=counts)
