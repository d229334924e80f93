"""The Python surface of the NFC normalisation: capi.nfc_host and the argument checks without a GPU; Tokenizer.normalize_batch,
encode_batch_to_numpy_normalized and the `normalizer` option of Tokenizer / Encoding on one."""
import numpy as np
import pytest

import helpers as H
import nfc_truth as nt
from tokendagger_amd import capi, vocab_io
from tokendagger_amd.capi import nfc_host  # noqa: F401  (the feature under test: without it nothing here runs)

E_ACUTE_NFD, E_ACUTE_NFC = nt.U(0x65, 0x301).decode(), nt.U(0xE9).decode()


def test_nfc_host():
    text, offs = nt.batch([E_ACUTE_NFD.encode(), b"plain", nt.U(0x212B), nt.U(0x301), b"\xff" + nt.U(0x301)])
    out, ooff, flags, changed, counts = nfc_host(text, offs)
    assert bytes(out) == E_ACUTE_NFC.encode() + b"plain" + nt.U(0xC5) + nt.U(0x301) + b"\xff" + nt.U(0x301)
    assert ooff.tolist() == [0, 2, 7, 9, 11, 14] and flags.tolist() == [1, 0, 1, 1, 1] and changed.tolist() == [1, 0, 1, 0, 0]
    assert counts.tolist() == [14, 4, 2, 4, 5, 1, 2, 0]
    assert nfc_host(text, offs, want_text=False)[0] is None
    assert vocab_io.QWEN2_NORMALIZER == "NFC"


def test_bad_form_and_bad_normalizer():
    import tokendagger as tiktoken
    pat, mr, special = H.llama4()
    with pytest.raises(ValueError):
        tiktoken.Encoding(name="x", pat_str=pat, mergeable_ranks=mr, special_tokens=special, normalizer="NFKC")
    with pytest.raises(ValueError):
        tiktoken.Tokenizer("x", pat_str=pat, mergeable_ranks=mr, normalizer="nfc")
    with pytest.raises(ValueError):
        tiktoken.Tokenizer.normalize_batch(object.__new__(tiktoken.Tokenizer), b"", [0], form="NFD")


@pytest.fixture(scope="module")
def encs():
    import tokendagger as tiktoken
    pat, mr, special = H.llama4()
    plain = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    nfc = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special, normalizer=vocab_io.QWEN2_NORMALIZER)
    return plain, nfc


@pytest.mark.gpu
def test_normalizer_option(encs):
    plain, nfc = encs
    assert plain.normalizer is None and nfc.normalizer == "NFC"
    want = plain.encode(E_ACUTE_NFC)
    assert nfc.encode(E_ACUTE_NFD) == want and plain.encode(E_ACUTE_NFD) != want
    s = "caf" + E_ACUTE_NFD + " " + nt.U(0x1112, 0x1161, 0x11AB).decode() + " plain"
    t = nt.nfc_by_runs(s.encode()).decode() if nt.UNICODE_VERSION == capi.nfc_info(0) else nfc_host(s.encode(), [0, len(s.encode())])[0].tobytes().decode()
    assert t != s
    assert nfc.encode_ordinary(s) == plain.encode_ordinary(t) and nfc.encode_with_special_tokens(s) == plain.encode_with_special_tokens(t)
    assert nfc.encode_batch([s, "x", s]) == plain.encode_batch([t, "x", t]) and nfc.encode_ordinary_batch([s]) == plain.encode_ordinary_batch([t])
    assert np.array_equal(nfc.encode_to_numpy(s), plain.encode_to_numpy(t)) and np.array_equal(nfc.encode_to_numpy(s.encode()), plain.encode_to_numpy(t))
    # normalizer=None gives today's ids
    assert plain.encode(s) == plain.encode_ordinary(s) and plain.encode(s) != plain.encode(t)
    assert nfc.decode(nfc.encode(s)) == t


@pytest.mark.gpu
def test_normalize_batch_and_normalized_encode(encs):
    plain, _ = encs
    text, offs = nt.batch([nt.mixed(5000, "NFD"), b"plain text", b"", nt.mixed(100, "NFC")])
    want = nfc_host(text, offs)
    got = plain.normalize_batch(text, offs)
    assert bytes(got.text) == bytes(want[0]) and np.array_equal(got.offsets, want[1]) and np.array_equal(got.flags, want[2])
    assert np.array_equal(got.changed, want[3]) and np.array_equal(got.counts, want[4])
    got = plain.normalize_batch(bytes(text), offs, form="NFC")
    assert bytes(got.text) == bytes(want[0])
    ids, toff = plain.encode_batch_to_numpy_normalized(text, offs)
    wi, wo = plain.encode_batch_to_numpy(want[0], want[1])
    assert np.array_equal(ids, wi) and np.array_equal(toff, wo)
    ids, toff, norm = plain.encode_batch_to_numpy_normalized(text, offs, ordinary=True, return_text=True)
    assert np.array_equal(ids, wi) and bytes(norm.text) == bytes(want[0]) and np.array_equal(norm.offsets, want[1])
    assert np.array_equal(norm.changed, want[3])
    # the other bulk methods take the normalised text as it stands
    _, total = plain.encode_batch_to_minhash(got.text, got.offsets)
    assert total == len(wi)
    with pytest.raises(ValueError):
        plain.normalize_batch(text, offs, form="NFKC")
