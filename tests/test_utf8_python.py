"""The Python surface of the UTF-8 repair: capi.utf8_host and the argument checks without a GPU; Tokenizer.validate_batch, repair_batch and
encode_batch_to_numpy_repaired against the interpreter's codec on one."""
import numpy as np
import pytest

import helpers as H
import utf8_truth as ut
from tokendagger_amd import capi
from tokendagger_amd.capi import utf8_host  # noqa: F401  (the feature under test: without it nothing here runs)

DOCS = ["naïve café".encode(), b"plain", "€".encode()[:2], b"\x80\x80abc", b"", "日本語 😀".encode() + b"\xf0\x9f", b"\xed\xa0\x80", b"\xc0\xaf"]


def test_utf8_host():
    text, offs = ut.batch(DOCS)
    for policy, errors in ((capi.TD_UTF8_REPLACE, "replace"), (capi.TD_UTF8_IGNORE, "ignore")):
        out, ooff, flags, first, nbad, counts = utf8_host(text, offs, policy)
        want = [d.decode("utf-8", errors).encode() for d in DOCS]
        assert bytes(out) == b"".join(want) and ooff.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
        assert flags.tolist() == [0, 0, 1, 1, 0, 1, 1, 1] and first.tolist() == [-1, -1, 0, 0, -1, 14, 0, 0] and nbad.tolist() == [0, 0, 1, 2, 0, 1, 3, 2]
        assert counts.tolist() == [len(b"".join(want)), 5, 9, 11, 1, 2, 0, 0]
    assert utf8_host(text, offs, want_text=False)[0] is None


def test_bad_errors_argument():
    import tokendagger as tiktoken
    t = object.__new__(tiktoken.Tokenizer)
    for call in (lambda: t.repair_batch(b"", [0], errors="strict"), lambda: t.encode_batch_to_numpy_repaired(b"", [0], errors="surrogateescape"),
                 lambda: t.repair_batch(b"", [0], errors=None)):
        with pytest.raises(ValueError):
            call()


@pytest.fixture(scope="module")
def enc():
    import tokendagger as tiktoken
    pat, mr, special = H.llama4()
    return tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)


@pytest.mark.gpu
def test_validate_repair_and_repaired_encode(enc):
    text, offs = ut.batch(DOCS * 3 + [ut.filler(5000), ("Привет " * 900).encode()[:-1]])
    docs = ut.docs_of(text, offs)
    v = enc.validate_batch(text, offs)
    assert v.flags.tolist() == [int(d.decode("utf-8", "ignore").encode() != d) for d in docs]
    assert np.array_equal(v.first_bad, utf8_host(text, offs)[3]) and v.counts[1] == v.flags.sum()
    for errors in ("replace", "ignore"):
        want = [d.decode("utf-8", errors).encode() for d in docs]
        r = enc.repair_batch(text, offs, errors=errors)
        assert bytes(r.text) == b"".join(want) and r.offsets.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
        host = utf8_host(text, offs, capi.TD_UTF8_REPLACE if errors == "replace" else capi.TD_UTF8_IGNORE)
        assert np.array_equal(r.flags, host[2]) and np.array_equal(r.first_bad, host[3]) and np.array_equal(r.n_bad, host[4])
        assert np.array_equal(r.counts, host[5])
        assert bytes(enc.repair_batch(bytes(text), offs, errors).text) == b"".join(want)
        wi, wo = enc.encode_batch_to_numpy(np.frombuffer(b"".join(want), dtype=np.uint8), r.offsets)
        ids, toff = enc.encode_batch_to_numpy_repaired(text, offs, errors=errors)
        assert np.array_equal(ids, wi) and np.array_equal(toff, wo)
        ids, toff, fixed = enc.encode_batch_to_numpy_repaired(text, offs, errors=errors, ordinary=True, return_text=True)
        assert np.array_equal(ids, wi) and bytes(fixed.text) == b"".join(want) and np.array_equal(fixed.offsets, r.offsets)
        assert np.array_equal(fixed.n_bad, host[4])
        # repaired text checks clean, and goes to the other bulk methods as it stands
        again = enc.validate_batch(r.text, r.offsets)
        assert not again.flags.any() and (again.first_bad == -1).all()
        n = enc.normalize_batch(r.text, r.offsets)
        assert bytes(n.text) == bytes(r.text)
    with pytest.raises(ValueError):
        enc.repair_batch(text, offs, errors="backslashreplace")
