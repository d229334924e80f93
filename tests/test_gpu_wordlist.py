"""Word-list matches on the GPU (td_word_matches_device, td_word_matches, Tokenizer.word_matches) against the rule in plain Python
(tests/wordlist_truth.py): stats, totals and entry hits must be EQUAL.  The outputs lie in buffers filled with 0x77 that are longer than
the call may write.  No case here makes the device fault: every error is one the library reports by a status code."""
import random

import numpy as np
import pytest

import helpers as H
import wordlist_truth as wt

pytestmark = pytest.mark.gpu

FILL, SLACK = 0x77, 9
CASES = wt.seam_cases()
BIG = "a set above the LDS budget"


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
def case(tok):
    """name -> (the case's word set, the truth's answer), made once a case and left unchanged"""
    memo = {}

    def get(name):
        if name not in memo:
            text, offs, entries, groups, flags = CASES[name]
            memo[name] = tok.word_set(entries, groups, flags), wt.matches(text, offs, entries, groups, flags)
        return memo[name]
    return get


class Call:
    """One td_word_matches_device call enqueued on `stream`, the text `shift` bytes off the 16-byte grid; result() waits and reads back."""

    def __init__(self, tok, stream, wset, text, offs, flags=0, shift=0, want_totals=True, want_hits=True, n_bytes=None):
        import torch
        dev = torch.device("cuda", 0)
        text, offs = np.frombuffer(bytes(text), dtype=np.uint8), np.asarray(offs, dtype=np.int64)
        self.n_docs, self.n_entries, self.stream = len(offs) - 1, wset.n_entries, stream
        with torch.cuda.stream(stream):
            self.raw = torch.from_numpy(np.concatenate([np.full(16 + shift, 0x74, np.uint8), text, np.full(16, 0x65, np.uint8)])).to(dev)
            self.offs = torch.from_numpy(offs).to(dev)
            self.stats = torch.full((self.n_docs * 4 + SLACK,), FILL, dtype=torch.int64, device=dev)
            self.totals = torch.full((4 + SLACK,), FILL, dtype=torch.int64, device=dev)
            self.hits = torch.full((self.n_entries + SLACK,), FILL, dtype=torch.int64, device=dev)
        tok.word_matches_device(wset, self.raw.data_ptr() + 16 + shift, len(text) if n_bytes is None else n_bytes, self.offs.data_ptr(), self.n_docs,
                                flags, self.stats.data_ptr(), self.totals.data_ptr() if want_totals else 0,
                                self.hits.data_ptr() if want_hits else 0, stream.cuda_stream)

    def result(self):
        """-> ((stats, totals, entry_hits), the slack behind every output is untouched, the whole buffers)"""
        self.stream.synchronize()
        stats, totals, hits = (x.cpu().numpy() for x in (self.stats, self.totals, self.hits))
        n, e = self.n_docs, self.n_entries
        slack = bool((stats[4 * n:] == FILL).all() and (totals[4:] == FILL).all() and (hits[e:] == FILL).all())
        return (stats[:4 * n].reshape(n, 4), totals[:4], hits[:e]), slack, (stats, totals, hits)


# every case, off the 16-byte grid by 0, 1 and 15 bytes, resident and in global memory (the set above the LDS budget: there only)
@pytest.mark.parametrize("name, shift, no_lds", [(n, s, g) for n in CASES for s in (0, 1, 15) for g in (0, 1) if g or n != BIG])
def test_seam_cases(tok, side, case, name, shift, no_lds):
    from tokendagger_amd import capi
    wset, want = case(name)
    assert wset.info["resident"] == (name != BIG) and wset.info["max_len"] == max(map(len, CASES[name][2]))
    got, slack, _ = Call(tok, side, wset, *CASES[name][:2], flags=capi.TD_WL_NO_LDS if no_lds else 0, shift=shift).result()
    assert tok.device_status_pos(side.cuda_stream) == (capi.TD_OK, 0)
    wt.same(got, want, (name, shift, no_lds))
    assert slack


def test_without_totals_and_entry_hits(tok, side, case):
    name = "dense"
    wset, want = case(name)
    (stats, _, _), _, (_, totals, hits) = Call(tok, side, wset, *CASES[name][:2], want_totals=False, want_hits=False).result()
    assert stats.tolist() == want[0] and (totals == FILL).all() and (hits == FILL).all()


@pytest.mark.parametrize("offs, n_bytes, bad", [([0, 30, 20, 10, 40], 40, 1), ([1, 10, 40], 40, 0), ([0, 10, 50], 40, 1), ([0, -1, 40], 40, 0)])
def test_bad_offsets_write_nothing(tok, side, case, offs, n_bytes, bad):
    from tokendagger_amd import capi
    call = Call(tok, side, case("dense")[0], b"the " * 16, offs, n_bytes=n_bytes)
    assert tok.device_status_pos(side.cuda_stream) == (capi.TD_E_INVALID, bad)
    assert all((x == FILL).all() for x in call.result()[2])


def test_the_host_buffer_call_and_the_tokenizer(tok, case):
    import tokendagger as tiktoken
    name = "first hit with hits in two tiles"
    text, offs, entries, groups, flags = CASES[name]
    wset, want = case(name)
    wt.same(tok.word_matches(wset, text, offs), want, "td_word_matches")
    pat, mr, special = H.llama4()
    tk = tiktoken.Encoding(name="llama4", pat_str=pat, mergeable_ranks=mr, special_tokens=special)
    ws = tk.word_set(["The", "be", b"to", "of", "AND", "that", "have", "with", "the"], groups="each")  # (upper case folded, the repeat dropped)
    assert ws.dropped == [8] and ws.n_entries == 8
    wm = tk.word_matches(text, np.asarray(offs, dtype=np.int64), ws)
    wt.same((wm.stats, wm.totals, wm.entry_hits), want, "Tokenizer.word_matches")
    assert wm.distinct_groups.tolist() == [0, 2] and np.array_equal(wm.first_hit, wm.stats[:, 2]) and wm.hits.sum() == wm.totals[0]


def test_random_words(tok, side):
    rnd = random.Random(3)
    vocab = [bytes(rnd.choice(b"abcdefgh") for _ in range(rnd.randrange(1, 7))) for _ in range(50)]
    entries = sorted(set(rnd.sample(vocab, 20) + [b"a b", b"b. c"]))
    docs = []
    for _ in range(40):
        docs.append(b"".join(rnd.choice(vocab) + rnd.choice([b" ", b" ", b". ", b"\n", b"", b"\xc3\xa9 "]) for _ in range(rnd.randrange(0, 900))))
    text, offs = b"".join(docs), np.cumsum([0] + [len(d) for d in docs]).tolist()
    assert len(text) > 60000
    groups = [i % 64 for i in range(len(entries))]
    with tok.word_set(entries, groups) as wset:
        got, slack, _ = Call(tok, side, wset, text, offs, shift=5).result()
    wt.same(got, wt.matches(text, offs, entries, groups), "random words")
    assert slack
