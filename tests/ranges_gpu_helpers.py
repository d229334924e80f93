"""What tests/test_gpu_ranges.py and tests/test_gpu_ranges_limits.py share: the vocabulary and handle fixtures, the comparison of
every output of td_range_labels with a truth of tests/ranges_truth.py, the generators of ranges, and the device form's call.
Token lengths come from the vocabulary on the host (offsets_truth.id_lengths), never from the device."""
import numpy as np
import pytest

import helpers as H
import offsets_truth as OT
import ranges_truth as rt

TILE = 4096   # td::RNG_TILE
WIN = 512     # td::RNG_WIN


@pytest.fixture(scope="module")
def vocab():
    pat, mr, special = H.llama4()
    lengths = OT.id_lengths(OT.id_bytes(mr, special))
    pool = []
    for k in range(1, 13):
        pool += np.flatnonzero(lengths == k)[:3].tolist()
    pool += np.argsort(-lengths)[:3].tolist()
    return pat, mr, special, lengths, np.asarray(pool, dtype=np.int32)


@pytest.fixture(scope="module")
def tok(vocab):
    from tokendagger_amd import capi
    return capi.HipTokenizer(vocab[0], vocab[1], vocab[2], device=0)


def _spec(rule="overlap", ignore=-100):
    from tokendagger_amd import capi
    return capi.range_spec(rule, ignore)


def _same(got, want, what=""):
    for k, (p, q) in enumerate(zip(got, want)):
        assert p.dtype == q.dtype and p.shape == q.shape and np.array_equal(p, q), (what, k)


def _check(tok, lengths, ids, offs, ro, rg, rules=rt.RULES, combos=((True, True),), ignore=-100, starts=None, truth=rt.ranges_numpy):
    out = {}
    for rule in rules:
        t = truth(ids, offs, ro, rg, lengths, rule, ignore, starts)
        for mask, toff in combos:
            g = tok.range_labels(ids, offs, (ro, rg), _spec(rule, ignore), mask=mask, trained_offsets=toff, starts=starts)
            assert np.array_equal(g[3], t[3]), (rule, g[3], t[3])
            assert g[0].dtype == np.int32 and np.array_equal(g[0], t[0]), rule
            assert (g[1] is None) == (not mask) and (g[2] is None) == (not toff)
            if mask:
                assert g[1].dtype == np.uint8 and np.array_equal(g[1], t[1]), rule
            if toff:
                assert g[2].dtype == np.int64 and np.array_equal(g[2], t[2]), rule
        out[rule] = t
    return out


def _doc_sizes(lengths, ids, offs):
    cs = np.concatenate([[0], np.cumsum(lengths[ids])])
    return cs[offs[1:]] - cs[offs[:-1]]


def _bulk_ranges(rng, sizes, max_k, min_k=0):
    """Per document min_k to max_k sorted disjoint ranges inside its bytes (some empty, some touching, some up to its end)."""
    ro, out = [0], []
    for size in sizes.tolist():
        k = int(rng.integers(min_k, max_k + 1))
        cuts = np.sort(rng.integers(0, size + 1, 2 * k)).reshape(-1, 2)
        if k and rng.random() < 0.3:
            cuts[-1, 1] = size
        out.append(cuts)
        ro.append(ro[-1] + k)
    return np.asarray(ro, dtype=np.int64), np.concatenate(out).astype(np.int64) if out else np.zeros((0, 2), np.int64)


def _every_other_byte(n_ranges):
    return np.stack([2 * np.arange(n_ranges), 2 * np.arange(n_ranges) + 1], axis=1).astype(np.int64)


def _device_alloc(n, n_docs, dev, fill=77):
    import torch
    return (torch.full((max(n, 1),), fill, dtype=torch.int32, device=dev), torch.full((max(n, 1),), fill, dtype=torch.uint8, device=dev),
            torch.full((n_docs + 1,), fill, dtype=torch.int64, device=dev), torch.full((4,), fill, dtype=torch.int64, device=dev))


def _device_call(tok, ids, n_tokens, offs, ro, rg, spec, starts=None, fill=77):
    """The device form on torch's current stream -> (the four outputs as numpy, (code, err_pos))."""
    import torch
    dev = torch.device("cuda", 0)
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(dev)
    d_offs, d_ro = torch.from_numpy(np.asarray(offs, dtype=np.int64)).to(dev), torch.from_numpy(np.asarray(ro, dtype=np.int64)).to(dev)
    d_rg = torch.from_numpy(np.ascontiguousarray(rg, dtype=np.int64).reshape(-1, 2)).to(dev)
    d_st = torch.from_numpy(np.asarray(starts, dtype=np.int64)).to(dev) if starts is not None else None
    outs = _device_alloc(len(ids), len(offs) - 1, dev, fill)
    stream = torch.cuda.current_stream(dev).cuda_stream
    tok.range_labels_device(d_ids.data_ptr(), n_tokens, d_offs.data_ptr(), len(offs) - 1, d_ro.data_ptr(), d_rg.data_ptr() if len(rg) else 0,
                            len(rg), spec, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
                            d_st.data_ptr() if d_st is not None else 0, stream)
    status = tok.device_status_pos(stream)
    return [o.cpu().numpy() for o in outs], status
