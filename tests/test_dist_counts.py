"""dist.sum_counts on CPU: gloo processes each count their shard of one corpus of ids (the contract's host statement,
td_token_counts_host) and the all-reduced sum is the histogram of the whole corpus, as a numpy array and as a tensor."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
N_BINS, N_GROUPS, N_DOCS = 500, 3, 400


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _corpus():
    rng = np.random.default_rng(0)  # the same corpus on every rank
    lens = rng.integers(0, 200, size=N_DOCS)
    offs = np.zeros(N_DOCS + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    ids = rng.integers(-2, N_BINS + 2, size=int(offs[-1])).astype(np.int32)
    groups = rng.integers(0, N_GROUPS, size=N_DOCS).astype(np.int32)
    return ids, offs, groups


def _worker(rank, world, port, q):
    sys.path.insert(0, str(ROOT))
    import torch
    import torch.distributed as dist
    from tokendagger_amd import capi
    from tokendagger_amd import dist as tdist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ids, offs, groups = _corpus()
    d0, d1 = tdist.shard_documents(offs, world, rank)
    # tok_offsets[0] > 0: a rank counts its documents' ids where they lie
    mine, info = capi.token_counts_host(ids, offs[d0:d1 + 1], groups[d0:d1], capi.counts_spec(N_BINS, N_GROUPS))
    total = tdist.sum_counts(mine)
    assert total is not mine and total.shape == mine.shape and total.dtype == np.int64
    t = torch.from_numpy(mine.copy())
    same = tdist.sum_counts(t)
    assert same is t and np.array_equal(t.numpy(), total)
    q.put((rank, total, int(info[0])))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sum_counts_gloo(world):
    import torch.multiprocessing as mp
    sys.path.insert(0, str(ROOT))
    from tokendagger_amd import capi
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in range(world)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ids, offs, groups = _corpus()
    want, info = capi.token_counts_host(ids, offs, groups, capi.counts_spec(N_BINS, N_GROUPS))
    assert sum(r[2] for r in res) == int(info[0]) == int(want.sum())
    for r in res:
        assert np.array_equal(r[1], want)


def test_sum_counts_rejects_other_types():
    from tokendagger_amd import dist as tdist
    with pytest.raises(TypeError):
        tdist.sum_counts(np.zeros(4, dtype=np.int32))
