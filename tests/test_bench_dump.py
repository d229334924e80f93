"""bench.py --dump-outputs: the arrays it writes are the timed path's outputs (whole, or a fixed seeded sample of them with the
positions beside it), in float32 / float64, within 64 MiB, and the same from run to run.  CPU tensors stand in for the device buffers."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import bench


def _buffers(n_tok: int, n_docs: int):
    rng = np.random.default_rng(5)
    d_tok = torch.from_numpy(rng.integers(0, 200_000, size=n_tok + 64, dtype=np.int32))
    d_toff = torch.from_numpy(np.concatenate([np.sort(rng.integers(0, n_tok, size=n_docs)), [n_tok, n_docs]]).astype(np.int64))
    return d_tok, d_toff


def test_small_outputs_are_written_whole(tmp_path):
    d_tok, d_toff = _buffers(1000, 40)
    info = bench.dump_outputs(str(tmp_path), d_tok, d_toff, 1000, 40, 1, 0, None)
    assert sorted(info["files"]) == ["token_ids.npy", "token_offsets.npy"]
    ids, offs = np.load(tmp_path / "token_ids.npy"), np.load(tmp_path / "token_offsets.npy")
    assert ids.dtype == np.float32 and offs.dtype == np.float64
    assert np.array_equal(ids, d_tok[:1000].numpy().astype(np.float32))
    assert np.array_equal(offs, d_toff[:41].numpy().astype(np.float64))


def test_large_outputs_are_a_seeded_sample_within_budget(tmp_path):
    n_tok, n_docs = 3 << 20, (1 << 21) + 7
    d_tok, d_toff = _buffers(n_tok, n_docs)
    info = bench.dump_outputs(str(tmp_path / "a"), d_tok, d_toff, n_tok, n_docs, 1, 0, None)
    bench.dump_outputs(str(tmp_path / "b"), d_tok, d_toff, n_tok, n_docs, 1, 0, None)
    assert info["bytes"] <= 64 << 20
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 64 << 20
    for name, src, n in (("token_ids", d_tok, n_tok), ("token_offsets", d_toff, n_docs + 1)):
        vals, idx = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "a" / f"{name}_index.npy")
        assert len(vals) == len(idx) == bench.DUMP_MAX_ELEMENTS
        assert np.all(np.diff(idx) > 0) and idx[-1] < n
        assert np.array_equal(vals, src.numpy()[idx.astype(np.int64)].astype(vals.dtype))
        assert np.array_equal(vals, np.load(tmp_path / "b" / f"{name}.npy"))
        assert np.array_equal(idx, np.load(tmp_path / "b" / f"{name}_index.npy"))


def test_steps_must_be_positive():
    assert bench.parse_args(["--steps", "3"]).steps == 3
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
