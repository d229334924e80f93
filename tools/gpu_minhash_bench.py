"""Cost of the MinHash signatures: 1 GiB of English encoded once with td_encode_device and kept resident, then
td_minhash_device on those ids (k = 5, num_perm = 128, seed = 1) in two shapes:
  english_docs   the documents as they were encoded (about 127 ids each)
  short_docs     the same ids cut into documents of 8 to 40 ids (seeded): many documents a tile, a short run per document
each without band keys and with 32 bands of 4 rows, beside the dense device-to-device copy of the ids in the same process.  The cases
alternate `repeats` times; each time a case's figure is the median over `steps` windows after `warmup` calls, a window being as many
back-to-back calls between two HIP events as fill about `window_ms`, divided by their number; the report gives the median of those and
their smallest and largest, and hash evaluations per second = shingles hashed * num_perm / the median.  Before anything is timed both
shapes are held against td_minhash_host on the corpus' first 200 000 ids.

usage: gpu_minhash_bench.py [--size-mb 1024] [--num-perm 128] [--k 5] [--steps 10] [--warmup 3] [--repeats 3] [--window-ms 20] [--json OUT] [--only CASE]
Kernel times and counters: run this tool under rocprofv3 (--kernel-trace --stats, or --pmc ... alone), in a run of its own.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from tokendagger_amd import capi, vocab_io  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mb", type=int, default=1024)
    ap.add_argument("--num-perm", type=int, default=128)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--json", default="")
    ap.add_argument("--only", default="", help="time only the cases whose name contains this (a profiler run on one case)")
    args = ap.parse_args()
    _, pat, ranks, special = vocab_io.load_tdv(vocab_io.default_vocab_path())
    tok = capi.HipTokenizer(pat, ranks, special, device=0)
    n = args.size_mb << 20
    x, offs = bench.build_corpus("english", n, 1000)
    nd = len(offs) - 1
    side = torch.cuda.Stream()  # (td_minhash_device does not take the null stream)
    s = side.cuda_stream
    with torch.cuda.stream(side):
        dt = torch.from_numpy(x).cuda()
        do = torch.from_numpy(offs).cuda()
        cap = n // 3
        dk = torch.empty(cap, dtype=torch.int32, device="cuda")
        dto = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
        tok.encode_device(dt.data_ptr(), n, do.data_ptr(), nd, dk.data_ptr(), cap, dto.data_ptr(), s)
        tok.device_status(s)
        del dt
        h_toff = dto.cpu().numpy()
        ntok = int(h_toff[nd])
        real = dk[:ntok]
        # the same ids in documents of 8 to 40 ids
        rng = np.random.default_rng(11)
        lens = rng.integers(8, 41, size=ntok // 8 + 1)
        cuts = np.concatenate([[0], np.cumsum(lens)])
        cuts = cuts[:int(np.searchsorted(cuts, ntok, side="left")) + 1].astype(np.int64)
        cuts[-1] = ntok
        shapes = {"english_docs": (dto, nd, h_toff), "short_docs": (torch.from_numpy(cuts).cuda(), len(cuts) - 1, cuts)}
        max_docs = max(v[1] for v in shapes.values())
        sig = torch.empty(max_docs * args.num_perm, dtype=torch.int32, device="cuda")
        keys = torch.empty(max_docs * 32, dtype=torch.int64, device="cuda")
        counts = torch.zeros(4, dtype=torch.int64, device="cuda")
        out = torch.empty(ntok, dtype=torch.int32, device="cuda")
    plain = capi.minhash_spec(args.k, args.num_perm, 1)
    banded = capi.minhash_spec(args.k, args.num_perm, 1, 32, min(4, args.num_perm // 32)) if args.num_perm >= 32 else None

    def call(shape, spec):
        d_off, docs, _ = shapes[shape]
        return lambda: tok.minhash_device(real.data_ptr(), ntok, d_off.data_ptr(), docs, spec, sig.data_ptr(),
                                          keys.data_ptr() if spec.bands else 0, counts.data_ptr(), s)

    # sanity, before anything is timed: both shapes against the host statement on the first 200 000 ids
    head = real[:200000].cpu().numpy()
    shingles = {}
    for name, (d_off, docs, h_off) in shapes.items():
        kd = int(np.searchsorted(h_off, 200000, side="right")) - 1
        want = capi.minhash_host(head[:int(h_off[kd])], h_off[:kd + 1], banded or plain)
        call(name, banded or plain)()
        tok.device_status(s)
        side.synchronize()
        assert np.array_equal(sig[:kd * args.num_perm].cpu().numpy().view(np.uint32).reshape(kd, -1), want[0]), name
        if banded:
            assert np.array_equal(keys[:kd * 32].cpu().numpy().view(np.uint64).reshape(kd, 32), want[1]), name
        shingles[name] = counts.cpu().tolist()

    cases = {"dense_copy": lambda: out.copy_(real)}
    for name in shapes:
        cases[name] = call(name, plain)
        if banded:
            cases[name + "_bands_32x4"] = call(name, banded)
    if args.only:
        cases = {k: v for k, v in cases.items() if args.only in k}
    inner = {}

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
        side.synchronize()
        return e0.elapsed_time(e1) / calls

    def timed(k, fn):
        with torch.cuda.stream(side):
            for _ in range(args.warmup):
                fn()
        side.synchronize()
        tok.device_status(s)
        if k not in inner:
            inner[k] = int(min(max(round(args.window_ms / max(window(fn, 1), 1e-3)), 1), 256))
        ts = [window(fn, inner[k]) for _ in range(args.steps)]
        tok.device_status(s)
        return float(np.median(ts))

    medians = {k: [] for k in cases}
    for _ in range(args.repeats):
        for k, fn in cases.items():
            medians[k].append(timed(k, fn))
    res = {"corpus": "english", "size_mb": args.size_mb, "ids": ntok, "k": args.k, "num_perm": args.num_perm, "steps": args.steps,
           "repeats": args.repeats, "window_ms": args.window_ms,
           "shapes": {name: {"docs": v[1], "counts": shingles[name]} for name, v in shapes.items()}, "cases": []}
    for k, ms in medians.items():
        med = float(np.median(ms))
        row = {"case": k, "calls_per_window": inner[k], "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
               "medians_ms": [round(m, 4) for m in ms], "ids_per_us": round(ntok / med / 1e3, 2)}
        shape = k.replace("_bands_32x4", "")
        if shape in shingles:
            row["hash_evals_per_s"] = float(f"{shingles[shape][0] * args.num_perm / (med * 1e-3):.4g}")
        res["cases"].append(row)
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
