"""Cost of the token counts: 1 GiB of English encoded once with td_encode_device and kept resident, then
td_token_counts_device on (a) the real ids, (b) uniform random values over [0, n_bins), (c) one value everywhere, and (a) again
with eight document groups, beside three yardsticks in the same process: the dense device-to-device copy of the same bytes,
td_make_rows_device CONCAT ids-only at S = 8192 on the same ids, and torch.bincount(ids, minlength=n_bins) on the same device (the
off-the-shelf alternative).  The cases alternate `repeats` times; each time a case's figure is the median over `steps`
windows after `warmup` calls, a window being as many back-to-back calls between two HIP events as fill about `window_ms` (a call
of 0.3 ms alone between two events measures the events as much as the call), divided by their number; the report gives the
median of those and their smallest and largest.  Before anything is timed every counts case is compared with torch.bincount of
its stream, exactly.

usage: gpu_counts_bench.py [--size-mb 1024] [--steps 10] [--warmup 3] [--repeats 5] [--window-ms 20] [--json OUT]
Kernel times: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/gpu_counts_bench.py`, in a run of its own.
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

BOS, EOS = 200000, 200001
N_GROUPS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mb", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    _, pat, ranks, special = vocab_io.load_tdv(vocab_io.default_vocab_path())
    tok = capi.HipTokenizer(pat, ranks, special, device=0)
    n_bins = max(max(ranks.values()), max(special.values()) if special else 0) + 1
    n = args.size_mb << 20
    x, offs = bench.build_corpus("english", n, 1000)
    nd = len(offs) - 1
    dt = torch.from_numpy(x).cuda()
    do = torch.from_numpy(offs).cuda()
    cap = n // 3
    dk = torch.empty(cap, dtype=torch.int32, device="cuda")
    dto = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    tok.encode_device(dt.data_ptr(), n, do.data_ptr(), nd, dk.data_ptr(), cap, dto.data_ptr(), s)
    tok.device_status(s)
    del dt
    ntok = int(dto[nd].item())
    real = dk[:ntok]
    uniform = torch.randint(0, n_bins, (ntok,), dtype=torch.int32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    equal = torch.full((ntok,), 1234, dtype=torch.int32, device="cuda")
    d_grp = (torch.arange(nd, device="cuda", dtype=torch.int32) % N_GROUPS).contiguous()

    inner = {}  # calls per timed window, fixed per case at its first visit

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    def timed(k, fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        tok.device_status(s)
        if k not in inner:  # a call of 0.3 ms alone between two events measures the events as much as the call: windows of about args.window_ms
            inner[k] = int(min(max(round(args.window_ms / max(window(fn, 1), 1e-3)), 1), 256))
        ts = [window(fn, inner[k]) for _ in range(args.steps)]
        tok.device_status(s)
        return float(np.median(ts))

    out = torch.empty(ntok, dtype=torch.int32, device="cuda")
    counts = torch.zeros(N_GROUPS * n_bins, dtype=torch.int64, device="cuda")
    info = torch.zeros(4, dtype=torch.int64, device="cuda")
    sp_rows = capi.rows_spec(8192, capi.TD_ROWS_CONCAT, BOS, EOS, 0)
    rows = capi.rows_capacity_of(sp_rows, ntok, nd)
    r_out = torch.empty(rows * 8192, dtype=torch.int32, device="cuda")
    r_counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    one, eight = capi.counts_spec(n_bins), capi.counts_spec(n_bins, N_GROUPS)

    def count(ids, spec=one, grouped=False):
        return lambda: tok.token_counts_device(ids.data_ptr(), ntok, dto.data_ptr() if grouped else 0, nd if grouped else 0,
                                               d_grp.data_ptr() if grouped else 0, spec, counts.data_ptr(), info.data_ptr(), s)

    # sanity, before anything is timed: every stream's counts against torch.bincount, exactly
    for name, ids in (("real", real), ("uniform", uniform), ("equal", equal)):
        count(ids)()
        tok.device_status(s)
        assert torch.equal(counts[:n_bins], torch.bincount(ids, minlength=n_bins)), name
        assert info.tolist() == [ntok, 0, 0, 0], (name, info.tolist())
    count(real, eight, True)()
    tok.device_status(s)
    assert torch.equal(counts.view(N_GROUPS, n_bins).sum(0), torch.bincount(real, minlength=n_bins)) and info.tolist() == [ntok, 0, 0, 0]
    lens = (dto[1:] - dto[:-1])
    per_group = torch.zeros(N_GROUPS, dtype=torch.int64, device="cuda").index_add_(0, d_grp.long(), lens)
    assert torch.equal(counts.view(N_GROUPS, n_bins).sum(1), per_group)

    cases = {
        "rows_concat_8192_ids_only": lambda: tok.make_rows_device(dk.data_ptr(), cap, dto.data_ptr(), nd, sp_rows, r_out.data_ptr(), rows, 0, 0,
                                                                  r_counts.data_ptr(), s),
        "dense_copy": lambda: out.copy_(real),
        "torch_bincount_real": lambda: torch.bincount(real, minlength=n_bins),
        "torch_bincount_uniform": lambda: torch.bincount(uniform, minlength=n_bins),
        "torch_bincount_equal": lambda: torch.bincount(equal, minlength=n_bins),
        "counts_real": count(real),
        "counts_uniform": count(uniform),
        "counts_equal": count(equal),
        "counts_real_8_groups": count(real, eight, True),
    }
    medians = {k: [] for k in cases}
    for _ in range(args.repeats):
        for k, fn in cases.items():
            medians[k].append(timed(k, fn))
    res = {"corpus": "english", "size_mb": args.size_mb, "docs": nd, "ids": ntok, "n_bins": n_bins, "steps": args.steps, "repeats": args.repeats,
           "window_ms": args.window_ms, "cases": []}
    for k, ms in medians.items():
        med = float(np.median(ms))
        res["cases"].append({"case": k, "calls_per_window": inner[k], "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                             "medians_ms": [round(m, 4) for m in ms], "ms_per_gib_of_ids": round(med * (1 << 30) / (4 * ntok), 4)})
    by = {r["case"]: r for r in res["cases"]}
    # The issue's marks, against torch.bincount of the REAL ids: (a) no slower than it, the worst of (a) - (c) within its run-to-run
    # spread.  Beside them, every stream against torch.bincount of the SAME stream, with that reference's own spread.
    y = by["torch_bincount_real"]
    spread = y["max_ms"] - y["min_ms"]
    worst = max(by[k]["median_ms"] for k in ("counts_real", "counts_uniform", "counts_equal"))
    same = {}
    for name in ("real", "uniform", "equal"):
        c, b = by["counts_" + name], by["torch_bincount_" + name]
        same[name] = {"counts_ms": c["median_ms"], "bincount_ms": b["median_ms"], "bincount_spread_ms": round(b["max_ms"] - b["min_ms"], 4),
                      "ratio": round(c["median_ms"] / b["median_ms"], 4),
                      "within_spread": bool(c["median_ms"] <= b["median_ms"] + (b["max_ms"] - b["min_ms"]))}
    res["mark"] = {"comparator": "torch.bincount of the real ids", "bincount_real_ms": y["median_ms"], "bincount_spread_ms": round(spread, 4),
                   "counts_real_ms": by["counts_real"]["median_ms"], "worst_of_abc_ms": worst,
                   "real_no_slower_than_bincount": bool(by["counts_real"]["median_ms"] <= y["median_ms"]),
                   "worst_within_spread_of_bincount": bool(worst <= y["median_ms"] + spread),
                   "ratio_real_to_bincount": round(by["counts_real"]["median_ms"] / y["median_ms"], 4),
                   "ratio_worst_to_bincount": round(worst / y["median_ms"], 4),
                   "against_bincount_of_the_same_stream": same}
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
