"""Cost of the per-document text statistics, on resident text, in GB/s of input:
  english, mixed   --size-mb (1024) of bench.py's corpora each: td_text_stats_device with groups = LOCAL and LOCAL | RUNS, and in the same
                   process on the same buffer td_utf8_check_device (the project's read-speed yardstick) and td_encode_device (the step the
                   statistics stand beside).  Each case also as a multiple of the check and as a share of the encode.
Before anything is timed the device results are held against td_text_stats_host on the first MiB.  A case's figure is the median over
`steps` windows after `warmup` calls, a window being as many back-to-back calls between two HIP events as fill about `window_ms`.

usage: gpu_textstats_bench.py [--size-mb 1024] [--steps 7] [--warmup 2] [--window-ms 20] [--json OUT] [--only CASE]
       gpu_textstats_bench.py --merge OUT --kernel-stats CSV --json profiles/textstats_cost.json
Kernel times: run this tool under rocprofv3 --kernel-trace --stats in a run of its own (--only keeps it short), then hand its
kernel_stats.csv to --merge: the td_ts_* rows go into the result as "kernels".
"""
import argparse
import csv
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


def kernel_rows(path):
    """the td_ts_* rows of a rocprofv3 kernel_stats.csv -> [{kernel, calls, average_us, min_us, max_us}] (over every corpus of that run)"""
    out = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if "td_ts_" in name:
                out.append({"kernel": name.replace("td::(anonymous namespace)::", "").replace("void ", "").split("(")[0],
                            "calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 1),
                            "min_us": round(float(row["MinNs"]) / 1e3, 1), "max_us": round(float(row["MaxNs"]) / 1e3, 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mb", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--json", default="")
    ap.add_argument("--only", default="", help="time only the cases whose name contains this (a profiler run on one case)")
    ap.add_argument("--kernel-stats", default="", help="kernel_stats.csv of a separate rocprofv3 --kernel-trace --stats run of this tool")
    ap.add_argument("--merge", default="", help="no GPU: the last result line of this file with --kernel-stats added, written to --json")
    args = ap.parse_args()
    if args.merge:
        with open(args.merge) as f:
            res = json.loads(f.read().strip().splitlines()[-1])
        res["kernels"] = kernel_rows(args.kernel_stats)
        res["kernels_from"] = "a separate rocprofv3 --kernel-trace --stats run of this tool with --only 'text_stats local+runs' --steps 3 --warmup 1"
        with open(args.json, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        return
    _, pat, ranks, special = vocab_io.load_tdv(vocab_io.default_vocab_path())
    tok = capi.HipTokenizer(pat, ranks, special, device=0)
    side = torch.cuda.Stream()  # (the device forms do not take the null stream)
    s = side.cuda_stream
    res = {"steps": args.steps, "window_ms": args.window_ms, "corpora": {}, "cases": []}

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
        side.synchronize()
        return e0.elapsed_time(e1) / calls

    def timed(fn):
        with torch.cuda.stream(side):
            for _ in range(args.warmup):
                fn()
        side.synchronize()
        tok.device_status(s)
        inner = int(min(max(round(args.window_ms / max(window(fn, 1), 1e-3)), 1), 256))
        ts = [window(fn, inner) for _ in range(args.steps)]
        tok.device_status(s)
        return float(np.median(ts)), float(min(ts)), float(max(ts)), inner

    for name in ("english", "mixed"):
        x, offs = bench.build_corpus(name, args.size_mb << 20, 1000)
        n, nd = len(x), len(offs) - 1
        with torch.cuda.stream(side):
            dt, do = torch.from_numpy(x).cuda(), torch.from_numpy(offs).cuda()
            stats = torch.empty(max(nd, 1) * capi.TD_TS_COLS, dtype=torch.int64, device="cuda")
            totals = torch.empty(capi.TD_TS_COLS, dtype=torch.int64, device="cuda")
            flags = torch.empty(max(nd, 1), dtype=torch.uint8, device="cuda")
            first = torch.empty(max(nd, 1), dtype=torch.int64, device="cuda")
            counts = torch.zeros(8, dtype=torch.int64, device="cuda")
            ids = torch.empty(n, dtype=torch.int32, device="cuda")
            toff = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
        ts = lambda g: tok.text_stats_device(dt.data_ptr(), n, do.data_ptr(), nd, g, stats.data_ptr(), totals.data_ptr(), s)  # noqa: E731
        check = lambda: tok.utf8_check(dt.data_ptr(), n, do.data_ptr(), nd, flags.data_ptr(), first.data_ptr(), counts.data_ptr(), s)  # noqa: E731
        encode = lambda: tok.encode_device(dt.data_ptr(), n, do.data_ptr(), nd, ids.data_ptr(), n, toff.data_ptr(), stream=s)  # noqa: E731
        # sanity, before anything is timed: the first MiB's documents against the host statement
        kd = int(np.searchsorted(offs, 1 << 20, side="right")) - 1
        want = capi.text_stats_host(x[:int(offs[kd])], offs[:kd + 1])[0]
        ts(capi.TD_TS_ALL)
        tok.device_status(s)
        side.synchronize()
        got = stats.cpu().numpy().reshape(-1, capi.TD_TS_COLS)
        assert np.array_equal(got[:kd], want), (name, "the statistics differ from td_text_stats_host")
        res["corpora"][name] = {"bytes": n, "docs": nd, "totals": totals.cpu().tolist()}
        cases = {"utf8_check": check, "encode_device": encode, "text_stats local": lambda: ts(capi.TD_TS_LOCAL),
                 "text_stats local+runs": lambda: ts(capi.TD_TS_ALL)}
        med_of = {}
        for k, fn in cases.items():
            if args.only and args.only not in f"{name}/{k}":
                continue
            med, lo, hi, inner = timed(fn)
            med_of[k] = med
            res["cases"].append({"corpus": name, "case": k, "calls_per_window": inner, "median_ms": round(med, 4), "min_ms": round(lo, 4),
                                 "max_ms": round(hi, 4), "input_gb_per_s": round(n / med / 1e6, 1)})
        for c in res["cases"]:
            if c["corpus"] == name and c["case"].startswith("text_stats") and "utf8_check" in med_of and "encode_device" in med_of:
                c["times_utf8_check"] = round(c["median_ms"] / med_of["utf8_check"], 2)
                c["share_of_encode"] = round(c["median_ms"] / med_of["encode_device"], 3)
        del dt, do, stats, totals, flags, first, ids, toff
    if args.kernel_stats:
        res["kernels"] = kernel_rows(args.kernel_stats)
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
