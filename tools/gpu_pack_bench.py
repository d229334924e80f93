"""Cost of best-fit-decreasing rows: 1 GiB of English encoded with td_encode_device, then td_pack_rows_device
on the device ids at S = 8192 and 2048 with BOS + EOS; medians over `steps` calls after `warmup`.

Per S it reports
  call_ms     host wall time of td_pack_rows_device with the stream idle before it: the items kernel, the scan, the sort and the
              run-length encode, the one read-back, the host plan, the plan's upload and the output launches (it returns then)
  total_ms    the same call until the output kernels are done (torch.cuda.synchronize)
  plan_ms     the host planner alone on the same offsets (td_pack_plan: items, sort and placement all on the host)
  concat_ms   td_make_rows_device CONCAT at the same S, ids + cu_seqlens (HIP events), for comparison
  rows / fill of BFD against CONCAT (ceil(T / S) rows, documents cut) and PAD (one row per document)
With --stats DB (the rocpd database of a `rocprofv3 --kernel-trace` run of this same tool) it prints the kernel phases instead:
items, sort (rocPRIM scan, radix sort and run-length encode), segments, slots, median microseconds per call for each S.

usage: gpu_pack_bench.py [--size-mb 1024] [--steps 10] [--warmup 2] [--json OUT] [--stats DB]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from tokendagger_amd import capi, vocab_io  # noqa: E402

BOS, EOS = 200000, 200001
SEQ_LENS = (8192, 2048)


def _phase(name):
    if "td_pack_items" in name:
        return "items"
    if "rocprim" in name:
        return "sort"
    if "td_pack_segments" in name:
        return "segments"
    if "td_pack_slots" in name:
        return "slots"
    return None


def kernel_phases(path, per_s):
    """A rocprofv3 --kernel-trace database (rocpd SQLite) of a run of this tool -> per S, the median microseconds of each phase
    over the pack calls.  A call is the kernels from one td_pack_items dispatch to the next; the calls come in SEQ_LENS order,
    per_s of them for each S."""
    import sqlite3
    rows = sqlite3.connect(path).execute("select name, start, duration from kernels order by start").fetchall()
    calls = []
    for name, _, dur in rows:
        ph = _phase(name)
        if ph == "items":
            calls.append({"items": 0.0, "sort": 0.0, "segments": 0.0, "slots": 0.0})
        if ph and calls:
            calls[-1][ph] += dur / 1e3
    out = {}
    for i, S in enumerate(SEQ_LENS):
        mine = calls[i * per_s:(i + 1) * per_s]
        out[str(S)] = {k: round(float(np.median([c[k] for c in mine])), 1) for k in ("items", "sort", "segments", "slots")} if mine else {}
    return out, len(calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mb", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default="")
    ap.add_argument("--stats", default="", help="rocpd database of a rocprofv3 --kernel-trace run of this tool (summarised, no device)")
    args = ap.parse_args()
    if args.stats:  # (summary of a profiled run of this tool with the same --steps / --warmup; no device needed)
        ph, calls = kernel_phases(args.stats, args.warmup + args.steps)
        line = json.dumps({"kernel_trace": os.path.basename(args.stats), "pack_calls": calls, "us_median_per_call": ph})
        print(line, flush=True)
        if args.json:
            with open(args.json, "a") as f:
                f.write(line + "\n")
        return
    _, pat, ranks, special = vocab_io.load_tdv(vocab_io.default_vocab_path())
    tok = capi.HipTokenizer(pat, ranks, special, device=0)
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
    toffs = dto.cpu().numpy()
    ntok = int(toffs[-1])
    res = {"corpus": "english", "size_mb": args.size_mb, "docs": nd, "ids": ntok, "steps": args.steps, "cases": []}
    for S in SEQ_LENS:
        sp = capi.pack_spec(S, BOS, EOS, 0)
        t0 = time.perf_counter()
        counts = capi.pack_plan(toffs, sp)
        plan_ms = 1e3 * (time.perf_counter() - t0)
        rows = int(counts[0])
        out = torch.empty(rows * S, dtype=torch.int32, device="cuda")
        cu = torch.empty(nd + 2 * rows + 1, dtype=torch.int32, device="cuda")
        call, total = [], []
        for i in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c = tok.pack_rows_device(dk.data_ptr(), cap, dto.data_ptr(), nd, sp, out.data_ptr(), rows, 0, cu.data_ptr(), 0, 0, s)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i >= args.warmup:
                call.append(1e3 * (t1 - t0))
                total.append(1e3 * (t2 - t0))
        assert np.array_equal(c, counts), (c, counts)
        del out, cu
        # CONCAT at the same S (ids + cu_seqlens), HIP events
        csp = capi.rows_spec(S, capi.TD_ROWS_CONCAT, BOS, EOS, 0)
        crows = capi.rows_capacity_of(csp, ntok, nd)
        out = torch.empty(crows * S, dtype=torch.int32, device="cuda")
        aux = torch.empty(nd + crows + 1, dtype=torch.int32, device="cuda")
        dc = torch.zeros(4, dtype=torch.int64, device="cuda")
        ts = []
        for i in range(args.warmup + args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tok.make_rows_device(dk.data_ptr(), cap, dto.data_ptr(), nd, csp, out.data_ptr(), crows, 0, aux.data_ptr(), dc.data_ptr(), s)
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append(e0.elapsed_time(e1))
        tok.device_status(s)
        del out, aux
        T = ntok + 2 * nd
        L = np.diff(toffs)
        pad_real = int(np.minimum(L + 2, S).sum())
        res["cases"].append({
            "seq_len": S, "bfd": {"rows": rows, "real_slots": int(counts[1]), "segments": int(counts[2]), "documents_cut": int(counts[3]),
                                  "fill": round(int(counts[1]) / (rows * S), 6)},
            "concat": {"rows": crows, "fill": round(T / (crows * S), 6), "documents_cut_at_row_starts": "yes"},
            "pad": {"rows": nd, "fill": round(pad_real / (nd * S), 6), "documents_truncated": int((L + 2 > S).sum())},
            "call_ms_median": round(float(np.median(call)), 3), "total_ms_median": round(float(np.median(total)), 3),
            "call_ms_min": round(float(np.min(call)), 3), "total_ms_min": round(float(np.min(total)), 3),
            "plan_host_only_ms": round(plan_ms, 1), "concat_cu_ms_median": round(float(np.median(ts)), 3)})
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
