"""Cost of the document selection: 1 GiB of English encoded with td_encode_device, then td_select_docs_device on
the device ids for the identity, a random permutation and the permutation with min_len at the median length, beside two
yardsticks in the same process: the dense device-to-device copy of the identity's output bytes, and td_make_rows_device CONCAT
ids-only (no positions, no cu_seqlens) at S = 8192 on the same ids.  The five cases alternate `repeats` times; each time a
case's figure is the HIP-event median over `steps` single calls after `warmup`, and the report gives the median of those and
their smallest and largest.  The bytes a case must move are counted from the shapes (ids read and written, the scan's offsets,
out_offsets / out_docs / src_base written and read).

usage: gpu_select_bench.py [--size-mb 1024] [--steps 10] [--warmup 3] [--repeats 5] [--json OUT]
Kernel times: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/gpu_select_bench.py`, in a run of its own.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mb", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
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
    ntok = int(toffs[nd])
    median_len = int(np.median(np.diff(toffs)))
    perm = np.random.default_rng(1).permutation(nd).astype(np.int64)
    d_perm = torch.from_numpy(perm).cuda()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        tok.device_status(s)
        ts = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        tok.device_status(s)
        return float(np.median(ts))

    out = torch.empty(ntok, dtype=torch.int32, device="cuda")
    o_off = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
    o_docs = torch.empty(nd, dtype=torch.int64, device="cuda")
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    sp_rows = capi.rows_spec(8192, capi.TD_ROWS_CONCAT, BOS, EOS, 0)
    rows = capi.rows_capacity_of(sp_rows, ntok, nd)
    r_out = torch.empty(rows * 8192, dtype=torch.int32, device="cuda")
    r_counts = torch.zeros(4, dtype=torch.int64, device="cuda")

    def select(d_sel, spec):
        return lambda: tok.select_docs_device(dk.data_ptr(), cap, dto.data_ptr(), nd, d_sel, nd, spec, out.data_ptr(), ntok, o_off.data_ptr(),
                                              o_docs.data_ptr(), counts.data_ptr(), stream=s)

    cases = {
        "rows_concat_8192_ids_only": lambda: tok.make_rows_device(dk.data_ptr(), cap, dto.data_ptr(), nd, sp_rows, r_out.data_ptr(), rows, 0, 0,
                                                                  r_counts.data_ptr(), s),
        "dense_copy": lambda: out.copy_(dk[:ntok]),
        "select_identity": select(0, capi.select_spec()),
        "select_permutation": select(d_perm.data_ptr(), capi.select_spec()),
        "select_permutation_min_len_median": select(d_perm.data_ptr(), capi.select_spec(median_len)),
    }
    medians = {k: [] for k in cases}
    got = {}
    for _ in range(args.repeats):
        for k, fn in cases.items():
            medians[k].append(timed(fn))
            got[k] = (r_counts if k.startswith("rows") else counts).cpu().tolist()
    res = {"corpus": "english", "size_mb": args.size_mb, "docs": nd, "ids": ntok, "median_len": median_len, "steps": args.steps,
           "repeats": args.repeats, "cases": []}
    for k, ms in medians.items():
        c = got[k]
        if k == "dense_copy":
            moved, c = 8 * ntok, None
        elif k.startswith("rows"):
            moved = 4 * c[1] + 4 * rows * 8192 + 8 * (nd + 1)
        else:  # ids read and written; sel and two offsets an entry, twice (count, first); out_off, out_docs, src_base written, out_off and src_base read
            moved = 8 * c[1] + 2 * 8 * 3 * nd + 3 * 8 * c[0] + 2 * 8 * c[0]
        med = float(np.median(ms))
        res["cases"].append({"case": k, "counts": c, "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                             "medians_ms": [round(m, 4) for m in ms], "bytes_moved": int(moved), "tb_per_s": round(moved / (med * 1e-3) / 1e12, 3)})
    by = {r["case"]: r for r in res["cases"]}
    y = by["rows_concat_8192_ids_only"]
    res["mark"] = {"yardstick_ms": y["median_ms"], "yardstick_spread_ms": round(y["max_ms"] - y["min_ms"], 4),
                   "identity_ms": by["select_identity"]["median_ms"], "permutation_ms": by["select_permutation"]["median_ms"],
                   "met": bool(max(by["select_identity"]["median_ms"], by["select_permutation"]["median_ms"])
                               <= y["median_ms"] + (y["max_ms"] - y["min_ms"]))}
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
