"""Cost of the field joins: 1 GiB of English encoded with td_encode_device, then td_join_fields_device on the
device ids, ids + labels, K = 2 (BOS prompt SEP completion EOS, consecutive documents taken as prompt and completion), beside its
yardstick in the same process: td_select_docs_device with the identity list and a label stream on the same ids, the project's
near-copy of this access pattern (two streams read, two written; the join reads one and writes two, or three with types).  Cases:
the join with no limit, the join with max_total at the median example (both shrink modes), the join with the type stream as well.
The cases alternate `repeats` times; each time a case's figure is the HIP-event median over `steps` single calls after `warmup`,
and the report gives the median of those and their smallest and largest, with ns per id written.

usage: gpu_join_bench.py [--size-mb 1024] [--steps 10] [--warmup 3] [--repeats 5] [--json OUT]
Kernel times: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/gpu_join_bench.py`, in a run of its own.
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

BOS, EOS, SEP = 200000, 200001, 7


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
    print(f"building {args.size_mb} MiB of English", file=sys.stderr, flush=True)
    x, offs = bench.build_corpus("english", n, 1000)
    nd = (len(offs) - 1) // 2 * 2
    n_ex = nd // 2
    dt = torch.from_numpy(x).cuda()
    do = torch.from_numpy(offs).cuda()
    cap = n // 3
    dk = torch.empty(cap, dtype=torch.int32, device="cuda")
    dto = torch.empty(len(offs), dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    tok.encode_device(dt.data_ptr(), n, do.data_ptr(), len(offs) - 1, dk.data_ptr(), cap, dto.data_ptr(), s)
    tok.device_status(s)
    del dt
    toffs = dto.cpu().numpy()[:nd + 1]
    ntok = int(toffs[nd])
    d_lab = dk.clone()  # the yardstick's second stream

    def spec(max_total=None, shrink="order"):
        F = capi.join_field
        return capi.join_spec([F([BOS], shrink_rank=1, keep_tail=True), F([SEP], shrink_rank=2, train=True, type_value=1)], tail=[EOS],
                              tail_type=1, train_tail=True, max_total=max_total, shrink=shrink)

    full = capi.join_plan(toffs, spec())
    T = int(full[0][1])
    median_ex = int(np.median(np.diff(full[1])))

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

    out = torch.empty(T, dtype=torch.int32, device="cuda")
    out_lab = torch.empty(T, dtype=torch.int32, device="cuda")
    out_typ = torch.empty(T, dtype=torch.int32, device="cuda")
    o_off = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
    o_docs = torch.empty(nd, dtype=torch.int64, device="cuda")
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")

    def join(sp, types=False):
        return lambda: tok.join_fields_device(dk.data_ptr(), cap, dto.data_ptr(), nd, sp, out.data_ptr(), T, o_off.data_ptr(), counts.data_ptr(),
                                              d_out_labels=out_lab.data_ptr(), d_out_types=out_typ.data_ptr() if types else 0,
                                              d_out_examples=o_docs.data_ptr(), stream=s)

    cases = {
        "select_identity_labeled": lambda: tok.select_docs_device(dk.data_ptr(), cap, dto.data_ptr(), nd, 0, nd, capi.select_spec(), out.data_ptr(),
                                                                  T, o_off.data_ptr(), o_docs.data_ptr(), counts.data_ptr(), d_lab.data_ptr(),
                                                                  out_lab.data_ptr(), s),
        "join_labeled": join(spec()),
        "join_labeled_types": join(spec(), types=True),
        "join_labeled_max_total_median_order": join(spec(median_ex, "order")),
        "join_labeled_max_total_median_longest": join(spec(median_ex, "longest")),
    }
    medians = {k: [] for k in cases}
    got = {}
    for _ in range(args.repeats):
        for k, fn in cases.items():
            medians[k].append(timed(fn))
            got[k] = counts.cpu().tolist()
    res = {"corpus": "english", "size_mb": args.size_mb, "docs": nd, "examples": n_ex, "ids": ntok, "median_example": median_ex,
           "steps": args.steps, "repeats": args.repeats, "box": {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
                   "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "hip": torch.version.hip}, "cases": []}
    for k, ms in medians.items():
        c = got[k]
        streams_read, streams_written = (2, 2) if k.startswith("select") else (1, 3 if "types" in k else 2)
        read = ntok if k.startswith("select") or "max_total" not in k else c[1]  # (ids a cut example does not keep are not read)
        moved = 4 * (streams_read * read + streams_written * c[1])
        med = float(np.median(ms))
        res["cases"].append({"case": k, "counts": c, "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                             "medians_ms": [round(m, 4) for m in ms], "stream_bytes": int(moved), "ns_per_id_written": round(med * 1e6 / max(c[1], 1), 5),
                             "tb_per_s": round(moved / (med * 1e-3) / 1e12, 3)})
    by = {r["case"]: r for r in res["cases"]}
    y = by["select_identity_labeled"]
    res["ratios"] = {k: {"time_to_select": round(r["median_ms"] / y["median_ms"], 3),
                         "per_id_to_select": round(r["ns_per_id_written"] / y["ns_per_id_written"], 3),
                         "stream_bytes_to_select": round(r["stream_bytes"] / y["stream_bytes"], 3)} for k, r in by.items() if k != y["case"]}
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
