"""Cost of decode: 1 GiB of English encoded once with td_encode_device and kept resident, then
(a) td_decode_rows_device with the plain spec in the offsets form (the documents' offsets),
(b) the same ids as [R, 2048] rows of 2040 ids, one EOS and seven pads, with the pad skipped and EOS as stop,
(c) td_decode_device on the same ids (the decode of rounds 1 - 3, unchanged: its first figure of record),
(d) a dense device-to-device copy of (a)'s ids plus its output bytes, as the floor.
The cases alternate `repeats` times; each time a case's figure is the median over `steps` windows after `warmup` calls, a window
being as many back-to-back calls between two HIP events as fill about `window_ms`, divided by their number; the report gives the
median of those and their smallest and largest, and the ratios (a) / (c) and (a) / (d).  Before anything is timed every case is
compared with the bytes it must give: (a) and (c) with the text that was encoded and its document offsets, (b) with the plain decode
of the ids its rows hold.

usage: gpu_decode_rows_bench.py [--size-mb 1024] [--steps 10] [--warmup 3] [--repeats 5] [--window-ms 20] [--json OUT]
Kernel times: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/gpu_decode_rows_bench.py`, in a run of its own.
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

EOS = 200001
ROW, BODY = 2048, 2040


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
    pad = max(max(ranks.values()), max(special.values()) if special else 0) + 1  # n_vocab: above the vocabulary
    n = args.size_mb << 20
    x, offs = bench.build_corpus("english", n, 1000)
    nd = len(offs) - 1
    text = torch.from_numpy(x).cuda()
    do = torch.from_numpy(offs).cuda()
    cap = n // 3
    dk = torch.empty(cap, dtype=torch.int32, device="cuda")
    dto = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    tok.encode_device(text.data_ptr(), n, do.data_ptr(), nd, dk.data_ptr(), cap, dto.data_ptr(), s)
    tok.device_status(s)
    ntok = int(dto[nd].item())
    real = dk[:ntok]
    n_rows = ntok // BODY
    rows = torch.full((n_rows, ROW), pad, dtype=torch.int32, device="cuda")
    rows[:, :BODY] = real[:n_rows * BODY].view(n_rows, BODY)
    rows[:, BODY] = EOS
    rows[:, BODY + 1] = 5  # what lies behind the stop is not looked at

    out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    out_offs = torch.empty(max(nd, n_rows) + 1, dtype=torch.int64, device="cuda")
    seg_ids = torch.empty(max(nd, n_rows), dtype=torch.int64, device="cuda")
    info = torch.zeros(4, dtype=torch.int64, device="cuda")
    n_bytes = torch.zeros(1, dtype=torch.int64, device="cuda")
    ids_copy = torch.empty(ntok, dtype=torch.int32, device="cuda")
    bytes_copy = torch.empty(n, dtype=torch.uint8, device="cuda")
    plain = capi.decode_spec()
    padded = capi.decode_spec(ROW, skip=[pad], stop=[EOS])
    one = torch.tensor([0, n_rows * BODY], dtype=torch.int64, device="cuda")

    def a_plain():
        tok.decode_rows_device(real.data_ptr(), ntok, dto.data_ptr(), 0, nd, plain, out.data_ptr(), n, out_offs.data_ptr(), seg_ids.data_ptr(),
                               info.data_ptr(), s)

    def b_rows():
        tok.decode_rows_device(rows.data_ptr(), n_rows * ROW, 0, 0, n_rows, padded, out.data_ptr(), n, out_offs.data_ptr(), seg_ids.data_ptr(),
                               info.data_ptr(), s)

    def c_old():
        tok.decode_device(real.data_ptr(), ntok, out.data_ptr(), n, n_bytes.data_ptr(), s)

    def d_copy():
        ids_copy.copy_(real)
        bytes_copy.copy_(text)

    # before anything is timed: every case against the bytes it must give
    out.zero_()
    a_plain()
    tok.device_status(s)
    assert torch.equal(out[:n], text) and torch.equal(out_offs[:nd + 1], do), "plain decode rows"
    assert info.tolist() == [n, ntok, 0, 0] and torch.equal(seg_ids[:nd], dto[1:] - dto[:-1])
    out.zero_()
    c_old()
    tok.device_status(s)
    assert torch.equal(out[:n], text) and int(n_bytes.item()) == n, "td_decode_device"
    tok.decode_rows_device(real.data_ptr(), ntok, one.data_ptr(), 0, 1, plain, bytes_copy.data_ptr(), n, out_offs.data_ptr(), 0, info.data_ptr(), s)
    tok.device_status(s)
    body_bytes = int(info[0].item())
    out.zero_()
    b_rows()
    tok.device_status(s)
    assert info.tolist() == [body_bytes, n_rows * BODY, n_rows, n_rows], info.tolist()
    assert torch.equal(out[:body_bytes], bytes_copy[:body_bytes]) and bool((seg_ids[:n_rows] == BODY + 1).all()), "padded rows"

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
        if k not in inner:
            inner[k] = int(min(max(round(args.window_ms / max(window(fn, 1), 1e-3)), 1), 256))
        ts = [window(fn, inner[k]) for _ in range(args.steps)]
        tok.device_status(s)
        return float(np.median(ts))

    cases = {"a_decode_rows_plain_offsets": a_plain, "b_decode_rows_padded_2048": b_rows, "c_td_decode_device": c_old, "d_dense_copy": d_copy}
    medians = {k: [] for k in cases}
    for _ in range(args.repeats):
        for k, fn in cases.items():
            medians[k].append(timed(k, fn))
    res = {"corpus": "english", "size_mb": args.size_mb, "docs": nd, "ids": ntok, "rows": n_rows, "row_ids": ROW, "steps": args.steps,
           "repeats": args.repeats, "window_ms": args.window_ms, "cases": []}
    for k, ms in medians.items():
        med = float(np.median(ms))
        res["cases"].append({"case": k, "calls_per_window": inner[k], "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                             "medians_ms": [round(m, 4) for m in ms]})
    by = {r["case"]: r for r in res["cases"]}
    a, b, c, d = (by[k] for k in cases)
    spread = c["max_ms"] - c["min_ms"]
    res["mark"] = {"a_over_c": round(a["median_ms"] / c["median_ms"], 4), "a_over_d": round(a["median_ms"] / d["median_ms"], 4),
                   "b_over_a": round(b["median_ms"] / a["median_ms"], 4), "c_spread_ms": round(spread, 4),
                   "a_no_slower_than_c_within_its_spread": bool(a["median_ms"] <= c["median_ms"] + spread),
                   "a_gb_per_s_of_output": round(n / a["median_ms"] / 1e6, 1), "c_gb_per_s_of_output": round(n / c["median_ms"] / 1e6, 1)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
