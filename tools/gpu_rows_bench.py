"""Cost of training rows: 1 GiB of English encoded with td_encode_device, then td_make_rows_device on the device
ids; HIP-event medians over `steps` single calls after `warmup`.  The bytes each case must move are counted from the shapes (ids
read, rows written, offsets read, positions / cu_seqlens written); the rate is those bytes over the median, and its share of
the 6.29 TB/s a device-to-device copy reaches (tools/gpu_copy_ceiling.py).

usage: gpu_rows_bench.py [--size-mb 1024] [--steps 20] [--warmup 3] [--json OUT]
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

COPY_RATE = 6.29e12
BOS, EOS = 200000, 200001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mb", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
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
    ntok = int(dto[nd].item())
    res = {"corpus": "english", "size_mb": args.size_mb, "docs": nd, "ids": ntok, "funnel_src": os.environ.get("TD_ROWS_FUNNEL", "0") == "1",
           "cases": []}

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

    for name, S, layout, positions, cu in (("concat_ids", 8192, capi.TD_ROWS_CONCAT, False, False),
                                          ("concat_cu_seqlens", 8192, capi.TD_ROWS_CONCAT, False, True),
                                          ("concat_positions", 8192, capi.TD_ROWS_CONCAT, True, False),
                                          ("pad_2048", 2048, capi.TD_ROWS_PAD, False, True)):
        sp = capi.rows_spec(S, layout, BOS, EOS, 0)
        rows = capi.rows_capacity_of(sp, ntok, nd)
        out = torch.empty(rows * S, dtype=torch.int32, device="cuda")
        pos = torch.empty(rows * S, dtype=torch.int32, device="cuda") if positions else None
        aux = torch.empty(nd + rows + 1, dtype=torch.int32, device="cuda") if cu else None
        counts = torch.zeros(4, dtype=torch.int64, device="cuda")
        ms = timed(lambda: tok.make_rows_device(dk.data_ptr(), cap, dto.data_ptr(), nd, sp, out.data_ptr(), rows,
                                                pos.data_ptr() if pos is not None else 0, aux.data_ptr() if aux is not None else 0,
                                                counts.data_ptr(), s))
        c = counts.cpu().tolist()
        real = c[1]
        ids_read = 4 * real if layout == capi.TD_ROWS_CONCAT else 4 * min(real, ntok)
        moved = ids_read + 4 * rows * S + 8 * (nd + 1)
        if positions:
            moved += 4 * rows * S
        if cu and layout == capi.TD_ROWS_CONCAT:
            moved += 8 * (nd + 1) + 4 * (c[2] + 1)
        if cu and layout == capi.TD_ROWS_PAD:
            moved += 4 * nd
        del out, pos, aux
        res["cases"].append({"case": name, "seq_len": S, "rows": c[0], "real_slots": real, "segments": c[2], "truncated": c[3],
                             "median_ms": round(ms, 4), "bytes_moved": int(moved), "tb_per_s": round(moved / (ms * 1e-3) / 1e12, 3),
                             "copy_rate_share": round(moved / (ms * 1e-3) / COPY_RATE, 3)})
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
