"""Cost of window rows: 1 GiB of English encoded with td_encode_device, then td_window_rows_device on the device
ids, beside td_make_rows_device on the same input in the same process; HIP-event medians over `steps` single calls after
`warmup`, the yardstick's median taken `repeats` times so that its spread is known.  The bytes each case must move are counted
from the shapes (ids read, rows written, offsets read twice by the scan and once by the slots, first_row written and read, the
per-row outputs); the rate is those bytes over the median, and its share of the 6.29 TB/s a device-to-device copy reaches
(tools/gpu_copy_ceiling.py).

  A  windows against PAD: S = 2048, overlap 0, BOS + EOS, the documents as they are
  B  long documents: every 512th offset (documents of about 64 Ki ids), S = 8192, overlap 0 and 1024, beside CONCAT

usage: gpu_windows_bench.py [--size-mb 1024] [--steps 10] [--warmup 3] [--repeats 3] [--json OUT]
Kernel times: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/gpu_windows_bench.py`, in a run of its own.
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
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
    res = {"corpus": "english", "size_mb": args.size_mb, "docs": nd, "ids": ntok, "steps": args.steps, "cases": []}

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

    def record(name, S, overlap, c, medians, moved, n_docs, extra=None):
        ms = float(np.median(medians))
        row = {"case": name, "seq_len": S, "overlap": overlap, "docs": n_docs, "rows": c[0], "real_slots": c[1], "counts_2": c[2],
               "counts_3": c[3], "median_ms": round(ms, 4), "medians_ms": [round(m, 4) for m in medians], "bytes_moved": int(moved),
               "tb_per_s": round(moved / (ms * 1e-3) / 1e12, 3), "copy_rate_share": round(moved / (ms * 1e-3) / COPY_RATE, 3)}
        row.update(extra or {})
        res["cases"].append(row)

    def windows_case(name, d_offs, h_offs, S, overlap, repeats):
        n_docs = len(h_offs) - 1
        sp = capi.windows_spec(S, BOS, EOS, 0)
        rows = int(capi.window_plan(h_offs, sp, overlap)[0])
        out = torch.empty(rows * S, dtype=torch.int32, device="cuda")
        lens = torch.empty(rows, dtype=torch.int32, device="cuda")
        docs = torch.empty(rows, dtype=torch.int64, device="cuda")
        starts = torch.empty(rows, dtype=torch.int64, device="cuda")
        counts = torch.zeros(4, dtype=torch.int64, device="cuda")
        medians = [timed(lambda: tok.window_rows_device(dk.data_ptr(), cap, d_offs.data_ptr(), n_docs, sp, overlap, out.data_ptr(), rows, 0,
                                                        lens.data_ptr(), docs.data_ptr(), starts.data_ptr(), counts.data_ptr(), s))
                   for _ in range(repeats)]
        c = counts.cpu().tolist()
        body = c[1] - 2 * c[0]  # ids read: the real slots without the rows' BOS and EOS
        moved = 4 * body + 4 * rows * S + 3 * 8 * (n_docs + 1) + 2 * 8 * (n_docs + 1) + 20 * rows
        record(name, S, overlap, c, medians, moved, n_docs, {"scan_and_row_bytes": int(5 * 8 * (n_docs + 1) + 20 * rows)})
        return medians

    def rows_case(name, d_offs, n_docs, S, layout, repeats):
        sp = capi.rows_spec(S, layout, BOS, EOS, 0)
        rows = capi.rows_capacity_of(sp, ntok, n_docs)
        out = torch.empty(rows * S, dtype=torch.int32, device="cuda")
        aux = torch.empty(n_docs, dtype=torch.int32, device="cuda") if layout == capi.TD_ROWS_PAD else None
        counts = torch.zeros(4, dtype=torch.int64, device="cuda")
        medians = [timed(lambda: tok.make_rows_device(dk.data_ptr(), cap, d_offs.data_ptr(), n_docs, sp, out.data_ptr(), rows, 0,
                                                      aux.data_ptr() if aux is not None else 0, counts.data_ptr(), s))
                   for _ in range(repeats)]
        c = counts.cpu().tolist()
        ids_read = 4 * c[1] if layout == capi.TD_ROWS_CONCAT else 4 * min(c[1], ntok)
        moved = ids_read + 4 * rows * S + 8 * (n_docs + 1) + (4 * n_docs if aux is not None else 0)
        record(name, S, 0, c, medians, moved, n_docs)
        return medians

    # A: PAD first and last, windows between, so that a drift of the machine shows in the yardstick's own spread
    pad1 = rows_case("A_pad_2048_before", dto, nd, 2048, capi.TD_ROWS_PAD, args.repeats)
    win = windows_case("A_windows_2048", dto, toffs, 2048, 0, args.repeats)
    pad2 = rows_case("A_pad_2048_after", dto, nd, 2048, capi.TD_ROWS_PAD, args.repeats)
    pads = pad1 + pad2
    res["A"] = {"pad_median_ms": round(float(np.median(pads)), 4), "pad_min_ms": round(min(pads), 4), "pad_max_ms": round(max(pads), 4),
                "windows_median_ms": round(float(np.median(win)), 4), "windows_min_ms": round(min(win), 4), "windows_max_ms": round(max(win), 4)}
    # B: documents of about 64 Ki ids
    long_offs = np.ascontiguousarray(np.concatenate([toffs[:-1:512], toffs[-1:]]))
    d_long = torch.from_numpy(long_offs).cuda()
    rows_case("B_concat_8192", d_long, len(long_offs) - 1, 8192, capi.TD_ROWS_CONCAT, 1)
    windows_case("B_windows_8192_overlap_0", d_long, long_offs, 8192, 0, 1)
    windows_case("B_windows_8192_overlap_1024", d_long, long_offs, 8192, 1024, 1)
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
