"""td_span_labels_device on chat ids, held against a dense device-to-device copy of the same ids measured in the same process.

The corpus is td_corpus.chat (--mb MiB, default 1024), encoded with every special token allowed; the spec is the Llama-4 chat
one (opener <|header_start|>assistant<|header_end|>, closers <|eot|>, <|eom|>).  Three things are timed with device events, one
call each, alternating, --reps times after --warmup rounds: the copy (4 B read + 4 B written an id), labels only, and labels +
mask + trained_offsets.  Reported: the medians, the bytes the algorithm needs (`bytes`), the bytes the launches move on top of
them (`bytes_with_workspace`: the bitmap, the ids td_lab_tiles reads, the tiles' words, the per-lane words of trained_offsets),
the ratio to the copy.  The mark (labels only within 1.5 x the copy of the same bytes) is judged twice: against the copy timed here
(torch's copy_ with device events, alternating with the labels), and against the rate tools/gpu_copy_ceiling.py printed in the same
GPU job (--copy-ceiling-log: its output; a host clock around 20 copies of 881 MB), scaled to these bytes; it counts as met only
when both say so.  --bench-parent / --bench-this take files of default `bench.py` result lines of the same job, the parent commit's
and this one's; --kernel-stats takes the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats --output-format csv` run of this tool (a run of its
own).  Prints one JSON line and writes it to --out when given.
usage: python tools/gpu_labels_bench.py [--mb 1024] [--out profiles/labels_cost.json]"""
import argparse
import csv
import json
import re
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--copy-ceiling-log", default=None)
    ap.add_argument("--bench-parent", default=None)
    ap.add_argument("--bench-this", default=None)
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, it does not fall back")
    import td_corpus
    from tokendagger_amd import capi, vocab_io
    name, pat, ranks, special = vocab_io.load_tdv(vocab_io.default_vocab_path())
    tok = capi.HipTokenizer(pat, ranks, special, device=0)
    specials = sorted(special)
    text, doffs = td_corpus.chat(args.mb << 20, seed=0)
    ids, offs = tok.encode_batch_with_special_strs(text, doffs, specials)
    del text
    opener = tok.encode_with_special_strs(b"<|header_start|>assistant<|header_end|>", specials)[0].tolist()
    spec = capi.labels_spec([opener], [special["<|eot|>"], special["<|eom|>"]], -100, True)
    dev = torch.device("cuda", 0)
    n, n_docs = len(ids), len(offs) - 1
    d_ids, d_offs = torch.from_numpy(ids).to(dev), torch.from_numpy(offs).to(dev)
    d_lab, d_copy = torch.empty_like(d_ids), torch.empty_like(d_ids)
    d_mask = torch.empty(n, dtype=torch.uint8, device=dev)
    d_toff = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    d_counts = [torch.zeros(4, dtype=torch.int64, device=dev) for _ in range(2)]
    stream = torch.cuda.current_stream(dev).cuda_stream

    def labels_only():
        tok.span_labels_device(d_ids.data_ptr(), n, d_offs.data_ptr(), n_docs, spec, d_lab.data_ptr(), 0, 0, d_counts[0].data_ptr(), stream)

    def labels_all():
        tok.span_labels_device(d_ids.data_ptr(), n, d_offs.data_ptr(), n_docs, spec, d_lab.data_ptr(), d_mask.data_ptr(), d_toff.data_ptr(),
                               d_counts[1].data_ptr(), stream)

    cases = {"copy": lambda: d_copy.copy_(d_ids), "labels": labels_only, "labels_mask_offsets": labels_all}
    times = {k: [] for k in cases}
    for rep in range(args.warmup + args.reps):
        for k, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                times[k].append(e0.elapsed_time(e1))
    tok.device_status(stream)
    c0, c1 = d_counts[0].cpu().numpy(), d_counts[1].cpu().numpy()
    assert np.array_equal(c0, c1) and int(d_mask.sum(dtype=torch.int64)) == int(c1[0]) and int(d_toff[-1]) == int(c1[0])
    assert int((d_lab != -100).sum()) == int(c1[0])
    med = {k: statistics.median(v) for k, v in times.items()}
    # what the launches move besides the 8 (9) B an id, counted here and not measured: the bitmap zeroed and read by td_lab_apply
    # (n / 8 B each) and by td_lab_tiles for the ids it reads; the offsets read and 4 B read and written a document; td_lab_tiles'
    # ids, by the kernel's rule: backwards from each tile's end in steps of 256 to the first step with an event; a byte a tile
    # written, read, written, read; with trained_offsets 4 B a lane (16 ids) written, 8 B a tile written and read twice, and
    # 8 + 4 + 8 B a document boundary
    ev = np.isin(ids, [special["<|eot|>"], special["<|eom|>"], opener[-1]])
    ev[offs[:-1][offs[:-1] < n]] = True
    tile, step, tiles_read = 4096, 256, 0
    for t0 in range(0, n, tile):
        t1 = min(t0 + tile, n)
        hit = np.flatnonzero(ev[t0:t1])
        back = (t1 - t0) - int(hit[-1]) if len(hit) else t1 - t0
        tiles_read += min(-(-back // step) * step, t1 - t0)
    n_tiles = -(-n // tile)
    work = n // 8 * 2 + tiles_read // 8 + 16 * n_docs + 4 * tiles_read + 4 * n_tiles
    work_all = work + n // 4 + 32 * n_tiles + 20 * (n_docs + 1)
    res = {"tool": "tools/gpu_labels_bench.py", "corpus": f"td_corpus.chat {args.mb} MiB, all specials allowed", "ids": n, "docs": n_docs,
           "counts": c1.tolist(),
           "form": "launches, no look-back: td_lab_docs (offset checks, document-start bitmap), td_lab_tiles (each tile's last event, "
                   "backwards), td_lab_carry (one workgroup), td_lab_apply, td_lab_finish; + td_lab_count_carry with trained_offsets",
           "copy": "torch.Tensor.copy_ of the ids, device events, alternating with the labels calls in this process",
           "reps": args.reps, "median_ms": {k: round(v, 4) for k, v in med.items()},
           "min_ms": {k: round(min(v), 4) for k, v in times.items()}, "max_ms": {k: round(max(v), 4) for k, v in times.items()},
           "bytes": {"copy": 8 * n, "labels": 8 * n, "labels_mask_offsets": 9 * n + 8 * (n_docs + 1)},
           "bytes_with_workspace": {"labels": 8 * n + work, "labels_mask_offsets": 9 * n + 8 * (n_docs + 1) + work_all},
           "ids_read_by_td_lab_tiles": tiles_read,
           "tb_per_s_on_bytes": {k: round(b / med[k] / 1e9, 3) for k, b in (("copy", 8 * n), ("labels", 8 * n),
                                                                            ("labels_mask_offsets", 9 * n + 8 * (n_docs + 1)))},
           "labels_over_copy": round(med["labels"] / med["copy"], 3), "all_over_copy": round(med["labels_mask_offsets"] / med["copy"], 3),
           "mark": "labels <= 1.5 x copy", "mark_met": bool(med["labels"] <= 1.5 * med["copy"])}
    if args.copy_ceiling_log:
        m = re.search(r"dense copy of (\d+) MB: ([\d.]+) ms = ([\d.]+) TB/s", Path(args.copy_ceiling_log).read_text())
        if not m:
            raise SystemExit("no dense-copy line in " + args.copy_ceiling_log)
        ms_same = 8 * n / (2 * int(m.group(1)) * 1e6 / float(m.group(2)))
        res["copy_ceiling_tool"] = {"tool": "tools/gpu_copy_ceiling.py, same GPU job", "mb": int(m.group(1)), "ms": float(m.group(2)),
                                    "tb_per_s": float(m.group(3)), "ms_for_these_bytes": round(ms_same, 4),
                                    "labels_over_ceiling": round(med["labels"] / ms_same, 3)}
        res["mark_met"] = bool(res["mark_met"] and med["labels"] <= 1.5 * ms_same)
    if args.kernel_stats:
        with open(args.kernel_stats, newline="") as f:
            rows = [r for r in csv.DictReader(f) if "td_lab" in r.get("Name", "") or "opy" in r.get("Name", "")]
        res["kernel_trace"] = {}
        for r in rows:
            m = re.search(r"td_lab_\w+", r["Name"])
            res["kernel_trace"][m.group(0) if m else r["Name"][:100]] = {
                "calls": int(r["Calls"]), "mean_us": round(float(r["AverageNs"]) / 1e3, 1), "min_us": round(float(r["MinNs"]) / 1e3, 1),
                "max_us": round(float(r["MaxNs"]) / 1e3, 1)}
    for key, path in (("parent", args.bench_parent), ("this", args.bench_this)):
        if path:
            runs = [json.loads(ln) for ln in Path(path).read_text().splitlines() if ln.startswith("{")]
            res.setdefault("default_bench_line_same_job", {})[key] = {"gb_per_s": [r.get("value") for r in runs],
                                                                      "ms_per_step": [r.get("ms_per_step") for r in runs]}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
