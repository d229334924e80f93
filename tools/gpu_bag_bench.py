"""Cost of the bag models, on resident text: --size-mb (1024) of the bench's English corpus
  lid best / lid probs    a seeded lid.176-shaped model (dim 16, character 2-4-grams, 2 M buckets, 176 labels, hierarchical softmax),
                          best and best_prob only, and with d_probs
  dclm best / dclm probs  a seeded DCLM-shaped model (dim 256, word bigrams, 2 M buckets, 2 labels, softmax)
beside, on the same buffer in the same process,
  utf8_check              td_utf8_check_device: the frame's read-speed pass
  400 entries             td_word_matches_device with a seeded list of 400 entries, as gpu_wordlist_bench.py has it
Before anything is timed the device results are held against td_bag_classify_host on the first 256 KiB.  A case's figure is the median
over `steps` windows after `warmup` calls, a window being as many back-to-back calls between two HIP events as fill about `window_ms`.
The cases are timed in turn, twice over.  Rows gathered a second and the bytes they imply come from the FEATURES total.

usage: gpu_bag_bench.py [--size-mb 1024] [--steps 5] [--warmup 1] [--window-ms 200] [--json OUT] [--only CASE]
Kernel times: run this tool under rocprofv3 (--kernel-trace --stats) with --only, in a run of its own.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from tokendagger_amd import capi, vocab_io  # noqa: E402
from tools.gpu_wordlist_bench import seeded_list  # noqa: E402


def seeded_model(seed, dim, n_labels, loss, bucket, minn, maxn, word_ngrams, words):
    rng = np.random.default_rng(seed)
    draw = lambda r, c: (rng.integers(-128, 129, size=(r, c), dtype=np.int16) / np.float32(64)).astype(np.float32)  # noqa: E731
    counts = sorted((int(1e6 / (i + 1)) + 1 for i in range(n_labels)), reverse=True) if loss == capi.TD_BAG_HS else None
    return capi.BagSpec(words, draw(len(words) + bucket, dim), draw(n_labels - (loss == capi.TD_BAG_HS), dim), bucket=bucket, minn=minn,
                        maxn=maxn, word_ngrams=word_ngrams, loss=loss, label_counts=counts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mb", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--json", default="")
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    _, pat, ranks, special = vocab_io.load_tdv(vocab_io.default_vocab_path())
    tok = capi.HipTokenizer(pat, ranks, special, device=0)
    side = torch.cuda.Stream()
    s = side.cuda_stream
    res = {"steps": args.steps, "window_ms": args.window_ms, "models": {}, "cases": []}

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
        for _ in range(args.warmup):
            fn()
        side.synchronize()
        tok.device_status(s)
        inner = int(min(max(round(args.window_ms / max(window(fn, 1), 1e-3)), 1), 64))
        ts = [window(fn, inner) for _ in range(args.steps)]
        tok.device_status(s)
        return float(np.median(ts)), float(min(ts)), float(max(ts)), inner

    x, offs = bench.build_corpus("english", args.size_mb << 20, 1000)
    n, nd = len(x), len(offs) - 1
    words = [b"the", b"of", b"and", b"to", b"in", b"</s>"] + seeded_list(2000, 11)
    specs = {"lid": seeded_model(1, 16, 176, capi.TD_BAG_HS, 2000000, 2, 4, 1, words),
             "dclm": seeded_model(2, 256, 2, capi.TD_BAG_SOFTMAX, 2000000, 0, 0, 2, words)}
    with torch.cuda.stream(side):
        dt, do = torch.from_numpy(x).cuda(), torch.from_numpy(offs).cuda()
        best = torch.empty(nd, dtype=torch.int32, device="cuda")
        bprob = torch.empty(nd, dtype=torch.float32, device="cuda")
        probs = torch.empty((nd, 176), dtype=torch.float32, device="cuda")
        stats = torch.empty((nd, 8), dtype=torch.int64, device="cuda")
        totals = torch.empty(8, dtype=torch.int64, device="cuda")
        hits = torch.empty(400, dtype=torch.int64, device="cuda")
        flags = torch.empty(nd, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(8, dtype=torch.int64, device="cuda")
    kd = int(np.searchsorted(offs, 256 << 10, side="right")) - 1
    cases, keep = {}, []
    for name, spec in specs.items():
        bm = tok.bag_model(spec)
        keep.append(bm)
        want = capi.bag_classify_host(spec, x[:int(offs[kd])], offs[:kd + 1], capi.TD_BAG_EOS, probs=False, hidden=False)
        for label, pp in ((name + " best", 0), (name + " probs", probs.data_ptr())):
            fn = (lambda bm=bm, pp=pp: tok.bag_classify_device(bm, dt.data_ptr(), n, do.data_ptr(), nd, capi.TD_BAG_EOS, best.data_ptr(),
                                                               bprob.data_ptr(), pp, 0, stats.data_ptr(), totals.data_ptr(), s))
            fn()
            tok.device_status(s)
            side.synchronize()
            assert np.array_equal(stats.view(-1)[:kd * 4].cpu().numpy().reshape(kd, 4), want["stats"]), (label, "stats")
            res["models"][name] = dict(bm.info, totals=totals[:4].cpu().tolist(), row_bytes=int(spec.dim + 3 & ~3) * 4)
            cases[label] = fn
    ws = tok.word_set(seeded_list(400, 7), None)
    cases["utf8_check"] = lambda: tok.utf8_check(dt.data_ptr(), n, do.data_ptr(), nd, flags.data_ptr(), 0, counts.data_ptr(), s)
    cases["400 entries"] = lambda: tok.word_matches_device(ws, dt.data_ptr(), n, do.data_ptr(), nd, 0, stats.data_ptr(), totals.data_ptr(), hits.data_ptr(), s)
    res["text"] = {"bytes": n, "docs": nd}
    for turn in (1, 2):
        for k, fn in cases.items():
            if args.only and not any(o in k for o in args.only.split(",")):
                continue
            med, lo, hi, inner = timed(fn)
            res["cases"].append({"case": k, "turn": turn, "calls_per_window": inner, "median_ms": round(med, 4), "min_ms": round(lo, 4),
                                 "max_ms": round(hi, 4)})
    ms = {k: [c["median_ms"] for c in res["cases"] if c["case"] == k] for k in cases}
    if all(len(v) == 2 for v in ms.values()):
        for ref in ("utf8_check", "400 entries"):
            u = float(np.mean(ms[ref]))
            res[f"ratios_to_{ref.replace(' ', '_')}"] = {k: round(float(np.mean(v)) / u, 3) for k, v in ms.items()}
        for name in specs:
            t = float(np.mean(ms[name + " best"])) * 1e-3
            rows = res["models"][name]["totals"][2]
            res["models"][name].update(rows_per_s=round(rows / t), gather_gb_per_s=round(rows * res["models"][name]["row_bytes"] / t / 1e9, 1),
                                       text_gb_per_s=round(n / t / 1e9, 2))
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
