"""Cost of the line filter, on resident text: --size-mb (1024) of the bench's English corpus and of its mixed corpus, each
  line_filter c4         td_line_filter_device with a C4-like rule set (three words, a terminal mark, no word above 1000 bytes, seven
                         drop-line phrases, two count-doc phrases)
  line_filter identity   the empty rule set: every byte is copied once, as td_utf8_device does on well-formed text
  line_filter stats      the C4-like rule set with no output: the decision alone
beside, on the same buffers in the same process,
  utf8_device            td_utf8_device, policy replace
  text_stats             td_text_stats_device, LOCAL + RUNS
  encode_device          td_encode_device
Before anything is timed the device results are held against td_line_filter_host on the first MiB.  A case's figure is the median over
`steps` windows after `warmup` calls, a window being as many back-to-back calls between two HIP events as fill about `window_ms`; the
minimum and the maximum are reported beside it.  The cases are timed in turn, twice over, so that a drift shows as a pair that differs.

usage: gpu_linefilter_bench.py [--size-mb 1024] [--steps 7] [--warmup 2] [--window-ms 200] [--json OUT] [--only CASE]
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

DROP = (b"javascript", b"privacy policy", b"terms of use", b"cookie policy", b"uses cookies", b"use of cookies", b"use cookies")
COUNT = (b"lorem ipsum", b"{")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mb", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--json", default="")
    ap.add_argument("--only", default="", help="time only the cases whose name contains this (a profiler run on one case)")
    args = ap.parse_args()
    _, pat, ranks, special = vocab_io.load_tdv(vocab_io.default_vocab_path())
    tok = capi.HipTokenizer(pat, ranks, special, device=0)
    side = torch.cuda.Stream()  # (the device forms do not take the null stream)
    s = side.cuda_stream
    c4 = capi.LineRules.make(3, 1000, capi.TD_LF_NEED_TERMINAL,
                             [(capi.TD_LF_PHRASE_DROP_LINE, p) for p in DROP] + [(capi.TD_LF_PHRASE_COUNT_DOC, p) for p in COUNT])
    identity = capi.LineRules.make()
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
            out = torch.empty(n + 4096, dtype=torch.uint8, device="cuda")
            ooff = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
            stats = torch.empty((max(nd, 1), capi.TD_TS_COLS), dtype=torch.int64, device="cuda")
            totals = torch.empty(capi.TD_TS_COLS, dtype=torch.int64, device="cuda")
            counts = torch.zeros(8, dtype=torch.int64, device="cuda")
            ids = torch.empty(n, dtype=torch.int32, device="cuda")
            toff = torch.empty(nd + 1, dtype=torch.int64, device="cuda")

        def lf(rules, write=True):
            return lambda: tok.line_filter_device(dt.data_ptr(), n, do.data_ptr(), nd, rules, out.data_ptr() if write else 0, n if write else 0,
                                                  ooff.data_ptr() if write else 0, stats.data_ptr(), totals.data_ptr(), counts.data_ptr(), s)

        # sanity, before anything is timed: the first MiB's documents against the host statement, under both rule sets
        kd = int(np.searchsorted(offs, 1 << 20, side="right")) - 1
        kept = {}
        for label, rules in (("c4", c4), ("identity", identity)):
            want = capi.line_filter_host(x[:int(offs[kd])], offs[:kd + 1], rules)
            lf(rules)()
            tok.device_status(s)
            side.synchronize()
            assert np.array_equal(ooff[:kd + 1].cpu().numpy(), want[1]) and bytes(out[:int(want[1][-1])].cpu().numpy()) == bytes(want[0]), (name, label)
            assert np.array_equal(stats.view(-1)[:kd * 8].cpu().numpy().reshape(kd, 8), want[2]), (name, label, "stats")
            kept[label] = {"bytes": int(counts.cpu()[0]), "totals": totals[:8].cpu().tolist()}
        assert kept["identity"]["bytes"] == n
        res["corpora"][name] = {"bytes": n, "docs": nd, "kept": kept}
        cases = {
            "line_filter c4": lf(c4), "line_filter identity": lf(identity), "line_filter stats": lf(c4, write=False),
            "utf8_device": lambda: tok.utf8_device(dt.data_ptr(), n, do.data_ptr(), nd, capi.TD_UTF8_REPLACE, out.data_ptr(), n + 4096, ooff.data_ptr(),
                                                   0, 0, 0, counts.data_ptr(), s),
            "text_stats": lambda: tok.text_stats_device(dt.data_ptr(), n, do.data_ptr(), nd, capi.TD_TS_ALL, stats.data_ptr(), totals.data_ptr(), s),
            "encode_device": lambda: tok.encode_device(dt.data_ptr(), n, do.data_ptr(), nd, ids.data_ptr(), n, toff.data_ptr(), stream=s),
        }
        for turn in (1, 2):
            for k, fn in cases.items():
                if args.only and args.only not in f"{name}/{k}":
                    continue
                med, lo, hi, inner = timed(fn)
                res["cases"].append({"corpus": name, "case": k, "turn": turn, "calls_per_window": inner, "median_ms": round(med, 4),
                                     "min_ms": round(lo, 4), "max_ms": round(hi, 4), "input_gb_per_s": round(n / med / 1e6, 1)})
        ms = {k: float(np.mean([c["median_ms"] for c in res["cases"] if c["corpus"] == name and c["case"] == k])) for k in cases
              if any(c["corpus"] == name and c["case"] == k for c in res["cases"])}
        if len(ms) == len(cases):
            res["corpora"][name]["ratios"] = {
                "c4 / utf8_device": round(ms["line_filter c4"] / ms["utf8_device"], 3),
                "c4 / encode_device": round(ms["line_filter c4"] / ms["encode_device"], 4),
                "identity / utf8_device": round(ms["line_filter identity"] / ms["utf8_device"], 3),
                "identity / (utf8_device + text_stats)": round(ms["line_filter identity"] / (ms["utf8_device"] + ms["text_stats"]), 3),
            }
        del dt, do, out, ooff, stats, totals, ids, toff
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
