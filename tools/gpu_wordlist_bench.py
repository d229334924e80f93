"""Cost of the word-list matches, on resident text: --size-mb (1024) of the bench's English corpus
  stop words             td_word_matches_device with Gopher's eight stop words, one group each: a resident set, a hit every few words
  400 entries            a seeded list of 400 lower-case entries of 3 to 14 letters, resident in LDS
  400 entries global     the same set under TD_WL_NO_LDS: probed in global memory
  5000 entries           a seeded list of 5 000 entries: above the LDS budget, probed in global memory
beside, on the same buffer in the same process,
  utf8_check             td_utf8_check_device: the frame's read-speed pass
  mask clean             td_mask_addresses_device on the corpus as it is, which has no address: the nearest comparable pass
Before anything is timed the device results are held against td_word_matches_host on the first MiB.  A case's figure is the median over
`steps` windows after `warmup` calls, a window being as many back-to-back calls between two HIP events as fill about `window_ms`; the
minimum and the maximum are reported beside it.  The cases are timed in turn, twice over, so that a drift shows as a pair that differs.

usage: gpu_wordlist_bench.py [--size-mb 1024] [--steps 7] [--warmup 2] [--window-ms 200] [--json OUT] [--only CASE]
Kernel times: run this tool under rocprofv3 (--kernel-trace --stats) with --only, in a run of its own.
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from tokendagger_amd import capi, vocab_io  # noqa: E402

STOP = [b"the", b"be", b"to", b"of", b"and", b"that", b"have", b"with"]


def seeded_list(n, seed):
    rnd, seen = random.Random(seed), set()
    while len(seen) < n:
        seen.add(bytes(rnd.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randrange(3, 15))))
    return sorted(seen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mb", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--json", default="")
    ap.add_argument("--only", default="", help="time only the cases whose name contains one of these, comma-separated (a profiler run)")
    args = ap.parse_args()
    _, pat, ranks, special = vocab_io.load_tdv(vocab_io.default_vocab_path())
    tok = capi.HipTokenizer(pat, ranks, special, device=0)
    side = torch.cuda.Stream()  # (the device forms do not take the null stream)
    s = side.cuda_stream
    res = {"steps": args.steps, "window_ms": args.window_ms, "sets": {}, "cases": []}

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

    x, offs = bench.build_corpus("english", args.size_mb << 20, 1000)
    n, nd = len(x), len(offs) - 1
    lists = {"stop words": (STOP, list(range(8))), "400 entries": (seeded_list(400, 7), None), "5000 entries": (seeded_list(5000, 9), None)}
    with torch.cuda.stream(side):
        dt, do = torch.from_numpy(x).cuda(), torch.from_numpy(offs).cuda()
        stats = torch.empty((nd, 8), dtype=torch.int64, device="cuda")
        totals = torch.empty(8, dtype=torch.int64, device="cuda")
        hits = torch.empty(5000, dtype=torch.int64, device="cuda")
        out = torch.empty(n + 4096, dtype=torch.uint8, device="cuda")
        ooff = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
        flags = torch.empty(nd, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(8, dtype=torch.int64, device="cuda")
    kd = int(np.searchsorted(offs, 1 << 20, side="right")) - 1
    cases, sets = {}, {}
    for name, (entries, groups) in lists.items():
        ws = sets[name] = tok.word_set(entries, groups)
        want = capi.word_matches_host(entries, groups, capi.TD_WL_FOLD_ASCII, x[:int(offs[kd])], offs[:kd + 1])
        for label, fl in ((name, 0), (name + " global", capi.TD_WL_NO_LDS)):
            if fl and name != "400 entries":
                continue
            fn = (lambda ws=ws, fl=fl: tok.word_matches_device(ws, dt.data_ptr(), n, do.data_ptr(), nd, fl, stats.data_ptr(), totals.data_ptr(),
                                                               hits.data_ptr(), s))
            fn()  # sanity, before anything is timed: the first MiB's documents against the host statement
            tok.device_status(s)
            side.synchronize()
            assert np.array_equal(stats.view(-1)[:kd * 4].cpu().numpy().reshape(kd, 4), want[0]), (label, "stats")
            res["sets"][label] = dict(ws.info, totals=totals[:4].cpu().tolist())
            cases[label] = fn
    rules = capi.MaskRules.make(capi.TD_MA_EMAILS | capi.TD_MA_IPS | capi.TD_MA_KEEP_PRIVATE_IPS, (b"email@example.com",), (b"22.214.171.124",))
    cases["utf8_check"] = lambda: tok.utf8_check(dt.data_ptr(), n, do.data_ptr(), nd, flags.data_ptr(), 0, counts.data_ptr(), s)
    cases["mask clean"] = lambda: tok.mask_addresses_device(dt.data_ptr(), n, do.data_ptr(), nd, rules, out.data_ptr(), n + 4096, ooff.data_ptr(),
                                                            stats.data_ptr(), totals.data_ptr(), counts.data_ptr(), s)
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
        for ref in ("utf8_check", "mask clean"):
            u = float(np.mean(ms[ref]))
            res[f"ratios_to_{ref.replace(' ', '_')}"] = {k: round(float(np.mean(v)) / u, 3) for k, v in ms.items()}
        res["resident_over_global_400"] = round(float(np.mean(ms["400 entries"])) / float(np.mean(ms["400 entries global"])), 3)
        res["turns_spread_ms"] = {k: round(abs(v[0] - v[1]), 4) for k, v in ms.items()}
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
