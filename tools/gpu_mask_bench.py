"""Cost of the address mask, on resident text: --size-mb (1024) of the bench's English corpus
  mask clean             td_mask_addresses_device on the corpus as it is, which has no address: the anchor-free path
  mask every 4 KiB       the same text with an e-mail address and a public IPv4 address planted every 4 KiB
  mask every 256 B       the same, planted every 256 bytes: every tile is decided, scanned and written lane by lane
  mask mixed             the bench's mixed corpus as it is
beside, on the same buffers in the same process,
  utf8_device            td_utf8_device, policy replace: the yardstick, it reads the text twice and copies it once with no byte walk
  line_filter identity   td_line_filter_device with the empty rule set
Before anything is timed the device results are held against td_mask_addresses_host on the first MiB of every text.  A case's figure is
the median over `steps` windows after `warmup` calls, a window being as many back-to-back calls between two HIP events as fill about
`window_ms`; the minimum and the maximum are reported beside it.  The cases are timed in turn, twice over, so that a drift shows as a pair
that differs.

usage: gpu_mask_bench.py [--size-mb 1024] [--steps 7] [--warmup 2] [--window-ms 200] [--json OUT] [--only CASE]
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

PLANT = b" jane.roe+list@mail.example.org and 93.184.216.34 "
IPS = (b"22.214.171.124", b"126.96.36.199", b"188.8.131.52", b"184.108.40.206", b"220.127.116.11", b"18.104.22.168")


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
    rules = capi.MaskRules.make(capi.TD_MA_EMAILS | capi.TD_MA_IPS | capi.TD_MA_KEEP_PRIVATE_IPS, (b"email@example.com",), IPS)
    res = {"steps": args.steps, "window_ms": args.window_ms, "texts": {}, "cases": []}

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
    xm, offs_m = bench.build_corpus("mixed", args.size_mb << 20, 1000)
    texts = {"clean": (x, offs), "every 4 KiB": (x.copy(), offs), "every 256 B": (x.copy(), offs), "mixed": (xm, offs_m)}
    for name, step in (("every 4 KiB", 4096), ("every 256 B", 256)):
        at = np.arange(100, len(x) - len(PLANT), step, dtype=np.int64)
        texts[name][0][at[:, None] + np.arange(len(PLANT))] = np.frombuffer(PLANT, dtype=np.uint8)
    cap = max(len(t) for t, _ in texts.values()) + 4096  # (every literal here is shorter than what it replaces)
    nd_max = max(len(o) for _, o in texts.values())
    with torch.cuda.stream(side):
        out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        ooff = torch.empty(nd_max, dtype=torch.int64, device="cuda")
        stats = torch.empty((nd_max, 8), dtype=torch.int64, device="cuda")
        totals = torch.empty(8, dtype=torch.int64, device="cuda")
        counts = torch.zeros(8, dtype=torch.int64, device="cuda")
    cases, keep = {}, []
    for name, (t, o) in texts.items():
        n, nd = len(t), len(o) - 1
        with torch.cuda.stream(side):
            dt, do = torch.from_numpy(t).cuda(), torch.from_numpy(o).cuda()
        keep += [dt, do]
        fn = (lambda dt=dt, do=do, n=n, nd=nd: tok.mask_addresses_device(dt.data_ptr(), n, do.data_ptr(), nd, rules, out.data_ptr(), cap, ooff.data_ptr(),
                                                                          stats.data_ptr(), totals.data_ptr(), counts.data_ptr(), s))
        # sanity, before anything is timed: the first MiB's documents against the host statement
        kd = int(np.searchsorted(o, 1 << 20, side="right")) - 1
        want = capi.mask_addresses_host(t[:int(o[kd])], o[:kd + 1], rules)
        fn()
        tok.device_status(s)
        side.synchronize()
        assert np.array_equal(ooff[:kd + 1].cpu().numpy(), want[1]) and bytes(out[:int(want[1][-1])].cpu().numpy()) == bytes(want[0]), name
        assert np.array_equal(stats.view(-1)[:kd * 6].cpu().numpy().reshape(kd, 6), want[2]), (name, "stats")
        res["texts"][name] = {"bytes": n, "docs": nd, "out_bytes": int(counts.cpu()[0]), "totals": totals[:6].cpu().tolist()}
        cases[f"mask {name}"] = fn
        if name == "clean":
            cases["utf8_device"] = lambda dt=dt, do=do, n=n, nd=nd: tok.utf8_device(dt.data_ptr(), n, do.data_ptr(), nd, capi.TD_UTF8_REPLACE, out.data_ptr(),
                                                                                    cap, ooff.data_ptr(), 0, 0, 0, counts.data_ptr(), s)
            cases["line_filter identity"] = lambda dt=dt, do=do, n=n, nd=nd: tok.line_filter_device(dt.data_ptr(), n, do.data_ptr(), nd, capi.LineRules.make(),
                                                                                                    out.data_ptr(), cap, ooff.data_ptr(), stats.data_ptr(),
                                                                                                    totals.data_ptr(), counts.data_ptr(), s)
    for turn in (1, 2):
        for k, fn in cases.items():
            if args.only and not any(o in k for o in args.only.split(",")):
                continue
            med, lo, hi, inner = timed(fn)
            res["cases"].append({"case": k, "turn": turn, "calls_per_window": inner, "median_ms": round(med, 4), "min_ms": round(lo, 4),
                                 "max_ms": round(hi, 4)})
    ms = {k: [c["median_ms"] for c in res["cases"] if c["case"] == k] for k in cases}
    if all(len(v) == 2 for v in ms.values()):
        u = float(np.mean(ms["utf8_device"]))
        res["ratios_to_utf8_device"] = {k: round(float(np.mean(v)) / u, 3) for k, v in ms.items()}
        res["turns_spread"] = {k: round(abs(v[0] - v[1]) / u, 3) for k, v in ms.items()}
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
