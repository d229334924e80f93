"""Cost of the UTF-8 validation and repair, on resident text, in GB/s of input:
  english      --size-mb (1024) of the bench's English: td_utf8_check_device beside td_nfc_check_device on the same buffer, a read-only
               pass and a dense copy (what tools/gpu_copy_ceiling.py measures), td_utf8_device on the clean text and on the text with one
               byte in every 4 KiB overwritten by 0x80 (every tile takes the lane-by-lane path)
  mixed, code, chat   --other-mb (256) of bench.py's corpora: the check beside td_encode_device of the same text in the same run (the check
               must cost less than the encode it stands in front of), and the repair of `mixed` corrupted the same way
Before anything is timed the device results are held against td_utf8_host on the first MiB.  A case's figure is the median over `steps`
windows after `warmup` calls, a window being as many back-to-back calls between two HIP events as fill about `window_ms`.

usage: gpu_utf8_bench.py [--size-mb 1024] [--other-mb 256] [--steps 7] [--warmup 2] [--window-ms 20] [--json OUT] [--only CASE]
Kernel times and counters: run this tool under rocprofv3 (--kernel-trace --stats, or --pmc ... alone), in a run of its own.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mb", type=int, default=1024)
    ap.add_argument("--other-mb", type=int, default=256)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--json", default="")
    ap.add_argument("--only", default="", help="time only the cases whose name contains this (a profiler run on one case)")
    args = ap.parse_args()
    _, pat, ranks, special = vocab_io.load_tdv(vocab_io.default_vocab_path())
    tok = capi.HipTokenizer(pat, ranks, special, device=0)
    side = torch.cuda.Stream()  # (the device forms do not take the null stream)
    s = side.cuda_stream
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

    for name in ("english", "mixed", "code", "chat"):
        x, offs = bench.build_corpus(name, (args.size_mb if name == "english" else args.other_mb) << 20, 1000)
        n, nd = len(x), len(offs) - 1
        bad = x.copy()
        bad[2048::4096] = 0x80
        with torch.cuda.stream(side):
            dt, db = torch.from_numpy(x).cuda(), torch.from_numpy(bad).cuda()
            do = torch.from_numpy(offs).cuda()
            cap = n + (n >> 9) + 4096  # (a stray byte in every 4 KiB grows the text by two bytes there, and by up to six where it cuts a character)
            out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            ooff = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
            flags = torch.empty(max(nd, 1), dtype=torch.uint8, device="cuda")
            first = torch.empty(max(nd, 1), dtype=torch.int64, device="cuda")
            nbad = torch.empty(max(nd, 1), dtype=torch.int64, device="cuda")
            counts = torch.zeros(8, dtype=torch.int64, device="cuda")
            ids = torch.empty(n, dtype=torch.int32, device="cuda")
            toff = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
        check = lambda t=dt: tok.utf8_check(t.data_ptr(), n, do.data_ptr(), nd, flags.data_ptr(), first.data_ptr(), counts.data_ptr(), s)  # noqa: E731
        repair = lambda t=dt: tok.utf8_device(t.data_ptr(), n, do.data_ptr(), nd, capi.TD_UTF8_REPLACE, out.data_ptr(), cap, ooff.data_ptr(),  # noqa: E731
                                              flags.data_ptr(), first.data_ptr(), nbad.data_ptr(), counts.data_ptr(), s)
        nfc_check = lambda: tok.nfc_check(dt.data_ptr(), n, do.data_ptr(), nd, flags.data_ptr(), counts.data_ptr(), s)  # noqa: E731
        encode = lambda: tok.encode_device(dt.data_ptr(), n, do.data_ptr(), nd, ids.data_ptr(), n, toff.data_ptr(), stream=s)  # noqa: E731
        # sanity, before anything is timed: the first MiB's documents of the corrupted text against the host statement
        kd = int(np.searchsorted(offs, 1 << 20, side="right")) - 1
        want = capi.utf8_host(bad[:int(offs[kd])], offs[:kd + 1])
        check(db)
        tok.device_status(s)
        side.synchronize()
        assert np.array_equal(flags[:kd].cpu().numpy(), want[2]) and np.array_equal(first[:kd].cpu().numpy(), want[3]), (name, "the check")
        repair(db)
        tok.device_status(s)
        side.synchronize()
        assert np.array_equal(ooff[:kd + 1].cpu().numpy(), want[1]) and bytes(out[:int(want[1][-1])].cpu().numpy()) == bytes(want[0]), (name, "text")
        assert np.array_equal(nbad[:kd].cpu().numpy(), want[4]), (name, "n_bad")
        corrupted_counts = counts.cpu().tolist()
        check()
        tok.device_status(s)
        side.synchronize()
        res["corpora"][name] = {"bytes": n, "docs": nd, "documents_ill_formed": int(counts.cpu()[1]), "corrupted_counts": corrupted_counts}
        cases = {"utf8_check": check, "encode_device": encode}
        if name == "english":
            cases.update({"read_only_pass": lambda: dt[:n - n % 8].view(torch.int64).sum(), "dense_copy": lambda: out[:n].copy_(dt),
                          "nfc_check": nfc_check, "utf8_check (again)": check, "nfc_check (again)": nfc_check, "utf8_repair clean": repair})
        if name in ("english", "mixed"):
            cases.update({"utf8_check corrupted": lambda: check(db), "utf8_repair corrupted": lambda: repair(db)})
        for k, fn in cases.items():
            if args.only and args.only not in f"{name}/{k}":
                continue
            med, lo, hi, inner = timed(fn)
            res["cases"].append({"corpus": name, "case": k, "calls_per_window": inner, "median_ms": round(med, 4), "min_ms": round(lo, 4),
                                 "max_ms": round(hi, 4), "input_gb_per_s": round(n / med / 1e6, 1)})
        del dt, db, do, out, ooff, flags, first, nbad, ids, toff
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
