"""Cost of the NFC normalisation: td_nfc_check_device alone and the full td_nfc_device call on resident text, in GB/s
of input, on
  english      --size-mb (1024) of the bench's English: every window is proven by its bytes alone
  mixed        --mixed-mb (256) of the mixed-script corpus as it is (NFC): most windows hold lead bytes >= 0xCC and are decoded
  mixed_nfd    the NFD of the same corpus (made here by unicodedata): every accent is a segment to rewrite, every tile shrinks
each beside what tools/gpu_copy_ceiling.py measures on the same box in the same run: a read-only pass (a sum over the text as int64) and
a dense device-to-device copy of the text.  Also td_encode_batch_nfc against td_encode_batch, host to host, on the English: the
difference is the price of the proof.  Before anything is timed the device results are held against td_nfc_host on the first MiB.
A case's figure is the median over `steps` windows after `warmup` calls, a window being as many back-to-back calls between two HIP events
as fill about `window_ms`, divided by their number.

usage: gpu_nfc_bench.py [--size-mb 1024] [--mixed-mb 256] [--steps 7] [--warmup 2] [--window-ms 20] [--json OUT] [--only CASE] [--no-e2e]
Kernel times and counters: run this tool under rocprofv3 (--kernel-trace --stats, or --pmc ... alone), in a run of its own.
"""
import argparse
import json
import os
import sys
import time
import unicodedata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from tokendagger_amd import capi, vocab_io  # noqa: E402


def nfd_corpus(x, offs):
    """The NFD of a corpus whose documents are lines."""
    raw = unicodedata.normalize("NFD", x.tobytes().decode("utf-8")).encode("utf-8")
    text = np.frombuffer(raw, dtype=np.uint8).copy()
    nl = np.nonzero(text == 10)[0] + 1
    return text, np.unique(np.concatenate([[0], nl[nl < len(text)], [len(text)]])).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mb", type=int, default=1024)
    ap.add_argument("--mixed-mb", type=int, default=256)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--json", default="")
    ap.add_argument("--only", default="", help="time only the cases whose name contains this (a profiler run on one case)")
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    _, pat, ranks, special = vocab_io.load_tdv(vocab_io.default_vocab_path())
    tok = capi.HipTokenizer(pat, ranks, special, device=0)
    side = torch.cuda.Stream()  # (the device forms do not take the null stream)
    s = side.cuda_stream
    corpora = {"english": bench.build_corpus("english", args.size_mb << 20, 1000)}
    unit, uo = bench.build_corpus("mixed", min(args.mixed_mb, 32) << 20, 1000)
    reps = max(args.mixed_mb // 32, 1)

    def tiled(u, o):
        return np.tile(u, reps), np.unique(np.concatenate([o + r * len(u) for r in range(reps)])).astype(np.int64)

    corpora["mixed"] = tiled(unit, uo)
    corpora["mixed_nfd"] = tiled(*nfd_corpus(unit, uo))
    res = {"unicode_version": capi.nfc_info(capi.TD_NFC_INFO_UNICODE_VERSION), "table_bytes": capi.nfc_info(capi.TD_NFC_INFO_TABLE_BYTES),
           "steps": args.steps, "window_ms": args.window_ms, "corpora": {}, "cases": []}

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

    for name, (x, offs) in corpora.items():
        n, nd = len(x), len(offs) - 1
        with torch.cuda.stream(side):
            dt = torch.from_numpy(x).cuda()
            do = torch.from_numpy(offs).cuda()
            cap = n + (n >> 3) + 64  # (NFC of these corpora does not grow them)
            out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            ooff = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
            flags = torch.empty(max(nd, 1), dtype=torch.uint8, device="cuda")
            changed = torch.empty(max(nd, 1), dtype=torch.uint8, device="cuda")
            counts = torch.zeros(8, dtype=torch.int64, device="cuda")
        check = lambda: tok.nfc_check(dt.data_ptr(), n, do.data_ptr(), nd, flags.data_ptr(), counts.data_ptr(), s)  # noqa: E731
        full = lambda: tok.nfc_device(dt.data_ptr(), n, do.data_ptr(), nd, out.data_ptr(), cap, ooff.data_ptr(), changed.data_ptr(),  # noqa: E731
                                      counts.data_ptr(), s)
        # sanity, before anything is timed: the first MiB's documents against the host statement
        kd = int(np.searchsorted(offs, 1 << 20, side="right")) - 1
        want = capi.nfc_host(x[:int(offs[kd])], offs[:kd + 1])
        check()
        tok.device_status(s)
        side.synchronize()
        assert np.array_equal(flags[:kd].cpu().numpy(), want[2]), (name, "flags")
        n_flagged = int(counts.cpu()[1])
        full()
        tok.device_status(s)
        side.synchronize()
        assert np.array_equal(ooff[:kd + 1].cpu().numpy(), want[1]) and bytes(out[:int(want[1][-1])].cpu().numpy()) == bytes(want[0]), (name, "text")
        res["corpora"][name] = {"bytes": n, "docs": nd, "documents_not_proven": n_flagged, "counts": counts.cpu().tolist()}
        cases = {"read_only_pass": lambda: dt[:n - n % 8].view(torch.int64).sum(), "dense_copy": lambda: out[:n].copy_(dt),
                 "nfc_check": check, "nfc_normalise": full}
        for k, fn in cases.items():
            if args.only and args.only not in f"{name}/{k}":
                continue
            med, lo, hi, inner = timed(fn)
            res["cases"].append({"corpus": name, "case": k, "calls_per_window": inner, "median_ms": round(med, 4), "min_ms": round(lo, 4),
                                 "max_ms": round(hi, 4), "input_gb_per_s": round(n / med / 1e6, 1)})
        if name == "english" and not args.no_e2e and not args.only:
            for k, fn in (("td_encode_batch", lambda: tok.encode_batch(x, offs)), ("td_encode_batch_nfc", lambda: tok.encode_batch_nfc(x, offs))):
                fn()
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                res["cases"].append({"corpus": name, "case": k + " (host to host)", "median_ms": round(float(np.median(ts)), 2),
                                     "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2), "input_gb_per_s": round(n / float(np.median(ts)) / 1e6, 2)})
        del dt, do, out, ooff, flags, changed
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
