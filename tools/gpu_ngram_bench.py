"""Cost of the n-gram matches: 1 GiB of English encoded once with td_encode_device and kept resident, then
td_ngram_matches_device on those ids with three sets:
  hits_100k     100 000 13-grams drawn from the corpus itself: hits exist
  nohits_1m     1 000 000 13-grams of English text of another seed: practically no hits
  lengths_3     lengths 8, 13 and 50 together, 100 000 of each from the other text
each with cover only and with cover, labels and doc_stats, beside two yardsticks in the same process on the same ids:
td_span_labels_device (the closest existing kernel: ids in, a per-id stream out, a halo in LDS) and the dense device-to-device
copy of the ids.  The cases alternate `repeats` times; each time a case's figure is the median over `steps` windows after `warmup`
calls, a window being as many back-to-back calls between two HIP events as fill about `window_ms`, divided by their number; the
report gives the median of those and their smallest and largest.  Before anything is timed the hits case is held against
td_ngram_matches_host on the corpus' first 200 000 ids.

usage: gpu_ngram_bench.py [--size-mb 1024] [--steps 10] [--warmup 3] [--repeats 3] [--window-ms 20] [--json OUT] [--only CASE]
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
import td_corpus  # noqa: E402
from tokendagger_amd import capi, vocab_io  # noqa: E402


def grams(ids, k, count, rng):
    """`count` k-grams of ids at random starts -> (flat int32, offsets)."""
    starts = rng.integers(0, len(ids) - k, size=count)
    flat = ids[starts[:, None] + np.arange(k)[None, :]].astype(np.int32).reshape(-1)
    return flat, np.arange(count + 1, dtype=np.int64) * k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mb", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--json", default="")
    ap.add_argument("--only", default="", help="time only the cases whose name contains this (a profiler run on one case)")
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
    real = dk[:ntok]
    head = real[:4 << 20].cpu().numpy()  # the patterns of the hits case come from the corpus' first ids
    other_text, other_offs = td_corpus.english(64 << 20, seed=977)
    other, _ = tok.encode_batch(other_text, other_offs)
    rng = np.random.default_rng(5)
    l8, l13, l50 = (grams(other, k, 100000, rng) for k in (8, 13, 50))
    sets = {
        "hits_100k": tok.ngram_set(*grams(head, 13, 100000, rng)),
        "nohits_1m": tok.ngram_set(*grams(other, 13, 1000000, rng)),
        "lengths_3": tok.ngram_set(np.concatenate([l8[0], l13[0], l50[0]]),
                                   np.concatenate([l8[1], l8[1][-1] + l13[1][1:], l8[1][-1] + l13[1][-1] + l50[1][1:]])),
    }
    cover = torch.empty(ntok, dtype=torch.uint8, device="cuda")
    labels = real.clone()
    stats = torch.zeros(2 * nd, dtype=torch.int64, device="cuda")
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    spec = capi.ngram_spec(-100)

    def match(nset, full):
        return lambda: tok.ngram_matches_device(nset, real.data_ptr(), ntok, dto.data_ptr(), nd, spec, cover.data_ptr(),
                                                labels.data_ptr() if full else 0, stats.data_ptr() if full else 0, 0, counts.data_ptr(), s)

    # sanity, before anything is timed: the hits case against the host statement on the first 200 000 ids
    k_docs = int(np.searchsorted(dto.cpu().numpy(), 200000, side="right")) - 1
    sub_offs = dto[:k_docs + 1].cpu().numpy()
    sub = head[:int(sub_offs[-1])]
    hp, ho = grams(head, 13, 100000, np.random.default_rng(5))  # (not the set's list: any list does for the comparison)
    with tok.ngram_set(hp, ho) as chk:
        got = tok.ngram_matches(chk, sub, sub_offs, labels=sub)
        want = capi.ngram_matches_host(hp, sub, sub_offs, offsets=ho, labels=sub, pattern_counts=False)
        for g, w in zip(got, want):
            assert (g is None and w is None) or np.array_equal(g, w)
        assert want[4][0] > 0
    found = {}
    for name, nset in sets.items():
        match(nset, True)()
        tok.device_status(s)
        found[name] = counts.tolist()
        labels.copy_(real)

    lab_out = torch.empty_like(real)
    lab_counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    lspec = capi.labels_spec([head[100:102].tolist()], [int(head[200])], -100, True)
    out = torch.empty(ntok, dtype=torch.int32, device="cuda")
    cases = {"dense_copy": lambda: out.copy_(real),
             "span_labels": lambda: tok.span_labels_device(real.data_ptr(), ntok, dto.data_ptr(), nd, lspec, lab_out.data_ptr(), 0, 0,
                                                           lab_counts.data_ptr(), s)}
    for name, nset in sets.items():
        cases[name + "_cover"] = match(nset, False)
        cases[name + "_cover_labels_stats"] = match(nset, True)

    if args.only:
        cases = {k: v for k, v in cases.items() if args.only in k}
    inner = {}

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

    medians = {k: [] for k in cases}
    for _ in range(args.repeats):
        for k, fn in cases.items():
            medians[k].append(timed(k, fn))
    res = {"corpus": "english", "size_mb": args.size_mb, "docs": nd, "ids": ntok, "steps": args.steps, "repeats": args.repeats,
           "window_ms": args.window_ms, "sets": {k: v.info for k, v in sets.items()}, "found": found, "cases": []}
    for k, ms in medians.items():
        med = float(np.median(ms))
        res["cases"].append({"case": k, "calls_per_window": inner[k], "median_ms": round(med, 4), "min_ms": round(min(ms), 4),
                             "max_ms": round(max(ms), 4), "medians_ms": [round(m, 4) for m in ms],
                             "ids_per_us": round(ntok / med / 1e3, 2)})
    by = {r["case"]: r["median_ms"] for r in res["cases"]}
    if "span_labels" in by and "dense_copy" in by:
        res["ratios"] = {k: {"to_span_labels": round(v / by["span_labels"], 3), "to_dense_copy": round(v / by["dense_copy"], 3)}
                         for k, v in by.items() if k not in ("span_labels", "dense_copy")}
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")
    for v in sets.values():
        v.close()


if __name__ == "__main__":
    main()
