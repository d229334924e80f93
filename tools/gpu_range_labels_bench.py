"""td_range_labels_device on chat ids, beside a dense device-to-device copy of the same ids and td_span_labels_device on them,
measured in the same process.

The corpus is td_corpus.chat (--mb MiB, default 1024), encoded with every special token allowed; the ranges are the assistant
contents (from behind <|header_start|>assistant<|header_end|> to the end of the next <|eot|> / <|eom|>), found on the host by
searching the literals in the bytes, so the range labels must equal the span labels: the tool checks that before it times
anything.  Timed with device events, one call each, alternating, --reps times after --warmup rounds:
  copy                 torch's copy_ of the ids (4 B read + 4 B written an id)
  span_labels          td_span_labels_device, labels only (the sibling)
  range_labels         td_range_labels_device, the covered form, labels only: the starts are scanned and never stored
  starts_then_ranges   td_token_starts_device (8 B an id written) then the explicit-starts form (8 B an id read): what fusing buys
  range_labels_all     the covered form with mask and trained_offsets
Reported: medians with min and max, the bytes the algorithm needs per case, the ratios to the copy and to span_labels.  Prints one
JSON line and writes it to --out when given.
usage: python tools/gpu_range_labels_bench.py [--mb 1024] [--out profiles/range_labels_cost.json]"""
import argparse
import json
import re
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

OPENER = b"<|header_start|>assistant<|header_end|>"
CLOSERS = [b"<|eot|>", b"<|eom|>"]


def chat_ranges(text, doffs):
    """(range_offsets, ranges[n, 2]) of the assistant contents, closer included; document-relative bytes."""
    data = bytes(text)
    pat = re.compile(b"|".join(re.escape(x) for x in [OPENER] + CLOSERS))
    ro, out = [0], []
    for d in range(len(doffs) - 1):
        lo, hi = int(doffs[d]), int(doffs[d + 1])
        begin = None
        for m in pat.finditer(data, lo, hi):
            if m.group() == OPENER:
                if begin is None:
                    begin = m.end() - lo
            elif begin is not None:
                out.append((begin, m.end() - lo))
                begin = None
        if begin is not None:
            out.append((begin, hi - lo))
        ro.append(len(out))
    return np.asarray(ro, dtype=np.int64), np.asarray(out, dtype=np.int64).reshape(-1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
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
    ro, rg = chat_ranges(text, doffs)
    del text
    opener = tok.encode_with_special_strs(OPENER, specials)[0].tolist()
    lspec = capi.labels_spec([opener], [special["<|eot|>"], special["<|eom|>"]], -100, True)
    rspec = capi.range_spec("overlap", -100)
    dev = torch.device("cuda", 0)
    n, n_docs, n_ranges = len(ids), len(offs) - 1, len(rg)
    d_ids, d_offs = torch.from_numpy(ids).to(dev), torch.from_numpy(offs).to(dev)
    d_ro, d_rg = torch.from_numpy(ro).to(dev), torch.from_numpy(rg).to(dev)
    d_lab = {k: torch.empty_like(d_ids) for k in ("span", "range", "two", "all")}
    d_copy = torch.empty_like(d_ids)
    d_starts = torch.empty(n, dtype=torch.int64, device=dev)
    d_mask = torch.empty(n, dtype=torch.uint8, device=dev)
    d_toff = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    d_counts = {k: torch.zeros(4, dtype=torch.int64, device=dev) for k in d_lab}
    stream = torch.cuda.current_stream(dev).cuda_stream

    def ranges(key, starts=0, mask=0, toff=0):
        tok.range_labels_device(d_ids.data_ptr(), n, d_offs.data_ptr(), n_docs, d_ro.data_ptr(), d_rg.data_ptr(), n_ranges, rspec,
                                d_lab[key].data_ptr(), mask, toff, d_counts[key].data_ptr(), starts, stream)

    def two_steps():
        tok.token_starts_device(d_ids.data_ptr(), n, d_offs.data_ptr(), n_docs, d_starts.data_ptr(), capi.TD_UNIT_BYTES, stream)
        ranges("two", starts=d_starts.data_ptr())

    cases = {"copy": lambda: d_copy.copy_(d_ids),
             "span_labels": lambda: tok.span_labels_device(d_ids.data_ptr(), n, d_offs.data_ptr(), n_docs, lspec, d_lab["span"].data_ptr(), 0, 0,
                                                           d_counts["span"].data_ptr(), stream),
             "range_labels": lambda: ranges("range"),
             "starts_then_ranges": two_steps,
             "range_labels_all": lambda: ranges("all", mask=d_mask.data_ptr(), toff=d_toff.data_ptr())}
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
    c = {k: v.cpu().numpy() for k, v in d_counts.items()}
    for k in ("range", "two", "all"):  # the two device features agree, id for id
        assert torch.equal(d_lab[k], d_lab["span"]), k
        assert c[k][0] == c["span"][0] and c[k][1] == 0 and c[k][2] == int((rg[:, 1] - rg[:, 0]).sum()), (k, c[k])
    assert int(d_mask.sum(dtype=torch.int64)) == int(c["all"][0]) == int(d_toff[-1])
    med = {k: statistics.median(v) for k, v in times.items()}
    bytes_ = {"copy": 8 * n, "span_labels": 8 * n, "range_labels": 8 * n + 24 * n_ranges + 8 * (n_docs + 1),
              "starts_then_ranges": 8 * n + 16 * n + 4 * n + 24 * n_ranges + 8 * (n_docs + 1),
              "range_labels_all": 9 * n + 24 * n_ranges + 16 * (n_docs + 1)}
    res = {"tool": "tools/gpu_range_labels_bench.py", "corpus": f"td_corpus.chat {args.mb} MiB, all specials allowed", "ids": n, "docs": n_docs,
           "ranges": n_ranges, "counts": c["all"].tolist(),
           "form": "td_rng_docs, td_rng_check, td_rng_cum, td_off_scan<0> + td_off_carry (covered form), td_rng_apply, td_rng_status, "
                   "td_lab_finish; + td_lab_count_carry with trained_offsets",
           "reps": args.reps, "median_ms": {k: round(v, 4) for k, v in med.items()},
           "min_ms": {k: round(min(v), 4) for k, v in times.items()}, "max_ms": {k: round(max(v), 4) for k, v in times.items()},
           "bytes": bytes_, "tb_per_s_on_bytes": {k: round(bytes_[k] / med[k] / 1e9, 3) for k in med},
           "over_copy": {k: round(med[k] / med["copy"], 3) for k in med},
           "over_span_labels": {k: round(med[k] / med["span_labels"], 3) for k in med},
           "fused_over_two_steps": round(med["range_labels"] / med["starts_then_ranges"], 3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
