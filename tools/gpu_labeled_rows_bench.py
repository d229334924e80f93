"""Label rows: the pair call (td_*_rows_labeled_device: ids and labels by one placement) against the two single calls it replaces
(the existing device entry point once on the ids and once on the labels), device-resident, per layout and seq_len.

Then the fused entry, host to host, on td_corpus.chat: Tokenizer.encode_batch_to_labeled_rows against the calls it replaces,
encode_batch_to_labels followed by the layout's ids_to_*_rows on the ids and again on the labels (no BOS / EOS: the only framing the
two-call form can do).

usage: tools/gpu_labeled_rows_bench.py [--mib 1024] [--out profiles/labeled_rows_cost.json] [--bench-parent F --bench-this F]

Device time by HIP events around the calls on one stream; the three forms of a case alternate, one call each a round, and the median
of --reps rounds after a warm-up round is reported; for BESTFIT (which synchronises to plan on the host) the wall time matters too.
The fused comparison is wall time, --fused-reps alternating rounds after a warm-up round.  The ids are the encode of td_corpus.english, the label stream is
random int32: what the kernels move does not depend on the values."""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--fused-reps", type=int, default=3)
    ap.add_argument("--bench-parent", default="", help="bench.py lines of the parent build, same GPU job")
    ap.add_argument("--bench-this", default="", help="bench.py lines of this build, same GPU job")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import td_corpus
    from tokendagger_amd import capi, vocab_io
    name, pat, ranks, special = vocab_io.load_tdv(vocab_io.default_vocab_path())
    tok = capi.HipTokenizer(pat, ranks, special, device=0)
    dev = torch.device("cuda", 0)
    text, offs = td_corpus.english(a.mib << 20, seed=3)
    ids, toffs = tok.encode_batch(text, offs)
    n, n_docs = len(ids), len(toffs) - 1
    d_ids = torch.from_numpy(ids).to(dev)
    d_src = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32, device=dev)
    d_offs = torch.from_numpy(toffs).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {"bytes": int(len(text)), "ids": n, "docs": n_docs, "reps": a.reps, "library": os.environ.get("TD_HIP_LIB", "this build"), "cases": []}

    def timed(fns, reps, events=True):
        """fns: {name: call}; alternating, one call of each a round, the first round not counted."""
        dts, walls = {k: [] for k in fns}, {k: [] for k in fns}
        for rep in range(reps + 1):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    walls[k].append((time.perf_counter() - t0) * 1e3)
                    dts[k].append(e0.elapsed_time(e1))
        out = {}
        for k in fns:
            out[k] = {"wall_ms": round(statistics.median(walls[k]), 4), "wall_ms_min": round(min(walls[k]), 4), "wall_ms_max": round(max(walls[k]), 4)}
            if events:
                out[k].update(device_ms=round(statistics.median(dts[k]), 4), device_ms_min=round(min(dts[k]), 4), device_ms_max=round(max(dts[k]), 4))
        return out

    for S in (2048, 8192):
        for layout in ("concat", "pad", "bestfit", "windows"):
            b, e, pad = 5, 7, 3
            if layout == "concat":
                spec, rows = capi.rows_spec(S, capi.TD_ROWS_CONCAT, b, e, pad), capi.rows_capacity_of(capi.rows_spec(S, 0, b, e, pad), n, n_docs)
            elif layout == "pad":
                spec, rows = capi.rows_spec(S, capi.TD_ROWS_PAD, b, e, pad), n_docs
            elif layout == "bestfit":
                spec = capi.pack_spec(S, b, e, pad)
                rows = int(capi.pack_plan(toffs, spec)[0])
            else:
                spec = capi.windows_spec(S, b, e, pad)
                rows = int(capi.window_plan(toffs, spec, 64)[0])
            slots = rows * S
            out1 = torch.empty(slots, dtype=torch.int32, device=dev)
            out2 = torch.empty(slots, dtype=torch.int32, device=dev)
            counts = torch.zeros(4, dtype=torch.int64, device=dev)

            def single(src, out):
                if layout in ("concat", "pad"):
                    tok.make_rows_device(src.data_ptr(), n, d_offs.data_ptr(), n_docs, spec, out.data_ptr(), rows, 0, 0, counts.data_ptr(), stream)
                elif layout == "bestfit":
                    tok.pack_rows_device(src.data_ptr(), n, d_offs.data_ptr(), n_docs, spec, out.data_ptr(), rows, stream=stream)
                else:
                    tok.window_rows_device(src.data_ptr(), n, d_offs.data_ptr(), n_docs, spec, 64, out.data_ptr(), rows, d_counts=counts.data_ptr(),
                                           stream=stream)

            def pair():
                lab = capi.rows_labels(d_src.data_ptr(), out2.data_ptr(), -100, e, -100)
                if layout in ("concat", "pad"):
                    tok.make_rows_labeled_device(d_ids.data_ptr(), n, d_offs.data_ptr(), n_docs, spec, out1.data_ptr(), rows, lab,
                                                 d_counts=counts.data_ptr(), stream=stream)
                elif layout == "bestfit":
                    tok.pack_rows_labeled_device(d_ids.data_ptr(), n, d_offs.data_ptr(), n_docs, spec, out1.data_ptr(), rows, lab, stream=stream)
                else:
                    tok.window_rows_labeled_device(d_ids.data_ptr(), n, d_offs.data_ptr(), n_docs, spec, 64, out1.data_ptr(), rows, lab,
                                                   d_counts=counts.data_ptr(), stream=stream)

            case = {"layout": layout, "seq_len": S, "rows": rows,
                    **timed({"one_call": lambda: single(d_ids, out1), "two_calls": lambda: (single(d_ids, out1), single(d_src, out2)),
                             "pair": pair}, a.reps)}
            case["pair_over_two_calls_device"] = round(case["pair"]["device_ms"] / case["two_calls"]["device_ms"], 4)
            case["pair_over_two_calls_wall"] = round(case["pair"]["wall_ms"] / case["two_calls"]["wall_ms"], 4)
            assert tok.device_status_pos(stream)[0] == 0
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            del out1, out2
    del d_ids, d_src, d_offs, ids, text
    torch.cuda.empty_cache()

    # ---- the fused entry, host to host, on chat text ----
    from tokendagger_amd import wrapper
    wtok = wrapper.llama4_scout(0)
    ctext, coffs = td_corpus.chat(a.mib << 20, seed=5)
    OPEN, CLOSE = ["<|header_start|>assistant<|header_end|>"], ["<|eot|>", "<|eom|>"]
    res["fused"] = {"corpus": f"td_corpus.chat {a.mib} MiB, every special allowed", "bytes": int(len(ctext)), "docs": int(len(coffs) - 1),
                    "reps": a.fused_reps, "cases": []}
    for S in (2048, 8192):
        for layout in ("concat", "pad", "bestfit", "windows"):
            kw = dict(overlap=64) if layout == "windows" else {}

            def fused():
                return wtok.encode_batch_to_labeled_rows(ctext, coffs, S, layout=layout, open=OPEN, close=CLOSE, pad=3, **kw)

            def parts():
                lab = wtok.encode_batch_to_labels(ctext, coffs, open=OPEN, close=CLOSE)
                if layout in ("concat", "pad"):
                    f = lambda x, p: wtok.ids_to_rows(x, lab.tok_offsets, S, layout=layout, pad=p)
                elif layout == "bestfit":
                    f = lambda x, p: wtok.ids_to_packed_rows(x, lab.tok_offsets, S, pad=p)
                else:
                    f = lambda x, p: wtok.ids_to_window_rows(x, lab.tok_offsets, S, overlap=64, pad=p)
                return f(lab.ids, 3), f(lab.labels, -100)

            case = {"layout": layout, "seq_len": S, **timed({"parts": parts, "fused": fused}, a.fused_reps, events=False)}
            r, (pi, pl) = fused(), parts()
            assert np.array_equal(r.rows.ids, pi.ids) and np.array_equal(r.labels, pl.ids), (layout, S)  # (the same rows either way)
            case["rows"] = int(r.rows.counts[0])
            case["fused_over_parts_wall"] = round(case["fused"]["wall_ms"] / case["parts"]["wall_ms"], 4)
            res["fused"]["cases"].append(case)
            print(json.dumps(case), flush=True)
            del r, pi, pl
    for key, path in (("parent", a.bench_parent), ("this", a.bench_this)):
        if path:
            runs = [json.loads(ln) for ln in Path(path).read_text().splitlines() if ln.startswith("{")]
            res.setdefault("default_bench_line_same_job", {})[key] = {"gb_per_s": [r.get("value") for r in runs],
                                                                      "ms_per_step": [r.get("ms_per_step") for r in runs]}
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        cases, fcases = res.pop("cases"), res["fused"].pop("cases")  # (a case a line)
        lines = lambda cs: "[\n" + ",\n".join("  " + json.dumps(c) for c in cs) + "\n ]"
        res["fused"]["cases"], res["cases"] = "@F", "@C"
        Path(a.out).write_text(json.dumps(res, indent=1).replace('"@F"', lines(fcases)).replace('"@C"', lines(cases)) + "\n")


if __name__ == "__main__":
    main()
