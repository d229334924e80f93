"""Cost of per-token starts: td_encode_device alone, then td_encode_device_with_starts in bytes and in chars, and
td_token_starts_device alone on the same ids; device-event times over `steps` calls after `warmup`.  The bytes each starts pass
must move are counted here from the shapes; the share of the 8 TB/s peak is those bytes over the starts pass's own time
(with starts minus without).

usage: gpu_offsets_bench.py [--corpus english] [--size-mb 1024] [--pattern llama4|generic:autogen] [--steps 10] [--warmup 3] [--json OUT]
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

PEAK = 8.0e12
AUTOGEN = r"[a-zA-Z]+|\s+|[0-9]+|[^\w\s]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", default="english")
    ap.add_argument("--size-mb", type=int, default=1024)
    ap.add_argument("--pattern", default="llama4", choices=["llama4", "generic:autogen"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    _, pat, ranks, special = vocab_io.load_tdv(vocab_io.default_vocab_path())
    if args.pattern == "generic:autogen":
        pat = AUTOGEN
    tok = capi.HipTokenizer(pat, ranks, special, device=0)
    n = args.size_mb << 20
    x, offs = bench.build_corpus(args.corpus, n, 1000)
    nd = len(offs) - 1
    dt = torch.from_numpy(x).cuda()
    do = torch.from_numpy(offs).cuda()
    cap = n
    dk = torch.empty(cap, dtype=torch.int32, device="cuda")
    dto = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
    dst = torch.empty(cap, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    tok.reserve(n, nd)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        tok.device_status(s)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        tok.device_status(s)
        return e0.elapsed_time(e1) / args.steps

    enc = timed(lambda: tok.encode_device(dt.data_ptr(), n, do.data_ptr(), nd, dk.data_ptr(), cap, dto.data_ptr(), s))
    ntok = int(dto[nd].item())
    res = {"corpus": args.corpus, "size_mb": args.size_mb, "pattern": args.pattern, "docs": nd, "ids": ntok, "encode_ms": enc}
    for unit, name in ((capi.TD_UNIT_BYTES, "bytes"), (capi.TD_UNIT_CHARS, "chars")):
        ms = timed(lambda: tok.encode_device_with_starts(dt.data_ptr(), n, do.data_ptr(), nd, dk.data_ptr(), cap, dto.data_ptr(),
                                                         dst.data_ptr(), unit, s))
        res[f"encode_starts_{name}_ms"] = ms
        res[f"starts_{name}_ms"] = ms - enc
        st = timed(lambda: tok.token_starts_device(dk.data_ptr(), ntok, dto.data_ptr(), nd, dst.data_ptr(), unit, s))
        res[f"token_starts_{name}_ms"] = st
        # bytes of the covered pass: ids read twice (two scan passes), a head bit per id written and read twice, starts written,
        # the per-id length (bytes: two words of the offsets table) or character table lookups (cached; not counted)
        moved = 4 * ntok * 2 + 8 * ntok + ntok / 8 * 3 + 16 * (nd + 1)
        if name == "chars":
            moved += 16 * ntok  # (the packed pair read and the start written back by td_off_finish)
        if args.pattern.startswith("generic"):
            moved += n / 8 * 3 + n / 16 + 16 * ntok + 4 * ntok  # (the two bitmaps read, the covered bitmap and its prefixes, the finish pass)
            if name == "chars":
                moved += n + n / 8 + n / 16
        res[f"bytes_moved_{name}"] = moved
        res[f"token_starts_{name}_peak_share"] = moved / (st * 1e-3) / PEAK
        res[f"starts_{name}_peak_share"] = moved / (max(ms - enc, 1e-6) * 1e-3) / PEAK
    line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()})
    print(line, flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
