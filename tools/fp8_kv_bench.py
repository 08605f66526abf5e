"""Eager HIP-event timing of the target-verify attention over the full KV cache: fp16 (tf_attn_decode_act) against FP8
(tf_attn_decode_fp8_act, TRIFORCE_KV_CACHE=fp8) at 124 935 keys, 32 heads (7B) and 40 heads (13B), 1 / 7 / 17 query rows.
TB/s on each form's own bytes (K + V rows, plus the exponent bytes for FP8).  One JSON line per shape on stdout.

    python tools/fp8_kv_bench.py [--iters 50] [--out profiles/...jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from triforce_amd import ops  # noqa: E402


def timed(fn, iters, flush):
    ts = []
    for _ in range(iters):
        flush.zero_()                                    # evict: every launch streams the cache from HBM
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sk", type=int, default=124935)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, D, sk = "cuda:0", 128, args.sk
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    rows = []
    for H in (32, 40):
        k = (torch.randn(H, sk, D, device=dev) * 0.3).half()
        v = torch.randn(H, sk, D, device=dev).half()
        kc = torch.empty(H, sk, D, dtype=torch.float8_e4m3fn, device=dev)
        vc = torch.empty_like(kc)
        ke = torch.empty(H, sk, dtype=torch.uint8, device=dev)
        ve = torch.empty_like(ke)
        ops.kv_quant_rows(k, v, kc, vc, ke, ve, 0, deq=True)     # k, v now hold deq: same inputs for both forms
        for sq in (1, 7, 17):
            q = torch.randn(sq, H, D, device=dev).half()
            t16 = timed(lambda: ops.attn_decode(q, k, v, sk, 0.088, packed=sq >= 17), args.iters, flush)
            t8 = timed(lambda: ops.attn_decode_fp8(q, kc, vc, ke, ve, sk, 0.088, packed=sq >= 17), args.iters, flush)
            b16, b8 = 2 * H * sk * D * 2, 2 * H * sk * (D + 1)
            r = {"H": H, "sq": sq, "sk": sk, "nsplit": ops._pick_nsplit(H, sk), "fp16_us": round(t16, 1),
                 "fp8_us": round(t8, 1), "fp8_over_fp16": round(t8 / t16, 3), "fp16_TBps": round(b16 / t16 / 1e6, 2),
                 "fp8_TBps": round(b8 / t8 / 1e6, 2), "fp16_bytes": b16, "fp8_bytes": b8}
            print(json.dumps(r), flush=True)
            rows.append(r)
        del k, v, kc, vc, ke, ve
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
