"""Eager HIP-event timing of the retrieval-verify attention: fp16 rows (tf_attn_decode_act) against FP8 codes followed by the
fp16 spec rows in one launch (tf_attn_decode_fp8_tail_act, TRIFORCE_RETRIEVAL_KV=fp8) at the three shapes of
the retrieval tier: 7 rows x 4 103 keys x 32 heads (configs[1]), 17 x 12 305 x 32 (configs[3]) and 17 x 12 305 x 16 (a TP-2
shard).  L2 flushed before every launch, median of --iters.  TB/s on each form's own bytes (K + V rows; for FP8 the codes, the
exponent bytes and the fp16 spec rows).  ``fp8_all_codes_us``: tf_attn_decode_fp8_act over as many keys, all of them codes.
One JSON line per shape on stdout.

    python tools/retrieval_kv_bench.py [--iters 50] [--out profiles/retrieval_kv_fp8_attn.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from triforce_amd import ops  # noqa: E402

SHAPES = ((7, 4096, 32), (17, 12288, 32), (17, 12288, 16))          # (spec rows = gamma + 1, budget, heads)


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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, D = "cuda:0", 128
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    rows = []
    for sq, B, H in SHAPES:
        sk = B + sq
        k = (torch.randn(H, sk, D, device=dev) * 0.3).half()
        v = torch.randn(H, sk, D, device=dev).half()
        kc = torch.empty(H, B, D, dtype=torch.float8_e4m3fn, device=dev)
        vc = torch.empty_like(kc)
        ke = torch.empty(H, B, dtype=torch.uint8, device=dev)
        ve = torch.empty_like(ke)
        ops.kv_quant_rows(k[:, :B], v[:, :B], kc, vc, ke, ve, 0, deq=True)     # k, v rows [0, B) now hold deq: same inputs
        tk, tv = k[:, B:].contiguous(), v[:, B:].contiguous()
        # the all-codes kernel of the FP8 full cache over as many keys (the spec rows quantized too): what the FP8 stream costs
        # at this length without the second source
        ac = [torch.empty(H, sk, D, dtype=torch.float8_e4m3fn, device=dev) for _ in range(2)]
        ae = [torch.empty(H, sk, dtype=torch.uint8, device=dev) for _ in range(2)]
        ops.kv_quant_rows(k, v, *ac, *ae, 0)
        q = torch.randn(sq, H, D, device=dev).half()
        packed = sq >= 17
        a = ops.attn_decode(q, k, v, sk, 0.088, packed=packed)
        b = ops.attn_decode_fp8_tail(q, kc, vc, ke, ve, tk, tv, B, 0.088, packed=packed)
        same = torch.equal(a.t, b.t) if packed else torch.equal(a, b)
        t16 = timed(lambda: ops.attn_decode(q, k, v, sk, 0.088, packed=packed), args.iters, flush)
        t8 = timed(lambda: ops.attn_decode_fp8_tail(q, kc, vc, ke, ve, tk, tv, B, 0.088, packed=packed), args.iters, flush)
        tall = timed(lambda: ops.attn_decode_fp8(q, *ac, *ae, sk, 0.088, packed=packed), args.iters, flush)
        b16, b8 = 2 * H * sk * D * 2, 2 * H * (B * (D + 1) + sq * D * 2)
        r = {"H": H, "sq": sq, "sk_codes": B, "sk": sk, "nsplit": ops._pick_nsplit(H, sk), "bit_identical": same,
             "fp16_us": round(t16, 1), "fp8_us": round(t8, 1), "fp8_all_codes_us": round(tall, 1), "fp8_over_fp16": round(t8 / t16, 3),
             "fp16_TBps": round(b16 / t16 / 1e6, 2), "fp8_TBps": round(b8 / t8 / 1e6, 2), "fp16_bytes": b16, "fp8_bytes": b8,
             "iters": args.iters}
        print(json.dumps(r), flush=True)
        rows.append(r)
        del k, v, kc, vc, ke, ve, ac, ae
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
