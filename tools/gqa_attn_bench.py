#!/usr/bin/env python3
"""Decode attention of a grouped-query target against its two multi-head neighbours.

At sq rows x sk keys, D = 128, four launches are timed with HIP events, alternating, after a warm-up of each:
  (i)   tf_attn_decode_act, H = Hkv heads           — the same K/V bytes as (ii), 1/g of its query rows
  (ii)  tf_attn_decode_gqa_act, H query / Hkv KV heads
  (iii) tf_attn_decode_act, H heads                 — the multi-head launch of the same query rows, g times the bytes
  (iv)  tf_attn_decode_act, Hkv heads x gs * sq rows — (i)'s bytes with (ii)'s q-tile count and no stacking: what the second
        q-tile costs by itself
One JSON line per form: median / min / max microseconds per launch over the rounds, the K/V bytes the launch must read
(2 * heads * sk * D * 2) and bytes / median time.  (ii) is also checked against (iii) on the repeated K/V (same bits).

    python tools/gqa_attn_bench.py --out profiles/gqa_decode_attention.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=7)
    ap.add_argument("--keys", type=int, default=124935)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--launches", type=int, default=40, help="launches per timed batch")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default="profiles/gqa_decode_attention.jsonl")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gqa_attn_bench needs a HIP device: a timing on anything else says nothing")
    from triforce_amd import ops
    dev, D = "cuda:0", 128
    sq, sk, H, Hkv = args.rows, args.keys, args.heads, args.kv_heads
    g = H // Hkv
    gen = torch.Generator().manual_seed(1)
    q = torch.randn(sq, H, D, generator=gen).to(torch.float16).to(dev)
    k = torch.randn(Hkv, sk, D, generator=gen).to(torch.float16).to(dev)
    v = torch.randn(Hkv, sk, D, generator=gen).to(torch.float16).to(dev)
    ke, ve = k.repeat_interleave(g, dim=0).contiguous(), v.repeat_interleave(g, dim=0).contiguous()
    q_small = q[:, ::g].contiguous()                                   # one query head per KV head
    scale = float(1 / torch.sqrt(torch.tensor(D, dtype=torch.float16)))
    gs, sub = ops.gqa_stack(g, sq)
    q_tall = torch.randn(gs * sq, Hkv, D, generator=gen).to(torch.float16).to(dev)
    forms = {
        "mha_kv_heads": (lambda: ops.attn_decode(q_small, k, v, sk, scale), Hkv, Hkv, ops._pick_nsplit(Hkv, sk)),
        "gqa": (lambda: ops.attn_decode_gqa(q, k, v, sk, scale), H, Hkv, ops._pick_nsplit(Hkv * sub, sk)),
        "mha_all_heads": (lambda: ops.attn_decode(q, ke, ve, sk, scale), H, H, ops._pick_nsplit(H, sk)),
        "mha_kv_heads_stacked_row_count": (lambda: ops.attn_decode(q_tall, k, v, sk, scale), Hkv, Hkv,
                                           ops._pick_nsplit(Hkv, sk)),
    }
    n = ops._pick_nsplit(Hkv * sub, sk)
    same = torch.equal(ops.attn_decode_gqa(q, k, v, sk, scale, nsplit=n), ops.attn_decode(q, ke, ve, sk, scale, nsplit=n))
    for fn, *_ in forms.values():                                      # warm-up: code objects, allocator, tickets
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, (fn, *_rest) in forms.items():                       # alternating: drift hits all forms alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for name, (_, heads, kv_heads, nsplit) in forms.items():
            us = statistics.median(times[name])
            kv_bytes = 2 * kv_heads * sk * D * 2
            row = dict(what="decode attention, HIP events around batches of launches (includes the launch gaps)", form=name,
                       rows=sq, keys=sk, D=D, query_heads=heads, kv_heads=kv_heads, nsplit=nsplit,
                       stacked_rows=gs * sq if name in ("gqa", "mha_kv_heads_stacked_row_count") else sq,
                       launches_per_batch=args.launches, rounds=args.rounds,
                       us_median=round(us, 2), us_min=round(min(times[name]), 2), us_max=round(max(times[name]), 2),
                       kv_bytes=kv_bytes, tb_per_s=round(kv_bytes / us * 1e-6, 3),
                       gqa_bits_equal_mha_on_repeated_kv=same, device=torch.cuda.get_device_name(0))
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
