"""What the attention bias costs the decode GEMMs that carry it: the fused q|k|v + RoPE + KV-append GEMM
and the o_proj + residual GEMM at 7 rows, with and without a bias, at the 7B shape (K 4096, q|k|v N 12 288) and at the
Qwen2.5-7B shape (K 3584, q|k|v N 4608: 28 query / 4 KV heads of 128).  Every launch streams its weights from HBM (the weight
copies of one round exceed the 256 MB Infinity Cache).  After a warm-up the two forms ALTERNATE batch by batch, each batch
between HIP events; reported: the median microseconds per launch of either form, their ratio, and the bias-free form's own
run-to-run spread (its batches' (max - min) / median) — the yardstick for that ratio.  The bias adds N * 2 bytes to
N * K * 2.  One JSON line per (GEMM, shape).

    python tools/attn_bias_bench.py [--batches 15] [--out profiles/attn_bias_gemm.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from triforce_amd import ops  # noqa: E402

DEV = "cuda:0"
ROWS = 7
SHAPES = {"llama-7B": dict(hidden=4096, H=32, Hkv=32, D=128), "qwen2.5-7B": dict(hidden=3584, H=28, Hkv=4, D=128)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(0)
    lines = []
    for shape, s in SHAPES.items():
        hid, H, Hkv, D = s["hidden"], s["H"], s["Hkv"], s["D"]
        for gemm, N, K in (("qkv_rope", (H + 2 * Hkv) * D, hid), ("o_proj", hid, H * D)):
            copies = max(2, int(0.6e9 // (N * K * 2)) + 1)
            rope = (H, Hkv, D) if gemm == "qkv_rope" else None
            ws = [(torch.randn(N, K, generator=g, device=DEV) * 0.02).half() for _ in range(copies)]
            free = [ops.PackedLinear(w, rope=rope) for w in ws]
            with_b = [ops.PackedLinear(w, rope=rope, bias=(torch.randn(N, generator=g, device=DEV) * 0.5).half()) for w in ws]
            x = torch.randn(ROWS, K, generator=g, device=DEV).half()
            ln = torch.ones(K, dtype=torch.float16, device=DEV)
            cos = torch.ones(64, D, dtype=torch.float16, device=DEV)
            sin = torch.zeros(64, D, dtype=torch.float16, device=DEV)
            pos = torch.arange(ROWS, device=DEV)
            kc = torch.zeros(Hkv, 64, D, dtype=torch.float16, device=DEV)
            vc = torch.zeros(Hkv, 64, D, dtype=torch.float16, device=DEV)
            res = torch.zeros(ROWS, N, dtype=torch.float16, device=DEV)
            ss = ops.ss_buffer(N, DEV)

            def run(pl):
                if gemm == "qkv_rope":
                    kw = {} if pl.bias is None else {"bias": pl.bias_rope}
                    ops.qkv_rope(x, pl, ln, 1e-6, cos, sin, pos, kc, vc, 0, H, D, Hkv=Hkv, **kw)
                else:
                    kw = {} if pl.bias is None else {"bias": pl.bias}
                    ops.linear(x, pl, resid=res, out=res, ss_out=ss, **kw)

            def batch(pls):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for pl in pls:
                    run(pl)
                t1.record()
                torch.cuda.synchronize()
                return t0.elapsed_time(t1) * 1e3 / len(pls)

            for _ in range(2):                                      # warm-up of both forms
                batch(free), batch(with_b)
            t_free, t_bias = [], []
            for _ in range(a.batches):                              # the forms alternate
                t_free.append(batch(free))
                t_bias.append(batch(with_b))
            mf, mb = statistics.median(t_free), statistics.median(t_bias)
            line = dict(gemm=gemm, shape=shape, rows=ROWS, N=N, K=K, copies=copies, batches=a.batches,
                        us_bias_free=round(mf, 2), us_bias=round(mb, 2), ratio=round(mb / mf, 4),
                        spread_bias_free=round((max(t_free) - min(t_free)) / mf, 4),
                        spread_bias=round((max(t_bias) - min(t_bias)) / mb, 4),
                        extra_bytes_ratio=round(1.0 / K, 6))
            lines.append(line)
            print(json.dumps(line), flush=True)
            del free, with_b, ws
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
