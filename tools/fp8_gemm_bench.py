"""Stream rate of the FP8-weight skinny GEMMs against their 16-bit forms: the five GEMMs of a 7B
retrieval verify (q|k|v + RoPE, o + residual, gate|up + SwiGLU, down + residual, lm_head with fp32 logits) at 7 and 17 rows,
each timed over enough weight copies that every launch streams from HBM (> the 256 MB Infinity Cache), one JSON line per
(GEMM, rows, form) with microseconds per launch and the achieved TB/s of the weight bytes.  Run it under
``rocprofv3 --kernel-trace --stats -- python tools/fp8_gemm_bench.py`` for the per-kernel view.

    python tools/fp8_gemm_bench.py [--iters 20] [--rows 7,17]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from triforce_amd import ops  # noqa: E402

DEV = "cuda:0"
HID, INTER, VOCAB, H, D = 4096, 11008, 32000, 32, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", default="7,17")
    a = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(0)

    def w(n, k):
        return (torch.randn(n, k, generator=g, device=DEV) * 0.02).half()

    shapes = {"qkv_rope": (3 * HID, HID, 1, (H, D)), "o_proj": (HID, HID, 1, None), "gate_up": (2 * INTER, HID, 2, None),
              "down_proj": (HID, INTER, 1, None), "lm_head": (VOCAB, HID, 1, None)}
    ln = torch.ones(HID, dtype=torch.float16, device=DEV)
    cos = torch.ones(8192, D, dtype=torch.float16, device=DEV)
    sin = torch.zeros(8192, D, dtype=torch.float16, device=DEV)
    kc = torch.zeros(H, 64, D, dtype=torch.float16, device=DEV)
    vc = torch.zeros(H, 64, D, dtype=torch.float16, device=DEV)
    for name, (N, K, split, rope) in shapes.items():
        copies = max(2, int(1.2e9 // (N * K * 2)) + 1)             # > 1 GB of fp16 weights per round: no cache reuse
        pls = [ops.PackedLinear(w(N, K), split=split, rope=rope) for _ in range(copies)]
        f8s = [ops.Fp8Linear(p) for p in pls]
        for M in [int(r) for r in a.rows.split(",")]:
            x = (torch.randn(M, K, generator=g, device=DEV)).half()
            xa = ops.Act.from_rows(x) if ops.act_packed(M) else x
            pos = torch.arange(M, device=DEV)
            res = ops.Act.from_rows(torch.zeros(M, N, dtype=torch.float16, device=DEV)) if ops.act_packed(M) else \
                torch.zeros(M, N, dtype=torch.float16, device=DEV)
            ss = ops.ss_buffer(N, DEV)

            def run(wt):
                if name == "qkv_rope":
                    ops.qkv_rope(xa, wt, ln, 1e-5, cos, sin, pos, kc, vc, 0, H, D)
                elif name == "gate_up":
                    ops.mlp_act(xa, wt, ln=ln, eps=1e-5)
                elif name == "lm_head":
                    ops.linear(xa, wt, out_f32=True, ln=ln, eps=1e-5)
                else:
                    ops.linear(xa, wt, resid=res, out=res, ss_out=ss)
            for form, ws in (("fp16", pls), ("fp8", f8s)):
                for wt in ws:                                      # warm-up
                    run(wt)
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.iters):
                    for wt in ws:
                        run(wt)
                t1.record()
                torch.cuda.synchronize()
                us = t0.elapsed_time(t1) * 1e3 / (a.iters * len(ws))
                nbytes = N * K * (2 if form == "fp16" else 1) + (0 if form == "fp16" else 4 * N)
                print(json.dumps(dict(gemm=name, rows=M, form=form, N=N, K=K, us=round(us, 2), weight_MB=round(nbytes / 1e6, 1),
                                      TBps=round(nbytes / us / 1e6, 3))), flush=True)
        del pls, f8s
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
