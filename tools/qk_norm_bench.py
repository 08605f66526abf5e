"""What QK norm costs a decoder layer, at the Qwen3-8B q|k|v shape (K 4096, N 6144: 32 query / 8 KV heads
of 128).  A norm-free model of that shape takes ONE launch for [RMSNorm ->] q|k|v GEMM -> RoPE -> KV append
(tf_skinny_qkv_rope_gqa_act); a QK-norm model takes the norm GEMM to row-major rows (tf_skinny_gemm_act) and then
tf_qk_norm_rope_append.  Protocol of tools/attn_bias_bench.py: every launch streams its weights from HBM (the weight copies
of one round exceed the 256 MB Infinity Cache), after a warm-up the two forms ALTERNATE batch by batch, each batch between HIP
events; reported: the median microseconds per layer step of either form, their difference, and the fused form's own
run-to-run spread (its batches' (max - min) / median) — the yardstick for that difference.  The new kernel alone is timed
at 7 / 17 / 4096 rows.  One JSON line per measurement.

    python tools/qk_norm_bench.py [--batches 15] [--out profiles/qk_norm_gemm.jsonl]
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
HID, H, HKV, D, LAYERS = 4096, 32, 8, 128, 36
N = (H + 2 * HKV) * D
EPS = 1e-6


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(reps):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(0)
    lines = []
    copies = max(2, int(0.6e9 // (N * HID * 2)) + 1)
    ws = [(torch.randn(N, HID, generator=g, device=DEV) * 0.02).half() for _ in range(copies)]
    fused = [ops.PackedLinear(w, rope=(H, HKV, D)) for w in ws]
    plain = [ops.PackedLinear(w) for w in ws]
    ln = torch.ones(HID, dtype=torch.float16, device=DEV)
    qn = (1 + 0.1 * torch.randn(D, generator=g, device=DEV)).half()
    kn = (1 + 0.1 * torch.randn(D, generator=g, device=DEV)).half()
    cos = torch.ones(4096, D, dtype=torch.float16, device=DEV)
    sin = torch.zeros(4096, D, dtype=torch.float16, device=DEV)
    kc = torch.zeros(HKV, 4096, D, dtype=torch.float16, device=DEV)
    vc = torch.zeros(HKV, 4096, D, dtype=torch.float16, device=DEV)
    for rows in (7, 17):
        x = torch.randn(rows, HID, generator=g, device=DEV).half()
        pos = torch.arange(rows, device=DEV)
        buf = torch.empty(rows, N, dtype=torch.float16, device=DEV)

        def run_fused(i):
            ops.qkv_rope(x, fused[i], ln, EPS, cos, sin, pos, kc, vc, 0, H, D, Hkv=HKV)

        def run_split(i):
            ops.linear(x, plain[i], ln=ln, eps=EPS, out=buf)
            ops.qk_norm_rope_append(buf, qn, kn, EPS, cos, sin, pos, kc, vc, 0, H, D, Hkv=HKV)

        for _ in range(2):                                          # warm-up of both forms
            timed(run_fused, copies), timed(run_split, copies)
        t_f, t_s = [], []
        for _ in range(a.batches):                                  # the forms alternate
            t_f.append(timed(run_fused, copies))
            t_s.append(timed(run_split, copies))
        mf, ms = statistics.median(t_f), statistics.median(t_s)
        line = dict(what="qkv layer step", shape="qwen3-8B", rows=rows, N=N, K=HID, copies=copies, batches=a.batches,
                    us_fused_norm_free=round(mf, 2), us_gemm_plus_qk_norm=round(ms, 2), extra_us_per_layer=round(ms - mf, 2),
                    extra_us_per_forward=round((ms - mf) * LAYERS, 1), ratio=round(ms / mf, 4),
                    spread_fused=round((max(t_f) - min(t_f)) / mf, 4), spread_split=round((max(t_s) - min(t_s)) / ms, 4))
        lines.append(line)
        print(json.dumps(line), flush=True)
    for rows in (7, 17, 4096):                                      # the new kernel alone (its input stays cache-resident)
        buf = torch.randn(rows, N, generator=g, device=DEV).half()
        pos = torch.arange(rows, device=DEV)
        reps = 200 if rows <= 32 else 20

        def run_kernel(i):
            ops.qk_norm_rope_append(buf, qn, kn, EPS, cos, sin, pos, kc, vc, 0, H, D, Hkv=HKV)

        timed(run_kernel, reps)
        ts = [timed(run_kernel, reps) for _ in range(a.batches)]
        m = statistics.median(ts)
        line = dict(what="tf_qk_norm_rope_append alone", shape="qwen3-8B", rows=rows, H=H, Hkv=HKV, D=D, reps=reps,
                    batches=a.batches, us=round(m, 2), spread=round((max(ts) - min(ts)) / m, 4),
                    bytes_moved=rows * (2 * N) * 2)
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
