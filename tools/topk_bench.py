"""Temperature + top-k + top-p + softmax (tf_topk_topp_probs) against tf_topp_probs (one workgroup per row, no top-k) on the same
rows, and against the sort-based torch route norm_logits(top_k=k) took before the kernel existed.  HIP events, median of 50
samples; a kernel sample is one replay of a hipGraph of 20 calls, a torch-route sample is one eager call (torch.topk's
multi-block form is not replayed from a graph).  One JSON line per (rows, kind, k).
    python tools/topk_bench.py [--out profiles/topk_probs_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from triforce_amd import ops  # noqa: E402
from triforce_amd.utils import sampling  # noqa: E402

DEV = "cuda:0"
T, P = 0.6, 0.9


def rows_of(rows, V, kind):
    g = torch.Generator().manual_seed(7 + rows)
    lg = torch.randn(rows, V, generator=g) * 2.5
    lg = {"sigma2.5": lg, "sharp": (lg * 4).half().float()}[kind]
    return lg.to(DEV)


def samples_us(fn, calls, samples=50):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(samples):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / calls * 1e3)
    return round(statistics.median(out), 2), round(min(out), 2)


def graphed(fn, calls=20):
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    return g.replay, calls


def torch_route(lg, k):
    x = lg / T
    return torch.softmax(sampling.top_k_top_p_filter(x, top_k=k, top_p=P), dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ops.TOPP_MULTI = False                                    # tf_topp_probs itself: one workgroup per row
    V, lines = 32000, []
    with torch.inference_mode():
        for kind in ("sharp", "sigma2.5"):
            for rows in (7, 8):
                lg = rows_of(rows, V, kind)
                replay, calls = graphed(lambda: ops.topp_probs(lg, T, P))
                base = samples_us(replay, calls)
                for k in (20, 50, 1000):
                    replay, calls = graphed(lambda: ops.topk_topp_probs(lg, T, k, P))
                    new = samples_us(replay, calls)
                    old = samples_us(lambda: torch_route(lg, k), 1)
                    line = {"what": "temperature + top-k + top-p + softmax, V = 32000, T 0.6 / top_p 0.9; median (min) of 50 HIP-event samples",
                            "rows": rows, "kind": kind, "top_k": k,
                            "topk_topp_us": new[0], "topk_topp_min_us": new[1],
                            "topp_one_workgroup_per_row_us": base[0], "topp_min_us": base[1],
                            "torch_sort_route_eager_us": old[0], "torch_sort_route_min_us": old[1],
                            "ratio_to_topp": round(new[0] / base[0], 3),
                            "kept_in_row_0": int((ops.topk_topp_probs(lg, T, k, P)[0] > 0).sum())}
                    lines.append(line)
                    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
