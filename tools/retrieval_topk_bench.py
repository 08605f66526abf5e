"""What the retrieval top-k costs above 32 768 chunks: HIP events around batches of launches after a warm-up,
the forms of one shape alternated in one process, the median over --batches batches, per launch.  One JSON line per shape,
appended to --out.
  tf_retrieval_topk_large at H in {4, 32}, sets = 512, C in {32 768, 126 250 (1 010 000 tokens / 8), 1 048 576}, N(0, 1) scores;
  beside it tf_retrieval_topk at C = 32 768 (the kernel routing keeps there) and tf_retrieval_score at the same C (chunk 8,
  D = 128: what a build pays next to the top-k; not at H = 32, C = 1 048 576, whose K alone is 68 GB).
    python tools/retrieval_topk_bench.py [--out profiles/retrieval_topk_large.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
DEV = "cuda:0"


def _batch_us(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / n


def _alternate(forms, batches, per_batch):
    for fn in forms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(batches):
        for k, fn in forms.items():
            times[k].append(_batch_us(fn, per_batch))
    return {k: (round(statistics.median(v), 2), round(min(v), 2)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--per-batch", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from triforce_amd import ops
    sets, chunk, D = 512, 8, 128
    for H in (4, 32):
        for C in (32768, 126250, 1048576):
            gen = torch.Generator().manual_seed(C % 1000 + H)
            scores = torch.randn(H, C, generator=gen).half().to(DEV)
            forms = {"tf_retrieval_topk_large": lambda: ops.retrieval_topk_large(scores, sets)}
            if C <= 32768:
                forms["tf_retrieval_topk"] = lambda: ops.retrieval_topk(scores, sets)
                assert torch.equal(ops.retrieval_topk(scores, sets), ops.retrieval_topk_large(scores, sets))
            k = None
            if H * C * chunk * D * 2 <= 16 << 30:
                k = torch.empty(H, C * chunk, D, dtype=torch.float16, device=DEV).normal_()
                q = torch.randn(H, D, generator=gen).half().to(DEV)
                forms["tf_retrieval_score"] = lambda: ops.retrieval_score(k, q, C, chunk)
            res = _alternate(forms, a.batches, a.per_batch)
            line = {"what": "retrieval top-k, one layer", "H": H, "C": C, "sets": sets, "batches": a.batches,
                    "launches_per_batch": a.per_batch, "median_us": {n: v[0] for n, v in res.items()},
                    "min_us": {n: v[1] for n, v in res.items()}}
            if k is None:
                line["tf_retrieval_score"] = "not measured (K of this shape is 68 GB)"
            print(json.dumps(line), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
            del k, forms
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
