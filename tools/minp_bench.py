"""What min-p costs on the device, on the protocol of tools/large_vocab_bench.py: HIP events, warm-up first,
the forms of every comparison alternated in one process, medians of --launches (>= 50).  One JSON line per measurement, appended
to --out.
  Rows 7 and 8 x 32 000 (tf_minp_probs) and 1 and 8 x 128 256 (tf_minp_probs_large), sharp rows (one model-like peak) and
  N(0, 2.5) rows, min_p in {0.05, 0.3} at top_p in {1.0, 0.9}, temperature 1, against
    the same rows through tf_topp_probs / tf_topp_probs_large (one workgroup per row: what min-p is added to), and
    the torch fallback of utils.sampling.norm_logits (filter, softmax, mask, renormalise: the route min-p would take on the host).
  Expectation: the kernel without min-p plus at most one pass over the row.
    python tools/minp_bench.py [--out profiles/minp_probs.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
DEV = "cuda:0"


def _emit(line, out):
    print(json.dumps(line), flush=True)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "a") as f:
            f.write(json.dumps(line) + "\n")


def _event_us(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3


def _alternate(forms, launches):
    for fn in forms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(launches):
        for k, fn in forms.items():
            times[k].append(_event_us(fn))
    return {k: (round(statistics.median(v), 2), round(min(v), 2)) for k, v in times.items()}


def _rows(kind, rows, V, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind == "sharp":                                    # what a language model emits: a few tokens carry the mass
        lg = torch.randn(rows, V, generator=gen)
        for r in range(rows):
            lg[r, torch.randperm(V, generator=gen)[:6]] += torch.tensor([14.0, 13.0, 12.0, 11.0, 10.0, 9.0])
        return lg
    return torch.randn(rows, V, generator=gen) * 2.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.launches >= 50
    from triforce_amd import ops
    from triforce_amd.utils import sampling as S

    def torch_route(lg, T, P, m):
        probs = torch.softmax(S.top_k_top_p_filter(lg / T, top_k=-1, top_p=P), dim=-1)
        probs = probs.masked_fill(probs < m * probs.amax(dim=-1, keepdim=True), 0.0)
        return probs / probs.sum(dim=-1, keepdim=True)
    ops.TOPP_MULTI = False                                 # one workgroup per row: the form min-p is added to
    T = 1.0
    for rows, V in ((7, 32000), (8, 32000), (1, 128256), (8, 128256)):
        small = V <= ops.TOPP_MAX_VOCAB
        for kind in ("sharp", "sigma2.5"):
            lg = _rows(kind, rows, V, 10 * rows + V % 7).to(DEV)
            for P in (1.0, 0.9):
                forms = {"without_min_p": (lambda: ops.topp_probs(lg, T, P)) if small else (lambda: ops.topp_probs_large(lg, T, P))}
                kept = {}
                for m in (0.05, 0.3):
                    fn = ops.minp_probs if small else ops.minp_probs_large
                    forms[f"min_p_{m}"] = lambda m=m, fn=fn: fn(lg, T, -1, P, m)
                    forms[f"torch_fallback_min_p_{m}"] = lambda m=m: torch_route(lg, T, P, m)
                    kept[f"min_p_{m}"] = [int(x) for x in (fn(lg, T, -1, P, m) > 0).sum(-1).tolist()]
                res = _alternate(forms, a.launches)
                _emit({"what": "temperature + top-p + min-p + softmax", "kernel": "tf_minp_probs" if small else "tf_minp_probs_large",
                       "rows": rows, "V": V, "row_kind": kind, "T": T, "top_p": P, "launches": a.launches, "kept_per_row": kept,
                       "median_us": {k: v[0] for k, v in res.items()}, "min_us": {k: v[1] for k, v in res.items()}}, a.out)


if __name__ == "__main__":
    main()
