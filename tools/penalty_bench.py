"""What the target tier's penalties cost.  HIP events, warm-up first, the forms of every comparison
alternated in one process, medians.  One JSON line per measurement, appended to --out.
  (a) kernel : tf_penalize_logits alone at 7 and 8 x 32 000 and 1 and 8 x 128 256 (contiguous rows: the 16-byte path; a row
               stride of V + 1: the scalar path; out == logits), and tf_penalty_commit of 7 ids: microseconds, and the bytes
               the kernel moves (rows * V * 8 + V * 5) over the time.
  (b) decode : TriForceRunner steps of the default bench shape (124 928 tokens, aligned weights) on ONE engine, its graphs
               captured without penalties, then with (1.1, 0, 0), then without again: ms per step and acceptance of each
               phase.  (Acceptance on the aligned synthetic weights says little about trained models: the drafts are aligned
               with the UNPENALISED target by construction.)
    python tools/penalty_bench.py --parts a,b [--out profiles/penalties.jsonl]"""
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


def kernel_part(a):
    from triforce_amd import ops
    from triforce_amd.utils.sampling import Penalties
    pen = Penalties(1.1, 0.2, 0.1)
    for rows, V in ((7, 32000), (8, 32000), (1, 128256), (8, 128256)):
        gen = torch.Generator().manual_seed(rows + V)
        x = (torch.randn(rows, V, generator=gen) * 3.0).to(DEV)
        wide = torch.empty(rows, V + 1, device=DEV)[:, :V]
        wide.copy_(x)
        st = ops.PenaltyState(V, DEV)
        st.reset(torch.randint(0, V, (1, 4096), generator=gen))
        ops.penalty_commit(st, torch.randint(0, V, (64,), generator=gen).to(DEV), 64)
        ids = torch.randint(0, V, (rows,), generator=gen).to(DEV)
        out, out_wide, inplace = torch.empty_like(x), torch.empty(rows, V + 1, device=DEV)[:, :V], x.clone()
        commit_ids = torch.randint(0, V, (7,), generator=gen).to(DEV)
        forms = {"vector_path": lambda: ops.penalize_logits(x, ids, st, pen, out=out),
                 "scalar_path_stride_V+1": lambda: ops.penalize_logits(wide, ids, st, pen, out=out_wide),
                 "out_is_logits": lambda: ops.penalize_logits(inplace, ids, st, pen, out=inplace),
                 "row_copy_for_scale": lambda: out.copy_(x),
                 "penalty_commit_7_ids": lambda: ops.penalty_commit(st, commit_ids, 7)}
        res = _alternate(forms, a.launches)
        moved = rows * V * 8 + V * 5
        _emit({"what": "tf_penalize_logits / tf_penalty_commit alone", "part": "a", "rows": rows, "V": V, "launches": a.launches,
               "bytes_moved": moved, "median_us": {k: v[0] for k, v in res.items()}, "min_us": {k: v[1] for k, v in res.items()},
               "vector_path_GB_per_s": round(moved / res["vector_path"][0] / 1e3, 1)}, a.out)


def decode_part(a):
    import bench
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.sampling import UniformSource
    args = bench.parse(["--gpus", "1", "--steps", "1", "--warmup", "1", "--prefill", str(a.prefill), "--gen_cap", "2048"])
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    kind, tspec, dspec, wlabel = bench.resolve_weights(args)
    target, draft = bench.load_models(args, device, kind, tspec, dspec)
    ge = bench.build_engine(args, device, target, draft)
    tcfg, _ = bench.target_config(args.target)
    input_ids = torch.randint(3, tcfg.vocab_size, (1, args.prefill), generator=torch.Generator().manual_seed(args.seed)).to(device)
    phases = []
    for name, rep in (("plain", 1.0), ("repetition_1.1", 1.1), ("plain_again", 1.0)):
        if phases:                                             # the same engine, its graphs captured again with / without
            ge.initialize_cuda_graph(args.gamma, probs=True, temperature=args.temp, top_p=args.top_p, verbose=False,
                                     repetition_penalty=rep)
        run = TriForceRunner(bench._Tok(), ge, args.gamma, top_p=args.top_p, temperature=args.temp,
                             rng=UniformSource(device, seed=args.seed), repetition_penalty=rep)
        bench.do_prefill(run, ge, input_ids, "real")
        for _ in range(8):
            run.step()
        on_device = run._device_sets() is not None
        ms = []
        for _ in range(a.blocks):
            torch.cuda.synchronize()
            ms.append(_event_us(lambda: [run.step() for _ in range(a.block_steps)]) / 1e3 / a.block_steps)
        st = run.stats(1.0)
        phases.append({"phase": name, "repetition_penalty": rep, "step_set_up_on_device": on_device,
                       "ms_per_step": [round(x, 3) for x in ms], "median_ms": round(statistics.median(ms), 3),
                       "acceptance_rate": round(st["acceptance_rate"], 4), "tokens_per_step": round(st["n"] / len(st["counts"]), 3),
                       "distinct_tokens": len(set(st["tokens"])), "tokens": st["n"]})
    _emit({"what": "TriForceRunner steps, BASELINE configs[1] engine, " + wlabel, "part": "b", "blocks": a.blocks,
           "block_steps": a.block_steps, "phases": phases}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--prefill", type=int, default=124928)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parts = set(a.parts.split(","))
    assert parts <= {"a", "b"} and a.launches >= 30
    if "a" in parts:
        kernel_part(a)
    if "b" in parts:
        decode_part(a)


if __name__ == "__main__":
    main()
