"""What top-N alternatives and ranks cost beside the per-token log-probability.  HIP events, warm-up first,
the forms of every comparison alternated round by round in one process, medians over the rounds.  One JSON line per
measurement, appended to --out.
  (a) kernel: tf_token_top_logprobs_ids alone against tf_token_logprobs_ids on the same rows — rows in {1, 7}, V in {32 000,
              128 256}, N in {1, 5, 20}, on sharp rows (N(0, 4)) and on the all-equal row (every entry ties: the overflow
              path); each sample is --reps back-to-back launches between two events, microseconds per launch.
  (b) decode: TriForceRunner steps on the bench engine at --prefill tokens in alternating blocks with logprobs alone and with
              top_logprobs=5, ms per step.
    python tools/top_logprobs_bench.py --parts a,b [--out profiles/top_logprobs_bench.jsonl]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.logprobs_bench import _emit, _event_ms  # noqa: E402


def kernel_part(a):
    from triforce_amd import ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    for rows in (1, 7):
        for V in (32000, 128256):
            for kind in ("sharp", "all_equal"):
                x = torch.randn(rows, V, device=dev, generator=gen) * 4.0 if kind == "sharp" \
                    else torch.full((rows, V), 0.37, device=dev)
                ids = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(1)).tolist()
                out = torch.empty(rows, device=dev)
                bufs = {n: (torch.empty(rows, n, dtype=torch.int32, device=dev), torch.empty(rows, n, device=dev),
                            torch.empty(rows, dtype=torch.int32, device=dev)) for n in (1, 5, 20)}
                forms = {"single": lambda: ops.token_logprobs(x, ids, out=out)}
                for n, (ti, tl, rk) in bufs.items():
                    forms[f"top{n}"] = lambda n=n, ti=ti, tl=tl, rk=rk: ops.token_top_logprobs(x, ids, n, ti, tl, rk, out)
                for fn in forms.values():
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                us = {k: [] for k in forms}
                for _ in range(a.rounds):
                    for k, fn in forms.items():              # alternated
                        us[k].append(_event_ms(lambda: [fn() for _ in range(a.reps)]) * 1e3 / a.reps)
                med = {k: statistics.median(v) for k, v in us.items()}
                _emit({"what": "tf_token_top_logprobs_ids against tf_token_logprobs_ids", "part": "a", "rows": rows, "V": V,
                       "kind": kind, "rounds": a.rounds, "reps": a.reps,
                       "median_us": {k: round(v, 2) for k, v in med.items()}, "min_us": {k: round(min(v), 2) for k, v in us.items()},
                       "ratio_to_single": {k: round(v / med["single"], 2) for k, v in med.items() if k != "single"}}, a.out)


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
    run = TriForceRunner(bench._Tok(), ge, args.gamma, top_p=args.top_p, temperature=args.temp,
                         rng=UniformSource(device, seed=args.seed), top_logprobs=5)
    bench.do_prefill(run, ge, input_ids, "real")
    for _ in range(8):
        run.step()
    ms = {0: [], 5: []}
    for _ in range(a.blocks):
        for top in (0, 5):                                   # alternated blocks of one runner: same engine, same stream
            run.top_logprobs, run._lp_n = top, 0            # (the buffers start over: a block without top-N fills none)
            torch.cuda.synchronize()
            ms[top].append(_event_ms(lambda: [run.step() for _ in range(a.block_steps)]) / a.block_steps)
    _emit({"what": "TriForceRunner steps, bench engine, " + wlabel, "part": "b", "prefill": a.prefill, "blocks": a.blocks,
           "block_steps": a.block_steps, "vocab": tcfg.vocab_size,
           "ms_per_step_logprobs": [round(x, 3) for x in ms[0]], "ms_per_step_top5": [round(x, 3) for x in ms[5]],
           "median_logprobs_ms": round(statistics.median(ms[0]), 3), "median_top5_ms": round(statistics.median(ms[5]), 3)}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--prefill", type=int, default=32768)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parts = set(a.parts.split(","))
    assert parts <= {"a", "b"}
    if "a" in parts:
        kernel_part(a)
    if "b" in parts:
        decode_part(a)


if __name__ == "__main__":
    main()
