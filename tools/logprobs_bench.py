"""What per-token log-probabilities cost.  HIP events, warm-up first, the two forms of every comparison
alternated in one process, medians.  One JSON line per measurement, appended to --out.
  (a) kernel : tf_token_logprobs alone at 8 x 32 000, 1 024 x 32 000 and 8 x 128 256 (device targets; ids as kernel
               arguments where rows <= 32): microseconds and logits bytes / time.
  (b) prefill: the target's chunked prefill of the bench configuration (124 928 tokens, aligned weights) with and without
               prompt_logprobs, seconds.
  (c) decode : TriForceRunner steps on that engine in alternating blocks with and without logprobs, ms per step.
    python tools/logprobs_bench.py --parts a,b,c [--out profiles/logprobs_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _emit(line, out):
    print(json.dumps(line), flush=True)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "a") as f:
            f.write(json.dumps(line) + "\n")


def _event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def kernel_part(a):
    from triforce_amd import ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    for rows, V in ((8, 32000), (1024, 32000), (8, 128256)):
        x = torch.randn(rows, V, device=dev, generator=gen) * 4.0
        t = torch.randint(0, V, (rows,), device=dev, generator=gen)
        out = torch.empty(rows, device=dev)
        forms = {"device_targets": lambda: ops.token_logprobs(x, t, out=out)}
        if rows <= ops.TOKEN_LOGPROBS_MAX_IDS:
            ids = t.tolist()
            forms["ids_as_arguments"] = lambda: ops.token_logprobs(x, ids, out=out)
        for fn in forms.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(a.launches):
            for k, fn in forms.items():                  # alternated
                times[k].append(_event_ms(fn) * 1e3)
        for k, v in times.items():
            us = statistics.median(v)
            _emit({"what": "tf_token_logprobs alone", "part": "a", "form": k, "rows": rows, "V": V, "launches": len(v),
                   "median_us": round(us, 2), "min_us": round(min(v), 2),
                   "logits_GB_per_s": round(rows * V * 4 / us / 1e3, 1)}, a.out)


def engine_parts(a, parts):
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
    if "b" in parts:
        eng = ge.engine
        body, nxt = input_ids[:, :-1], input_ids[0, 1:].contiguous()

        def prefill(score):
            eng.kv_cache.reset()
            with torch.inference_mode():
                return ge.inference(input_ids=body, next_ids=nxt) if score else ge.inference(input_ids=body)

        prefill(True)                                        # warm-up (hipBLASLt heuristics, allocator)
        torch.cuda.synchronize()
        secs = {False: [], True: []}
        for _ in range(a.prefill_pairs):
            for score in (False, True):                      # alternated
                secs[score].append(_event_ms(lambda: prefill(score)) / 1e3)
        lp = prefill(True)[1]
        _emit({"what": "target chunked prefill, BASELINE configs[1] engine, " + wlabel, "part": "b", "prefill": args.prefill,
               "pairs": a.prefill_pairs, "seconds_plain": [round(s, 4) for s in secs[False]],
               "seconds_prompt_logprobs": [round(s, 4) for s in secs[True]],
               "median_plain_s": round(statistics.median(secs[False]), 4),
               "median_prompt_logprobs_s": round(statistics.median(secs[True]), 4),
               "mean_nll": round(float(-lp.double().mean()), 5)}, a.out)
    if "c" in parts:
        run = TriForceRunner(bench._Tok(), ge, args.gamma, top_p=args.top_p, temperature=args.temp,
                             rng=UniformSource(device, seed=args.seed), logprobs=True)
        bench.do_prefill(run, ge, input_ids, "real")
        for _ in range(8):
            run.step()
        on_device = run._device_sets() is not None
        ms = {False: [], True: []}
        for _ in range(a.blocks):
            for score in (False, True):                      # alternated blocks of one runner: same engine, same stream
                run.logprobs = score
                torch.cuda.synchronize()
                ms[score].append(_event_ms(lambda: [run.step() for _ in range(a.block_steps)]) / a.block_steps)
        run.logprobs = True
        _emit({"what": "TriForceRunner steps, BASELINE configs[1] engine, " + wlabel, "part": "c", "blocks": a.blocks,
               "block_steps": a.block_steps, "step_set_up_on_device": on_device,
               "ms_per_step_plain": [round(x, 3) for x in ms[False]], "ms_per_step_logprobs": [round(x, 3) for x in ms[True]],
               "median_plain_ms": round(statistics.median(ms[False]), 3),
               "median_logprobs_ms": round(statistics.median(ms[True]), 3)}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--prefill", type=int, default=124928)
    ap.add_argument("--prefill-pairs", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parts = set(a.parts.split(","))
    assert parts <= {"a", "b", "c"} and a.launches >= 30
    if "a" in parts:
        kernel_part(a)
    if parts & {"b", "c"}:
        engine_parts(a, parts)


if __name__ == "__main__":
    main()
