"""What the prompt-lookup n-gram draft tier costs and does.  HIP events, warm-up first, the forms of a
comparison alternated in one process, medians over rounds.  One JSON line per measurement, appended to --out.
  (a) kernel : microseconds per tf_ngram_draft launch as back-to-back replays of a captured one-launch hipGraph, at
               L in {2 048, 124 928} x V in {32 000, 151 936}, N = 3, a random history; and, in the same rounds of the same
               process, the 68M draft step the loop replays (GraphInferenceEngine.replay_draft(0) over a full StreamingLLM
               window, V = 32 000: the README's draft_step_us).  The bytes a launch must move are 4 L + 4 V.
               CONDITION: at L = 124 928, V = 32 000 the n-gram launch is cheaper than the 68M step.
  (b) decode : TriForceRunner steps of the default bench shape (aligned synthetic 7B, 124 928-token prompt) with the 68M tier
               and with --draft ngram over the SAME target and caches: tokens/s, inner iterations per step, middle-tier
               acceptance.  Synthetic weights say nothing about acceptance on text, and no trained checkpoint is at hand.
    python tools/ngram_draft_bench.py --parts a,b [--out profiles/ngram_draft.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
DEV = "cuda:0"


def _emit(line, out):
    print(json.dumps(line), flush=True)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "a") as f:
            f.write(json.dumps(line) + "\n")


def _replays_us(replay, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        replay()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / n


def _ngram_graph(L, V, cap, seed):
    from triforce_amd import ops
    gen = torch.Generator().manual_seed(seed)
    hist = torch.randint(0, V, (cap,), generator=gen).to(torch.int32).to(DEV)
    length = torch.tensor([L], dtype=torch.int32, device=DEV)
    blk = torch.randint(0, V, (1,), generator=gen).to(DEV)
    q = torch.empty(V, dtype=torch.float32, device=DEV)
    info = torch.zeros(4, dtype=torch.int32, device=DEV)
    ws = ops.ngram_workspace(DEV)
    run = lambda: ops.ngram_draft(hist, length, blk, 3, V, q=q, info=info, ws=ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run()
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    want = ops.ngram_draft_host(hist.cpu(), length.cpu(), blk.cpu(), 3, V)
    graph.replay()
    torch.cuda.synchronize()
    assert info.cpu().tolist() == want[1].tolist() and torch.equal(q.cpu(), want[0])      # what is timed is right
    return graph, (hist, length, blk, q, info, ws)


@torch.inference_mode()
def kernel_part(a):
    import bench
    args = bench.parse(["--gpus", "1", "--steps", "1", "--warmup", "1", "--target", "tiny", "--prefill", "2048", "--budget", "512",
                        "--weights", "random:1"])
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    kind, tspec, dspec, _ = bench.resolve_weights(args)
    target, draft = bench.load_models(args, device, kind, tspec, dspec)
    ge = bench.build_engine(args, device, target, draft)
    g = torch.Generator(device=device).manual_seed(1)
    ge.engine.draft_cache.k.normal_(generator=g)                   # a full window: the step's cost does not depend on the values
    ge.engine.draft_cache.v.normal_(generator=g)
    ge.tok_buf.fill_(100)
    shapes = [(L, V) for L in (2048, 124928) for V in (32000, 151936)]
    keep = []
    forms = {"draft_68m_step": lambda: ge.replay_draft(0)}
    for i, (L, V) in enumerate(shapes):
        graph, bufs = _ngram_graph(L, V, 124928 + 2048, 20 + i)
        keep.append(bufs)
        forms[f"ngram_L{L}_V{V}"] = graph.replay
    for fn in forms.values():
        _replays_us(fn, a.replays)
    torch.cuda.synchronize()
    rounds = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, fn in forms.items():
            rounds[k].append(_replays_us(fn, a.replays))
    med = {k: round(statistics.median(v), 2) for k, v in rounds.items()}
    key = "ngram_L124928_V32000"
    _emit({"what": "tf_ngram_draft launch against the 68M draft step, captured graphs replayed back to back", "part": "a",
           "N": 3, "rounds": a.rounds, "replays_per_round": a.replays, "median_us": med,
           "min_us": {k: round(min(v), 2) for k, v in rounds.items()}, "max_us": {k: round(max(v), 2) for k, v in rounds.items()},
           "bytes_moved": {f"ngram_L{L}_V{V}": 4 * L + 4 * V for L, V in shapes},
           "GB_per_s": {f"ngram_L{L}_V{V}": round((4 * L + 4 * V) / med[f"ngram_L{L}_V{V}"] / 1e3, 1) for L, V in shapes},
           "condition": f"{key} < draft_68m_step", "condition_met": med[key] < med["draft_68m_step"],
           "ratio_68m_over_ngram": round(med["draft_68m_step"] / med[key], 2)}, a.out)


@torch.inference_mode()
def decode_part(a):
    import bench
    from triforce_amd.models.ngram_draft import NgramCache, NgramDraft
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.graph_infer import GraphInferenceEngine
    from triforce_amd.utils.sampling import UniformSource
    args = bench.parse(["--gpus", "1", "--steps", "1", "--warmup", "1", "--prefill", str(a.prefill), "--gen_cap", "2048"])
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    kind, tspec, dspec, wlabel = bench.resolve_weights(args)
    target, draft = bench.load_models(args, device, kind, tspec, dspec)
    ge = bench.build_engine(args, device, target, draft)
    tcfg, _ = bench.target_config(args.target)
    input_ids = torch.randint(3, tcfg.vocab_size, (1, args.prefill), generator=torch.Generator().manual_seed(args.seed)).to(device)
    tiers = []
    for name in ("llama-68M", "ngram"):
        if name == "ngram":                                        # the same target, full cache and retrieval cache
            eng = ge.engine
            ge = GraphInferenceEngine(target, eng.kv_cache, eng.graph_cache, NgramDraft(tcfg.vocab_size, device, ngram_max=a.ngram_max),
                                      NgramCache(eng.kv_cache.max_budget, device, gamma=args.gamma))
            ge.initialize_cuda_graph(args.gamma, probs=True, temperature=args.temp, top_p=args.top_p, verbose=False)
        run = TriForceRunner(bench._Tok(), ge, args.gamma, top_p=args.top_p, temperature=args.temp,
                             rng=UniformSource(device, seed=args.seed))
        bench.do_prefill(run, ge, input_ids, "real")
        for _ in range(a.warm_steps):
            run.step()
        n0, steps0, inner0 = run.n, len(run.counts), run.inner_iters
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(a.steps):
            run.step()
        torch.cuda.synchronize()
        dt = time.time() - t0
        st = run.stats(dt)
        steps = len(run.counts) - steps0
        tiers.append({"draft": name, "steps": steps, "tokens": run.n - n0, "tokens_per_s": round((run.n - n0) / dt, 2),
                      "ms_per_step": round(dt / steps * 1e3, 3), "inner_iterations_per_step": round((run.inner_iters - inner0) / steps, 3),
                      "acc_rate_middle": round(st["acc_rate_middle"], 4), "acceptance_rate": round(st["acceptance_rate"], 4),
                      "tokens_per_step": round((run.n - n0) / steps, 3), "verify_replays": st["verify_replays"],
                      "lookahead_replays": st["lookahead_replays"], "lookahead_hits": st["lookahead_hits"]})
    _emit({"what": "TriForceRunner steps, BASELINE configs[1] engine, 68M tier against the n-gram tier, " + wlabel, "part": "b",
           "prefill": args.prefill, "gamma": args.gamma, "ngram_max": a.ngram_max, "warm_steps": a.warm_steps, "tiers": tiers,
           "note": "synthetic weights say nothing about acceptance on text; no trained checkpoint was at hand"}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--prefill", type=int, default=124928)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--warm-steps", type=int, default=10)
    ap.add_argument("--ngram_max", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parts = set(a.parts.split(","))
    assert parts <= {"a", "b"} and a.rounds >= 3
    if not torch.cuda.is_available():
        raise SystemExit("tools/ngram_draft_bench.py measures on the GPU: no device found")
    if "a" in parts:
        kernel_part(a)
    if "b" in parts:
        decode_part(a)


if __name__ == "__main__":
    main()
