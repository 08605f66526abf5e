"""The decode loop with top-k on the target tier: bench.py's headline engine (BASELINE configs[1], aligned synthetic weights)
stepped by a TriForceRunner(top_k=K).  Runs on any commit: ``top_k`` goes to initialize_cuda_graph only where the signature has
it — before the device-side top-k the runner left its captured verify for a graph replay + an eager sort chain.  Prints one JSON
line: ms per step, tokens/s, acceptance, and the latency of the target verify as this runner issues it.
    python tools/topk_loop_bench.py --top_k 50 [--steps 100] [--out profiles/topk_loop_bench.jsonl]"""
import argparse
import inspect
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--top_k", type=int, default=50)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--prefill", type=int, default=124928)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    args = bench.parse(["--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup), "--prefill", str(a.prefill)])
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)

    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache, StreamingLLMEvictionCache
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.graph_infer import GraphInferenceEngine
    from triforce_amd.utils.sampling import UniformSource, norm_logits

    kind, tspec, dspec, wlabel = bench.resolve_weights(args)
    target, draft = bench.load_models(args, device, kind, tspec, dspec)
    ge = GraphInferenceEngine(target, FlashSimpleCache(target, args.prefill + args.gen_cap + 16),
                              RetrievalCache(target, max_budget=args.budget, prefill=args.prefill, gamma=args.gamma,
                                             chunk_size=args.chunk_size),
                              draft, StreamingLLMEvictionCache(draft, start_size=16, recent_size=256 - 16 - args.gamma,
                                                               gamma=args.gamma))
    kw = dict(probs=True, temperature=args.temp, top_p=args.top_p, verbose=False)
    takes_top_k = "top_k" in inspect.signature(ge.initialize_cuda_graph).parameters
    if takes_top_k:
        kw["top_k"] = a.top_k
    ge.initialize_cuda_graph(args.gamma, **kw)
    tcfg, _ = bench.target_config(args.target)
    gen = torch.Generator().manual_seed(args.seed)
    input_ids = torch.randint(3, tcfg.vocab_size, (1, args.prefill), generator=gen).to(device)
    run = TriForceRunner(bench._Tok(), ge, args.gamma, top_k=a.top_k, top_p=args.top_p, temperature=args.temp,
                         rng=UniformSource(device, seed=args.seed))
    bench.do_prefill(run, ge, input_ids, "real")
    for _ in range(a.warmup):
        run.step()
    on_device = run._device_sets() is not None
    torch.cuda.synchronize()
    n0, acc0, dr0, t0 = run.n, run.accepted_count, run.draft_count, time.time()
    for _ in range(a.steps):
        run.step()
    torch.cuda.synchronize()
    seconds = time.time() - t0
    tokens = run.n - n0

    # the target verify as THIS runner issues it (rolled back after every probe), and the two draft-side stages
    eng, gamma = ge.engine, args.gamma
    S = eng.kv_cache.seq_len
    ids = torch.full((1, gamma + 1), 100, dtype=torch.long, device=device)
    pos = torch.arange(S, S + gamma + 1, device=device).unsqueeze(0)

    def verify():
        with torch.inference_mode():
            if takes_top_k:
                ge.verify_probs(ids, args.temp, args.top_p, top_k=a.top_k)
            elif a.top_k <= 0:
                ge.verify_probs(ids, args.temp, args.top_p)
            else:
                norm_logits(ge.inference(input_ids=ids)[0], temperature=args.temp, top_k=a.top_k, top_p=args.top_p)
        eng.kv_cache.seq_len = S
    stages = {"target_verify_us": round(bench._timed(verify, 5), 1),
              "retrieval_verify_us": round(bench._timed(lambda: ge.graph_verify(ids, pos), 5), 1),
              "draft_step_with_io_us": round(bench._timed(lambda: ge.graph_draft_inference(ids[:, :3], gamma_offset=2), 20), 1)}
    line = {"what": "TriForceRunner steps, BASELINE configs[1] engine, " + wlabel, "tag": a.tag, "top_k": a.top_k,
            "engine_takes_top_k": takes_top_k, "step_set_up_on_device": on_device, "steps": a.steps,
            "ms_per_step": round(seconds / a.steps * 1e3, 3), "tokens_per_s": round(tokens / seconds, 2),
            "tokens_per_step": round(tokens / a.steps, 3),
            "acceptance_rate": round((run.accepted_count - acc0) / max(run.draft_count - dr0, 1), 4), **stages}
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
