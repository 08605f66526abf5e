#!/usr/bin/env python
"""Time to first token of a follow-up question against a prefilled document (TriForceSession.ask, keep = prefill: DESIGN
section 18) against the only alternative without it, a full prefill() of document + question, on the same engine, the two
alternated; then the decode ms / step after ask() against a fresh run's.

    python tools/session_bench.py --out profiles/session_bench.json

One JSON object: per question length the alternated times (seconds), the split of ask() into target feed / retrieval
rebuild / draft refill, and the decode comparison with the step form the loop took."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import bench  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--target", default="llama-7B-128K")
    ap.add_argument("--prefill", type=int, default=124928)
    ap.add_argument("--budget", type=int, default=4096)
    ap.add_argument("--chunk_size", type=int, default=8)
    ap.add_argument("--gamma", type=int, default=6)
    ap.add_argument("--temp", type=float, default=0.6)
    ap.add_argument("--top_p", type=float, default=0.9)
    ap.add_argument("--weights", default="aligned:0.7:0.9")
    ap.add_argument("--followup-lens", default="64,1024", help="question lengths, comma separated")
    ap.add_argument("--repeats", type=int, default=3, help="alternations of full prefill / ask per question length")
    ap.add_argument("--steps", type=int, default=200, help="decode steps timed after ask() and after a fresh prefill")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON object here")
    return ap.parse_args(argv)


def step_form(run):
    """Which form the outer steps of this runner take."""
    if run._device_sets() is not None and run.rebuild_every == 0 and run.eager_every == 0:
        return "on_device"
    if hasattr(run.ge, "verify_probs_ids") and run.ge.target_graphs:
        return "verify_probs_ids"
    return "eager"


def timed_steps(run, steps, blocks=10):
    """ms / step over `steps` steps, and the per-block figures (the spread is the noise band)."""
    torch.cuda.synchronize()
    per_block, t_all = [], time.time()
    for b in range(blocks):
        t0 = time.time()
        for _ in range(steps // blocks):
            run.step()
        torch.cuda.synchronize()
        per_block.append((time.time() - t0) / (steps // blocks) * 1e3)
    total = (time.time() - t_all) / (steps // blocks * blocks) * 1e3
    return dict(ms_per_step=round(total, 3), block_min=round(min(per_block), 3), block_max=round(max(per_block), 3),
                tokens_per_step=round(run.n / max(len(run.counts), 1), 3))


def main():
    args = parse()
    lens = [int(x) for x in args.followup_lens.split(",")]
    args.no_graphs = False
    args.gen_cap = max(lens) + (args.steps + 16) * (args.gamma + 2) + 64
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    from triforce_amd.utils.decoding import TriForceSession
    from triforce_amd.utils.sampling import UniformSource
    kind = "aligned" if args.weights.startswith("aligned") else "random"
    specs = (args.weights, args.weights) if kind == "aligned" else ("random:1", "random:2")
    target, draft = bench.load_models(args, device, kind, *specs)
    ge = bench.build_engine(args, device, target, draft)
    tcfg, _ = bench.target_config(args.target)
    gen = torch.Generator().manual_seed(args.seed)
    doc = torch.randint(3, tcfg.vocab_size, (1, args.prefill), generator=gen).to(device)
    session = TriForceSession(bench._Tok(), ge, args.gamma, top_k=-1, top_p=args.top_p, temperature=args.temp,
                              rng=UniformSource(device, seed=args.seed))
    run = session.run
    run.time_extend = True
    out = {"config": dict(target=args.target, prefill=args.prefill, budget=args.budget, gamma=args.gamma, temp=args.temp,
                          top_p=args.top_p, weights=args.weights, kv_cache=os.environ.get("TRIFORCE_KV_CACHE", "fp16")),
           "step_form": None, "followups": []}

    session.prefill(doc)                                   # warm-up: graphs, the draft-prefill graph, calibration
    for _ in range(8):
        run.step()
    out["prefill_document_s"] = round(session.ttft, 4)
    out["step_form"] = step_form(run)

    for n in lens:
        rows = []
        for _ in range(args.repeats):
            q = torch.randint(3, tcfg.vocab_size, (1, n), generator=gen).to(device)
            session.prefill(torch.cat([doc, q], dim=1))    # without extend(): everything again
            full = session.ttft
            for _ in range(4):
                run.step()
            q = torch.randint(3, tcfg.vocab_size, (1, n), generator=gen).to(device)
            session._first_token(run.extend, q, keep=args.prefill)
            split = {k: round(v, 5) for k, v in run.extend_seconds.items() if k.endswith(("feed", "rebuild", "refill"))}
            rows.append(dict(full_prefill_s=round(full, 4), ask_s=round(session.ttft, 4), **split))
            print(json.dumps({"followup_len": n, **rows[-1]}), flush=True)
        mean = {k: round(sum(r[k] for r in rows) / len(rows), 5) for k in rows[0]}
        out["followups"].append(dict(followup_len=n, runs=rows, mean=mean,
                                     ratio_full_over_ask=round(mean["full_prefill_s"] / mean["ask_s"], 2)))

    # decode after ask() (the state the last ask left) against a fresh prefill of the document
    for _ in range(4):
        run.step()
    after = timed_steps(run, args.steps)
    form_after = step_form(run)
    session.prefill(doc)
    for _ in range(4):
        run.step()
    fresh = timed_steps(run, args.steps)
    out["decode"] = dict(after_ask=after, fresh=fresh, step_form_after_ask=form_after, step_form_fresh=step_form(run),
                         after_ask_followup_len=lens[-1])
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
