"""How often could the retrieval verify of inner iteration k already decide iteration k + 1?  

An inner iteration of Middle_Spec at position n draws d, verifies it and, when it is accepted, draws the follow-up b.  If a
guess of b had stood in the verify block's next row (and a draft token behind it), the SAME forward would have produced the
probability rows the next iteration needs: that iteration's retrieval verify could be skipped.  This tool counts, on the
bench's default workload and with existing kernels only, how often such a guess would have been right:

  * coupled draw : guess = invcdf(draft(tok[:n + 2]), u[c + 2]) — the very uniform b is drawn with;
  * argmax       : guess = argmax draft(tok[:n + 2]).

The decode loop itself is untouched (plain inner graphs): after every inner replay the draft's graph for n + 1 tokens is
replayed on the side over the token buffer the iteration left behind, both guesses are written to side buffers, and they
are compared with the recorded (acc, b) after the run.  The tool then walks every step's iterations as the lookahead loop
would (a hit skips the next replay; lookahead only at n <= gamma - 3) and projects the gain from the measured stage
latencies:   hits x retrieval_verify_us - lookahead replays x 2 x (draft_step_us + draw_us)   per step.

Depth 3: the same recorded iterations are also walked as a loop of depth <= 3 would run them
(`walk_depth`: a replay at n <= gamma - 5 decides up to three iterations while every guess holds), and the replays per step by
form, the third decisions per step and the net saving over depth 2,
    skipped replays x retrieval_verify_us - additional draft steps x (draft_step_us + draw_us)   per step,
go to profiles/lookahead3_hit_rate.jsonl with the per-step record [n, accepted, guess hit] of every iteration.

    python tools/lookahead_count.py [profiles/lookahead_hit_rate.jsonl] [--depth3-out profiles/lookahead3_hit_rate.jsonl]
                                    [--steps 200] [bench.py workload flags]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def walk(steps, gamma, key):
    """Replays / lookahead replays / hits of the lookahead loop over the recorded iterations (per step: [(n, acc, hit..)])."""
    replays = looks = hits = 0
    for its in steps:
        i = 0
        while i < len(its):
            it = its[i]
            replays += 1
            if it["n"] <= gamma - 3:
                looks += 1
                if it[key] and i + 1 < len(its):
                    hits += 1
                    i += 1                           # the next logical iteration rides on this replay
            i += 1
    return replays, looks, hits


def walk_depth(steps, gamma, key, max_depth=3):
    """The recorded iterations walked as a loop of lookahead depth <= max_depth would run them.  

    `steps` is a list of steps, each a list of iterations `{"n": position, key: the follow-up guess was right (and d accepted)}`
    in the order the plain loop ran them.  A replay at position n takes the largest depth D <= max_depth with
    n + 2 (D - 1) + 1 <= gamma; stage s + 1 of it runs iff stage s hit, and every stage that ran decides one recorded
    iteration.  Returns counts over all steps: replays by depth chosen, decisions by stage reached, draft steps (2 D - 1 per
    replay) and the logical iterations decided.
    """
    by_depth = {d: 0 for d in range(1, max_depth + 1)}
    decided = {d: 0 for d in range(1, max_depth + 1)}      # replays that decided exactly d iterations
    draft_steps = iterations = 0
    for its in steps:
        i = 0
        while i < len(its):
            n = its[i]["n"]
            depth = 1
            while depth < max_depth and n + 2 * depth + 1 <= gamma:
                depth += 1
            by_depth[depth] += 1
            draft_steps += 2 * depth - 1
            ran = 1
            while ran < depth and its[i + ran - 1][key] and i + ran < len(its):
                ran += 1
            decided[ran] += 1
            iterations += ran
            i += ran
    return {"replays": sum(by_depth.values()), "replays_by_depth": by_depth, "decided": decided,
            "draft_steps": draft_steps, "iterations": iterations}


def project_depth3(steps, gamma, key, rv_us, draft_us, draw_us):
    """Depth 3 against depth 2 over the same recorded iterations: replays per step by form, third decisions, net saving."""
    k = max(len(steps), 1)
    w2, w3 = walk_depth(steps, gamma, key, 2), walk_depth(steps, gamma, key, 3)
    skipped = w2["replays"] - w3["replays"]
    more_drafts = w3["draft_steps"] - w2["draft_steps"]
    return {"depth2": {"replays_per_step": round(w2["replays"] / k, 4), "draft_steps_per_step": round(w2["draft_steps"] / k, 4)},
            "depth3": {"replays_per_step": round(w3["replays"] / k, 4), "draft_steps_per_step": round(w3["draft_steps"] / k, 4),
                       "replays_per_step_by_form": {"depth3": round(w3["replays_by_depth"][3] / k, 4),
                                                    "depth2": round(w3["replays_by_depth"][2] / k, 4),
                                                    "plain": round(w3["replays_by_depth"][1] / k, 4)},
                       "third_decisions_per_step": round(w3["decided"][3] / k, 4),
                       "third_decisions_per_depth3_replay": round(w3["decided"][3] / max(w3["replays_by_depth"][3], 1), 4)},
            "skipped_replays_per_step": round(skipped / k, 4), "more_draft_steps_per_step": round(more_drafts / k, 4),
            "projected_net_saving_us_per_step": round((skipped * rv_us - more_drafts * (draft_us + draw_us)) / k, 1),
            "marginal_break_even_third_rate": round(2 * (draft_us + draw_us) / rv_us, 4)}


def measured_step_ms():
    """Median ms per step of the depth-2 form's 200-step bench runs (profiles/lookahead_bench.jsonl), the gate's denominator."""
    path = os.path.join(ROOT, "profiles", "lookahead_bench.jsonl")
    if not os.path.exists(path):
        return None
    runs = [json.loads(line) for line in open(path) if line.strip()]
    ms = sorted(r["ms_per_step"] for r in runs if r.get("build") == "change" and r.get("run", "").startswith("series-"))
    return ms[len(ms) // 2] if ms else None


def main():
    os.environ["TRIFORCE_INNER_LOOKAHEAD"] = "0"        # the count rides on the PLAIN inner graphs: one decision per replay
    argv = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "lookahead_hit_rate.jsonl")
    if argv and not argv[0].startswith("--"):
        out_path, argv = argv[0], argv[1:]
    out3_path = os.path.join(ROOT, "profiles", "lookahead3_hit_rate.jsonl")
    if "--depth3-out" in argv:
        k = argv.index("--depth3-out")
        out3_path, argv = argv[k + 1], argv[:k] + argv[k + 2:]
    if "--steps" not in argv:
        argv += ["--steps", "200"]
    args = bench.parse(argv + ["--warmup", "5"] if "--warmup" not in argv else argv)
    from triforce_amd import ops
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.sampling import UniformSource
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    kind, tspec, dspec, wlabel = bench.resolve_weights(args)
    target, draft = bench.load_models(args, dev, kind, tspec, dspec)
    ge = bench.build_engine(args, dev, target, draft)
    tcfg, _ = bench.target_config(args.target)
    input_ids = torch.randint(3, tcfg.vocab_size, (1, args.prefill), generator=torch.Generator().manual_seed(args.seed)).to(dev)
    run = TriForceRunner(bench._Tok(), ge, args.gamma, top_k=-1, top_p=args.top_p, temperature=args.temp,
                         rng=UniformSource(dev, seed=args.seed))
    bench.do_prefill(run, ge, input_ids, args.prefill_mode)
    if run.inner is None:
        raise SystemExit("the runner has no inner-iteration graphs (TRIFORCE_INNER_GRAPH=0, no mailbox?): nothing to count")
    for _ in range(args.warmup):
        run.step()

    gamma, rng = args.gamma, run.rng
    cap = args.steps * gamma + 8
    guess = torch.full((cap, 2), -1, dtype=torch.int64, device=dev)      # [coupled draw, argmax] per inner iteration
    log, steps, state = [], [], {}
    plain_replay, plain_read = run.inner.replay, run.bufs.mid_out.read

    def replay(n):
        state["n"], state["pos"] = n, rng.pos
        return plain_replay(n)

    def read(k):
        acc, b, d, at = plain_read(k)
        n, pos, i = state["n"], state["pos"], len(log)
        # on the side, behind the record: the draft over tok[:n + 2] = [.., t_n, d] and the two guesses of the follow-up token
        with torch.inference_mode():
            q2 = ge.replay_draft(n + 1)
            ops.sample_inverse_cdf(q2, rng.buf[pos + 2:pos + 3], guess[i, 0:1])
            guess[i, 1:2].copy_(torch.argmax(q2).view(1))
        log.append(dict(n=n, acc=int(acc), b=int(b)))
        steps[-1].append(log[-1])
        return [acc, b, d, at]

    run.inner.replay, run.bufs.mid_out.read = replay, read
    n0, acc0, dr0, in0 = run.n, run.accepted_count, run.draft_count, run.inner_iters
    for _ in range(args.steps):
        steps.append([])
        run.step()
    torch.cuda.synchronize()
    del run.inner.replay, run.bufs.mid_out.read
    g = guess[:len(log)].tolist()
    for it, (gc, ga) in zip(log, g):
        it["hit_coupled"] = bool(it["acc"] and gc == it["b"])
        it["hit_argmax"] = bool(it["acc"] and ga == it["b"])

    by_n = []
    for n in range(gamma):
        at_n = [it for it in log if it["n"] == n]
        by_n.append(dict(n=n, iterations=len(at_n), accepted=sum(it["acc"] for it in at_n),
                         hits_coupled=sum(it["hit_coupled"] for it in at_n), hits_argmax=sum(it["hit_argmax"] for it in at_n),
                         eligible=n <= gamma - 3))
    stages = bench.stage_latencies(ge, args, dev)
    with torch.inference_mode():
        q, tok = ge.replay_draft(0), torch.zeros(1, dtype=torch.int64, device=dev)
        draw_us = bench._timed(lambda: ops.sample_inverse_cdf_cur(q, rng.buf, rng.cursor, 0, tok), 50)
    iters = len(log)
    res = {"what": "would-be lookahead hits of the inner loop, counted beside the plain decode (tools/lookahead_count.py)",
           "weights": wlabel, "steps": args.steps, "warmup": args.warmup, "gamma": gamma, "tokens": run.n - n0,
           "inner_iterations": iters, "inner_iterations_per_step": round(iters / args.steps, 3),
           "inner_acceptance": round(sum(it["acc"] for it in log) / max(iters, 1), 4), "by_n": by_n,
           "stage_latency_us": stages, "draw_us": round(draw_us, 1)}
    assert iters == run.inner_iters - in0
    rv, extra = stages["retrieval_verify_us"], 2 * (stages["draft_step_us"] + draw_us)
    for name in ("coupled", "argmax"):
        key = "hit_" + name
        eligible_hits = sum(it[key] for it in log if it["n"] <= gamma - 3)
        replays, looks, hits = walk(steps, gamma, key)
        saved_us = (hits * rv - looks * extra) / args.steps
        res[name] = {"s_per_replay": round(eligible_hits / max(iters, 1), 4),
                     "s_per_eligible_replay": round(eligible_hits / max(sum(r["iterations"] for r in by_n if r["eligible"]), 1), 4),
                     "walk": {"replays_per_step": round(replays / args.steps, 3), "lookahead_replays_per_step": round(looks / args.steps, 3),
                              "hits_per_step": round(hits / args.steps, 3), "s_per_lookahead_replay": round(hits / max(looks, 1), 4)},
                     "projected_saving_us_per_step": round(saved_us, 1)}
    res["break_even_s"] = round(extra / rv, 4)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)

    # depth 3 against depth 2 over the same recorded iterations, priced from this run's own latencies
    res3 = {"what": "the recorded inner iterations walked as a depth-3 lookahead loop would run them (tools/lookahead_count.py)",
            "weights": wlabel, "steps": args.steps, "warmup": args.warmup, "gamma": gamma, "inner_iterations": iters,
            "stage_latency_us": stages, "draw_us": round(draw_us, 1), "guess": "coupled"}
    res3.update(project_depth3(steps, gamma, "hit_coupled", rv, stages["draft_step_us"], draw_us))
    step_ms = measured_step_ms()
    if step_ms:
        res3["measured_step_ms"] = step_ms
        res3["projected_net_saving_fraction_of_step"] = round(res3["projected_net_saving_us_per_step"] / (step_ms * 1e3), 4)
    res3["iterations_by_step"] = [[[it["n"], it["acc"], int(it["hit_coupled"])] for it in its] for its in steps]   # [n, acc, hit]
    with open(out3_path, "a") as f:
        f.write(json.dumps(res3) + "\n")
    print(json.dumps({k: v for k, v in res3.items() if k != "iterations_by_step"}), flush=True)


if __name__ == "__main__":
    main()
