"""A/B of TRIFORCE_RETRIEVAL_KV on bench.py: every case runs bench.py in a fresh process — from this tree, or
from a checkout of another commit (``--baseline-tree``, the parent: its fp16 retrieval cache is what the knob is compared
against) — and one row per run goes to ``--out``: ms per step, the retrieval-verify stage latency, the middle tier's per-token
acceptance and the process's peak device memory.  Cases alternate (baseline, fp8, baseline, fp8, ...) ``--repeat`` times.

    python tools/retrieval_kv_ab.py --baseline-tree ../parent --out profiles/retrieval_kv_fp8_bench.jsonl
    python tools/retrieval_kv_ab.py --setting g16 --weights fp8 --repeat 3 ...

Settings: ``cfg1`` = bench.py's default (BASELINE configs[1]: prefill 124 928, budget 4 096, gamma 6); ``g16`` = --prefill 130048
--budget 12288 --gamma 16, every layer resident."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = {"cfg1": [], "g16": ["--prefill", "130048", "--budget", "12288", "--gamma", "16"]}
CHILD = ("import json, runpy, sys, torch\n"
         "sys.argv = ['bench.py'] + sys.argv[1:]\n"
         "try:\n"
         "    runpy.run_path('bench.py', run_name='__main__')\n"
         "finally:\n"
         "    print(json.dumps({'max_memory_allocated': torch.cuda.max_memory_allocated()}), flush=True)\n")


def run_case(tree, env_over, bench_args, timeout):
    env = dict(os.environ)
    for k in ("TRIFORCE_RETRIEVAL_KV", "TRIFORCE_RETRIEVAL_WEIGHTS"):
        env.pop(k, None)
    env.update(env_over)
    p = subprocess.run([sys.executable, "-c", CHILD] + bench_args, cwd=tree, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=timeout)
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode != 0 or len(lines) < 2:
        raise RuntimeError(f"bench.py failed in {tree} (rc {p.returncode}):\n{p.stderr[-2000:]}")
    res, mem = lines[-2], lines[-1]
    return {"ms_per_step": res["ms_per_step"], "tokens_per_s": res["value"],
            "retrieval_verify_us": res.get("stage_latency_us", {}).get("retrieval_verify_us"),
            "target_verify_us": res.get("stage_latency_us", {}).get("target_verify_us"),
            "per_token_acceptance_middle": res.get("per_token_acceptance_middle"),
            "acceptance_rate": res.get("acceptance_rate"), "tokens_per_step": res.get("tokens_per_step"),
            "inner_iterations_per_step": res.get("inner_iterations_per_step"), "steps": res["steps"],
            "max_memory_allocated": mem["max_memory_allocated"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setting", nargs="+", default=["cfg1", "g16"], choices=sorted(SETTINGS))
    ap.add_argument("--weights", nargs="+", default=["fp16", "fp8"], choices=["fp16", "fp8"],
                    help="TRIFORCE_RETRIEVAL_WEIGHTS of both sides")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--baseline-tree", default=None, help="checkout whose bench.py gives the fp16 side (default: this tree, knob off)")
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    base_tree = os.path.abspath(args.baseline_tree) if args.baseline_tree else ROOT
    out = open(args.out, "a") if args.out else None
    for setting in args.setting:
        bench_args = ["--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup), "--full", "--no-cpu-baseline",
                      "--random-steps", "0"] + SETTINGS[setting]
        for w in args.weights:
            wenv = {"TRIFORCE_RETRIEVAL_WEIGHTS": w}
            cases = [("fp16 (baseline tree)" if args.baseline_tree else "fp16 (knob unset)", base_tree, wenv),
                     ("fp8", ROOT, dict(wenv, TRIFORCE_RETRIEVAL_KV="fp8"))]
            for rep in range(args.repeat):
                for label, tree, env in cases:
                    row = {"setting": setting, "bench_args": " ".join(SETTINGS[setting]) or "(default)", "retrieval_weights": w,
                           "retrieval_kv": label, "repeat": rep}
                    row.update(run_case(tree, env, bench_args, args.timeout))
                    print(json.dumps(row), flush=True)
                    if out:
                        out.write(json.dumps(row) + "\n")
                        out.flush()


if __name__ == "__main__":
    main()
