# python test/on_chip.py --prefill 124928 --budget 4096 --chunk_size 8 --top_p 0.9 --temp 0.6 --gamma 6
"""Entry point #1 — single-GPU on-chip TriForce benchmark with the flags and printed metrics of the reference's
test/on_chip.py: autoregressive baseline, then TriForce, latency and end-to-end speed-up.  Flags live in
triforce_amd/utils/cli.py (reference flags + --weights / --draft-weights / --tokenizer / --greedy / synthetic data)."""
import os
import sys

sys.path.append(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache, StreamingLLMEvictionCache  # noqa: E402
from triforce_amd.models import zoo  # noqa: E402
from triforce_amd.models.modeling_llama import LlamaForCausalLM  # noqa: E402
from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as LlamaForCausalLM_68M  # noqa: E402
from triforce_amd.models.ngram_draft import NgramCache, NgramDraft  # noqa: E402
from triforce_amd.utils import cli  # noqa: E402
from triforce_amd.utils.decoding import Autoregressive, TriForce, TriForceSession  # noqa: E402
from triforce_amd.utils.graph_infer import GraphInferenceEngine  # noqa: E402
from triforce_amd.utils.misc import colored, print_config  # noqa: E402

DEVICE = "cuda:0"


def penalties(args):
    """--repetition_penalty / --frequency_penalty / --presence_penalty as the keywords of the engine and of both loops."""
    return dict(repetition_penalty=args.repetition_penalty, frequency_penalty=args.frequency_penalty,
                presence_penalty=args.presence_penalty)


def build_engine(args, target, draft):
    """Caches sized as on_chip.py:76-80 (16 sink tokens, recent = draft budget - 16 - gamma) and the captured graphs."""
    # (--followups: a question's rows sit between the document and its answer; 0 by default.  --reanchor_at: the answer may
    #  be longer than the retrieval budget, its rows are the gen_len rows the full cache has room for either way)
    full = FlashSimpleCache(target, args.prefill + args.gen_len + 16 + (args.followup_len if args.followups > 0 else 0))
    budget = args.budget
    if budget > args.prefill:                      # a prompt shorter than the budget: every chunk of it is selected
        budget = args.prefill - args.prefill % args.chunk_size
        print(colored(f"retrieval budget {args.budget} > prefill {args.prefill}: using {budget}", "yellow"))
    retrieval = RetrievalCache(target, max_budget=budget, prefill=args.prefill, gamma=args.gamma,
                               chunk_size=args.chunk_size)
    if isinstance(draft, NgramDraft):              # --draft ngram: the token history of the full cache's rows, no K/V
        streaming = NgramCache(full.max_budget, draft.device, gamma=args.gamma)
    else:
        streaming = StreamingLLMEvictionCache(draft, start_size=16, recent_size=args.draft_cache_budget - 16 - args.gamma,
                                              gamma=args.gamma)
    engine = GraphInferenceEngine(target, full, retrieval, draft, streaming)
    engine.initialize_cuda_graph(args.gamma, probs=True, temperature=args.temp, top_p=args.top_p, top_k=args.top_k,
                                 min_p=args.min_p, **penalties(args))
    for c in (full, retrieval, streaming):
        c.print_status()
    return engine


def load_draft(args, target):
    """--draft llama-68M (default): the 68M-shaped draft of the target's vocabulary.  --draft ngram: the prompt-lookup draft
     — no 68M is built or loaded."""
    if cli.is_ngram_draft(args):
        print(colored(f"--draft ngram (--ngram_max {args.ngram_max}): no 68M draft is built; --draft-weights "
                      f"({args.draft_weights}) and --draft_cache_budget ({args.draft_cache_budget}) are ignored", "yellow"))
        return NgramDraft(target.config.vocab_size, target.device, ngram_max=args.ngram_max)
    return cli.load_causal_lm(LlamaForCausalLM_68M, cli.draft_weights(args), zoo.draft_for(args.target), DEVICE)


def followups(args, tokenizer, engine, prompt, vocab_size, sampling):
    """--followups N: prefill the document once, answer it, then ask N synthetic questions of --followup_len tokens against
    the same prefilled document (keep = prefill) and print each one's time to first token and decode speed."""
    import torch
    if args.followup_len < 1:
        raise SystemExit("--followups needs --followup_len >= 1")
    session = TriForceSession(tokenizer, engine, args.gamma, verbose=args.verbose, rebuild_every=args.rebuild_every,
                              reanchor_at=args.reanchor_at, logprobs=args.logprobs, **sampling)
    session.prefill(prompt)
    first = session.generate(args.gen_len)
    print(colored(f"[Session] prefill {prompt.shape[1]} tokens: time to first token {first['ttft']:.3f} s, "
                  f"{first['tokens_per_s']:.2f} tokens/s", "red"))
    if args.logprobs:
        print(colored(f"[Session] generation: mean log-probability {cli.mean(first['logprobs']):.4f}", "red"))
    gen = torch.Generator().manual_seed(0)
    for i in range(args.followups):
        question = torch.randint(3, vocab_size, (1, args.followup_len), generator=gen).to(prompt.device)
        st = session.ask(question, args.gen_len, keep=args.prefill)
        print(colored(f"[Session] follow-up {i + 1}/{args.followups} ({args.followup_len} tokens, keep {args.prefill}): "
                      f"time to first token {st['ttft']:.3f} s, {st['tokens_per_s']:.2f} tokens/s", "red"))
        if args.logprobs:
            print(colored(f"[Session] follow-up {i + 1}/{args.followups}: mean log-probability of the answer "
                          f"{cli.mean(st['logprobs']):.4f} over {len(st['logprobs'])} tokens", "red"))


def report_logprobs(tokenizer, engine, prompts, run):
    """--logprobs: one more TriForce run per prompt that scores the prompt during its prefill and every emitted token
    (DESIGN section 23), outside the timed runs above."""
    import math
    for i, p in enumerate(prompts):
        st = TriForce(tokenizer, engine, p, return_details=True, logprobs=True, prompt_logprobs=True, **run)
        nll = -float(st["prompt_logprobs"].double().mean())
        print(colored(f"[Logprobs] prompt {i + 1}/{len(prompts)} ({p.shape[1]} tokens): mean negative log-likelihood {nll:.4f}, "
                      f"perplexity {math.exp(nll):.3f}", "red"))
        print(colored(f"[Logprobs] generation: mean log-probability {cli.mean(st['logprobs']):.4f} over "
                      f"{len(st['logprobs'])} tokens", "red"))


def main():
    args = cli.parse("on_chip")
    cli.target_config(args.target)
    target = cli.load_causal_lm(LlamaForCausalLM, args.weights, args.target, DEVICE)
    draft = load_draft(args, target)
    tokenizer, prompts = cli.load_prompts(args, target.config.vocab_size)
    sampling = dict(top_k=args.top_k, top_p=args.top_p, temperature=args.temp)
    print_config(draft, target, args.prefill, args.gen_len, args.gamma, file_path=args.file, method="TriForce",
                 spec_args={"budget": args.budget, "chunk_size": args.chunk_size}, dataset=args.dataset, **sampling)
    engine = build_engine(args, target, draft)
    sampling["min_p"] = args.min_p                   # (target tier only, like top_k; print_config has the reference's columns)
    sampling.update(penalties(args))                 # (target tier only as well: DESIGN section 31)
    print(colored(f"tokenized_prompts length: {len(prompts)}", "green"))

    def clip(p):
        return p.to(target.device)[:, :args.prefill]

    # ---- autoregressive baseline (one warm-up run, then the first prompt timed) ----
    Autoregressive(tokenizer, engine, clip(prompts[0]), max_len=args.gen_len, verbose=args.verbose, **sampling)
    ar_speed = [Autoregressive(tokenizer, engine, clip(p), max_len=args.gen_len, verbose=args.verbose, **sampling)
                for p in prompts[:1]]
    baseline_latency = 1000 / cli.mean(ar_speed)
    print(colored(f"[Autoregressive] average latency: {baseline_latency} ms", "red"))

    # ---- TriForce (three warm-up runs, which also leave the retrieval cache's init_graph set) ----
    spec_args = {"budget": args.budget, "draft": args.draft, "chunk_size": args.chunk_size, "gamma": args.gamma,
                 "temperature": args.temp, "top_p": args.top_p, "baseline": baseline_latency / 1000}
    run = dict(gamma=args.gamma, max_len=args.gen_len, verbose=args.verbose, dataset=args.dataset, spec_args=spec_args,
               rebuild_every=args.rebuild_every, reanchor_at=args.reanchor_at, **sampling)
    for _ in range(3):
        TriForce(tokenizer, engine, clip(prompts[0]), **run)
    results = [TriForce(tokenizer, engine, clip(p), file_path=args.file, **run) for p in prompts]
    if args.logprobs:
        report_logprobs(tokenizer, engine, [clip(p) for p in prompts], run)
    method_latency = 1000 / cli.mean([speed for _, speed in results])
    print(colored(f"average acceptance rate (NOT per token): {cli.mean([acc for acc, _ in results])}", "red"))
    print(colored(f"[TriForce] average latency: {method_latency} ms", "red"))
    print(colored(f"[E2E Speedup]: {baseline_latency / method_latency}", "red"))

    if args.followups > 0:
        for p in prompts:
            followups(args, tokenizer, engine, clip(p), target.config.vocab_size, sampling)


if __name__ == "__main__":
    main()
