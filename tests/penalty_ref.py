"""Reference of the target tier's repetition / frequency / presence penalties (include/triforce_hip.h
"SAMPLING PENALTIES"): the formula as torch fp32 on the CPU, the scalars as fp32 tensors, every operation its own statement —
so every / * - is one IEEE fp32 operation with its own rounding, which is what the kernel is held to bit for bit.  Plus the
small builders the penalty tests share."""
import torch


def counts(gen_count, ids, rows, V):
    """(rows, V) int32: c[i][t] = gen_count[t] + #{ j <= i : ids[j] == t } (ids None: the second term is 0; an id outside
    [0, V) matches nothing)."""
    c = gen_count.to(torch.int32).cpu().reshape(1, V).repeat(rows, 1)
    if ids is not None:
        block = [int(t) for t in torch.as_tensor(ids).reshape(-1)[:rows].tolist()]
        run = torch.zeros(V, dtype=torch.int32)
        for i, t in enumerate(block):
            if 0 <= t < V:
                run[t] += 1
            c[i] += run
    return c


def penalize(logits, ids, gen_count, prompt_seen, repetition, frequency, presence):
    """(rows, V) fp32 logits -> the penalised rows (fp32, CPU)."""
    x = logits.detach().to(torch.float32).cpu()
    rows, V = x.shape
    c = counts(gen_count, ids, rows, V)
    seen = (prompt_seen.cpu().reshape(1, V) != 0) | (c > 0)
    r = torch.tensor(repetition, dtype=torch.float32)
    f = torch.tensor(frequency, dtype=torch.float32)
    p = torch.tensor(presence, dtype=torch.float32)
    y = x.clone()
    if float(r) != 1.0:
        quotient = x / r
        product = x * r
        scaled = torch.where(x > 0, quotient, product)
        y = torch.where(seen, scaled, x)
    cf = c.to(torch.float32)
    fc = f * cf
    lowered = y - fc
    lowered = lowered - p
    return torch.where(c > 0, lowered, y)


class HostState:
    """gen_count / prompt_seen on the host, for teacher-forced checks of a decode stream."""

    def __init__(self, V, context_ids):
        self.gen_count = torch.zeros(V, dtype=torch.int32)
        self.prompt_seen = torch.zeros(V, dtype=torch.uint8)
        self.prompt_seen[torch.as_tensor(context_ids).reshape(-1).long()] = 1

    def commit(self, token):
        self.gen_count[int(token)] += 1


def teacher_forced_penalised_gaps(g, stream, pen, build_oracle, prompt):
    """Feed ``stream`` (first token + generated tokens) through the CPU oracle's autoregressive path and return, for every
    token, how far its PENALISED oracle logit is below the best penalised logit given the same prefix.  The counts are kept on
    the host by the contract: token k's row counts stream[:k] (the pending token stream[k - 1] as the row's own input)."""
    eng, _, _ = build_oracle(g)
    V = g["tcfg"]["vocab_size"]
    st = HostState(V, prompt)
    eng.kv_cache.reset()
    logits = eng.inference(prompt)[0, -1]
    y = penalize(logits.reshape(1, V), None, st.gen_count, st.prompt_seen, *pen)[0]
    gaps = [float(y.max() - y[stream[0]])]
    for i in range(len(stream) - 1):
        logits = eng.model.forward(torch.tensor([[stream[i]]]), eng.kv_cache, None)[0, -1]
        y = penalize(logits.reshape(1, V), [stream[i]], st.gen_count, st.prompt_seen, *pen)[0]
        st.commit(stream[i])
        gaps.append(float(y.max() - y[stream[i + 1]]))
    return gaps


def aligned_streams(device, graphs, pen, n=60):
    """Aligned synthetic weights (models/aligned.py: the drafts mostly agree with the target, so drafted tokens ARE accepted
    and the verify blocks' later rows, with their in-block counts, decide tokens) at temperature 1, top-p 1, min_p = 1: the
    target's distribution is the maximum of the penalised row, so the speculative stream must be the autoregressive stream
    under the same penalties -> (runner, its engine, the Autoregressive ids)."""
    from oracle import specs
    from triforce_amd.models import aligned
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache, StreamingLLMEvictionCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as Draft
    from triforce_amd.utils.decoding import Autoregressive, TriForceRunner
    from triforce_amd.utils.graph_infer import GraphInferenceEngine
    from triforce_amd.utils.sampling import UniformSource
    V, P, B, gamma = 4096, 2048, 256, 4                                # (the shapes of tests/test_aligned_cpu.py)
    tcfg = LlamaConfig.from_dict(specs.tiny_target_config(vocab_size=V, layers=2, hidden=256, heads=2, max_pos=8192))
    dcfg = LlamaConfig.from_dict(specs.draft_68m_config(vocab_size=V))
    spec = aligned.parse_spec("aligned:0.7:0.9:0")
    target = LlamaForCausalLM(tcfg, device).init_aligned(spec, attn_keys=B)
    draft = Draft(dcfg, device).init_aligned(spec, attn_keys=256)
    ge = GraphInferenceEngine(target, FlashSimpleCache(target, P + 400),
                              RetrievalCache(target, max_budget=B, prefill=P, gamma=gamma, chunk_size=8), draft,
                              StreamingLLMEvictionCache(draft, start_size=16, recent_size=256 - 16 - gamma, gamma=gamma))
    kw = dict(repetition_penalty=pen[0], frequency_penalty=pen[1], presence_penalty=pen[2])
    sampling = dict(top_p=1.0, temperature=1.0, min_p=1.0)
    if graphs:
        ge.initialize_cuda_graph(gamma, probs=True, verbose=False, **sampling, **kw)
    else:
        ge.initialize_eager(gamma, probs=True, **sampling, **kw)

    class Tok:
        eos_token_id = 2
    prompt = specs.random_prompt(V, P, 11).to(device)
    run = TriForceRunner(Tok(), ge, gamma, rng=UniformSource(device, seed=3), **sampling, **kw)
    run.prefill(prompt)
    while run.n < n:
        run.step()
    emitted, counts = list(run.emitted), ge.penalty_state.gen_count.clone()
    _, ids = Autoregressive(Tok(), ge, prompt, max_len=len(emitted) - 1, rng=UniformSource(device, seed=4), return_tokens=True,
                            **sampling, **kw)
    return run, ge, counts, ids


def build_engine(g, device, graphs, penalties=(1.0, 0.0, 0.0), temperature=1.0, top_p=1.0, min_p=0.0, tcfg=None, tsd=None,
                 dsd=None):
    """The product engine over the golden's seeded weights (as tests/test_minp_cpu.py builds its own), initialised with
    ``penalties`` = (repetition, frequency, presence) -> (engine, tsd, dsd)."""
    from oracle import specs
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache, StreamingLLMEvictionCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as LlamaForCausalLM_68M
    from triforce_amd.utils.graph_infer import GraphInferenceEngine
    tcfg = g["tcfg"] if tcfg is None else tcfg
    gamma = g["gamma"]
    if tsd is None:
        tsd = specs.random_state_dict(tcfg, g["tseed"], head_std=g.get("head_std", 0.05))
    if dsd is None:
        dsd = specs.random_state_dict(g["dcfg"], g["dseed"], head_std=g.get("head_std", 0.05))
    target = LlamaForCausalLM.from_state_dict(LlamaConfig.from_dict(tcfg), tsd, device)
    draft = LlamaForCausalLM_68M.from_state_dict(LlamaConfig.from_dict(g["dcfg"]), dsd, device)
    ge = GraphInferenceEngine(target, FlashSimpleCache(target, g["prefill"] + g["gen_len"] + 16),
                              RetrievalCache(target, max_budget=g["budget"], prefill=g["prefill"], gamma=gamma, chunk_size=g["chunk"]),
                              draft, StreamingLLMEvictionCache(draft, start_size=16, recent_size=256 - 16 - gamma, gamma=gamma))
    kw = dict(probs=True, temperature=temperature, top_p=top_p, min_p=min_p, repetition_penalty=penalties[0],
              frequency_penalty=penalties[1], presence_penalty=penalties[2])
    if graphs:
        ge.initialize_cuda_graph(gamma, verbose=False, **kw)
    else:
        ge.initialize_eager(gamma, **kw)
    return ge, tsd, dsd
