#!/usr/bin/env python
"""bench.py — TriForce decode throughput on MI355X (BASELINE.json metric).

  python bench.py --gpus 1 --steps K --warmup W
  python bench.py --gpus N ...                      (re-executes itself under torch.distributed.run, one rank per GPU)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

Workload (N=1): BASELINE.json configs[1] — Llama2-7B-128K (YaRN) on-chip, prefill 124 928, retrieval budget 4 096,
chunk 8, gamma 6, T=0.6 / top_p=0.9 (reference README.md:49-55).  A *step* is one outer TriForce iteration
(utils/decoding.py:70-141): gamma-bounded Middle_Spec drafting (68M draft graphs + retrieval-verify graph), one target
verify over the full 125K-token KV cache (hipGraph, device-resident lengths), device-side accept/rollback and the cache
fix-ups.  The timed region starts after prefill + retrieval build + draft prefill, exactly like the reference's
time1/time2 (decoding.py:69,143), with device syncs added on both sides.

Weights (--weights): real checkpoints when both are found locally (zoo.find_checkpoint); otherwise — no hub access
offline — ALIGNED SYNTHETIC weights (triforce_amd/models/aligned.py): real shapes, dense values, every kernel streams
the bytes it streams for a trained model, and the draft -> retrieval-model -> full-model acceptance rates are set to
the requested values (default 0.7 / 0.9), so the loop runs in the regime speculative decoding exists for.  The
random-init number of round 1 (acceptance ~0.01: the loop's worst case) is measured in the same process afterwards and
reported as ``random_weights``.

value = tokens emitted in the K timed steps / wall time (tokens/s, whole job); ms_per_step = wall time / K.
roofline = the dominant kernel (split-KV target-verify attention, tf_attn_decode): algorithmic bytes per launch
2*S*H*D*2 / mean launch duration from HIP events recorded on the launch stream INSIDE the timed region:
every --roofline-every-th step runs its target verify eagerly instead of replaying the hipGraph, and every 8th
attention launch of such a verify is bracketed (an event record is a queue packet of its own).

A plain run (N=1) sets up, prefills, warms up, times the K steps and prints the line.  --full adds every measurement
that takes runs of its own after the timed steps: stage latencies and stage rooflines, the autoregressive baseline and
the speedup over it, the committed acceptance-sweep points, the random-weight run (random_weights), and
cpu_baseline = the CPU oracle (oracle/, kind "port") timed on this host for a bounded per-layer sample of the same
step, extrapolated to the step.

--dump-outputs DIR (N=1) writes what the last timed step computed: tokens.npy (the tokens it emitted, float64) and
verify_probs.npy (its target verify's probabilities after temperature / top-p, rows x vocab, float32).  Inputs, weights
and the uniform stream are seeded, so the same arguments give the same inputs in every run.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0        # MI355X HBM3E spec peak (guides/MI355X_MICROARCH.md)
REFERENCE_SPEEDUP = 2.2       # reference README.md:49-55: TriForce vs autoregressive, 1x A100, same config, trained weights


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--target", default="llama-7B-128K", choices=["llama-7B-128K", "llama-13B-128K", "lwm-128K", "tiny"])
    ap.add_argument("--prefill", type=int, default=124928)
    ap.add_argument("--budget", type=int, default=4096)
    ap.add_argument("--chunk_size", type=int, default=8)
    ap.add_argument("--gamma", type=int, default=6)
    ap.add_argument("--temp", type=float, default=0.6)
    ap.add_argument("--top_p", type=float, default=0.9)
    ap.add_argument("--gen_cap", type=int, default=512, help="KV slack reserved for generated tokens")
    ap.add_argument("--weights", default="auto",
                    help="auto = local checkpoints if present, else aligned:0.7:0.9 | aligned[:draft_acc[:retrieval_acc"
                         "[:seed]]] | random[:seed] | <local HF dir of the target> (draft: --draft-weights)")
    ap.add_argument("--draft-weights", default=None, help="local HF dir of the 68M draft (with a checkpoint target)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure stage latencies / rooflines, the AR baseline, the random-weight "
                         "run and the CPU baseline (single-GPU engine; a plain run times the steps only)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step computed to DIR/<name>.npy (single-GPU engine)")
    ap.add_argument("--random-steps", type=int, default=-1,
                    help="steps of the secondary random-init measurement with --full (-1 = min(steps, 12); 0 = skip)")
    ap.add_argument("--ar-steps", type=int, default=16, help="autoregressive steps timed for the AR baseline (--full)")
    ap.add_argument("--roofline-every", type=int, default=4,
                    help="every N-th step's target verify runs eagerly with HIP-event brackets (0 = never)")
    ap.add_argument("--prefill-mode", default="real", choices=["real", "synthetic"],
                    help="real = chunked prefill through the model; synthetic = N(0,1) KV fill "
                         "(the reference's own filler, DistributedSimpleCache.normal_, cache.py:303-308)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--on-chip", type=int, default=-1,
                    help="tensor-parallel / offloading engine: layers whose KV stays in HBM (-1 = all; fewer = the "
                         "offloading tier: the rest streams from pinned host memory every target forward)")
    ap.add_argument("--engine", default="auto", choices=["auto", "single", "tp"],
                    help="auto = single-GPU engine at --gpus 1, tensor-parallel engine above; tp forces the "
                         "TP / offloading engine (test/offloading_TP.py's) at any world size")
    ap.add_argument("--dry-run", action="store_true",
                    help="tensor-parallel path only: build the process group, the sharded engine and its weights, agree "
                         "across ranks, print the JSON line with dry_run=true and exit (no decode; runs on CPU under gloo)")
    ap.add_argument("--share-device", action="store_true",
                    help="tensor-parallel path only: put every rank on cuda:0 (a functional full-size check of world "
                         "size N on a 1-GPU box: real shards, real kernels, one-shot all-reduce across processes; "
                         "large collectives over gloo).  NOT a scaling measurement; the line says so")
    ap.add_argument("--allreduce", default=None, choices=["auto", "oneshot", "rccl"],
                    help="tensor-parallel path: decode-sized all-reduces through the one-shot peer-read kernel after its "
                         "collective self-check (auto: falls back to RCCL if the check fails; oneshot: fail instead of "
                         "falling back) or through RCCL — for A/B on a multi-GPU node.  Default: the environment's "
                         "TRIFORCE_ALLREDUCE if set, else auto")
    ap.add_argument("--require-graph-form", default=None, choices=["whole", "segments", "eager"],
                    help="tensor-parallel path: fail (rc != 0, JSON field 'failed') unless the decode forwards were "
                         "captured in this form")
    ap.add_argument("--eager-comparator", action="store_true",
                    help="also time the same-hardware un-tuned comparator (eager PyTorch-ROCm restatement, ~20 s; implies "
                         "--full: it is priced against the full line's AR baseline)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-graphs", action="store_true")
    ap.add_argument("--rebuild-every", type=int, default=0,
                    help="re-select the retrieval cache every N target verifies (0 = the reference: once per prompt)")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.eager_comparator:
        args.full = True
    if args.random_steps < 0:
        args.random_steps = min(args.steps, 12)
    # a step emits at most gamma + 2 tokens: size the KV slack for the worst case of the requested run
    # (never more than the retrieval budget: its tail holds every generated token, reference cache.py:180-182); the --full
    # measurements are counted with or without --full, so the same arguments always allocate the same caches
    total = args.steps + args.warmup + args.random_steps + 8
    args.gen_cap = max(args.gen_cap, min(total * (args.gamma + 2) + args.ar_steps + 64, args.budget))
    return args


METRIC_NAMES = {"llama-7B-128K": "Llama-7B-128K", "llama-13B-128K": "Llama-13B-128K", "lwm-128K": "LWM-Text-Chat-128K",
                "tiny": "tiny test model"}


def metric_label(target, prefill):
    """BASELINE.json's metric string for the headline workload (7B, 124 928-token prompt); for every other line the
    model and context actually run (a 13B / 130K line must not say "Llama-7B-128K @124K ctx")."""
    return f"decode tokens/sec + avg accepted len, {METRIC_NAMES.get(target, target)} @{prefill // 1000}K ctx"


def target_config(name):
    from triforce_amd.models import zoo
    return zoo.config(name), zoo.config("llama-68M")


def resolve_weights(args):
    """-> (kind, target_spec, draft_spec, label): kind in {"checkpoint", "aligned", "random"}."""
    from triforce_amd.models import zoo
    w = args.weights
    if w == "auto":
        t, d = zoo.find_checkpoint(args.target) if args.target in zoo.CONFIGS else None, zoo.find_checkpoint("llama-68M")
        if t and d:
            return "checkpoint", t, d, f"checkpoints {t} + {d}"
        w = "aligned:0.7:0.9"
    if w == "aligned" or w.startswith("aligned:"):
        return "aligned", w, w, w
    if w.startswith("random"):
        seed = int(w.split(":")[1]) if ":" in w and w.split(":")[1] else args.seed
        return "random", f"random:{seed + 1}", f"random:{seed + 2}", "random-init N(0,0.02) fp16"
    d = args.draft_weights or zoo.find_checkpoint("llama-68M")
    if not d:
        raise SystemExit("--weights <dir> needs --draft-weights <dir> (no local llama-68m checkpoint found)")
    return "checkpoint", w, d, f"checkpoints {w} + {d}"


class _Tok:
    eos_token_id = 2

    def decode(self, *a, **k):
        return ""


def load_models(args, device, kind, tspec, dspec):
    from triforce_amd.models.aligned import parse_spec
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as Draft68M
    tcfg, dcfg = target_config(args.target)
    if kind == "checkpoint":
        return LlamaForCausalLM.from_pretrained(tspec, device_map=device), Draft68M.from_pretrained(dspec, device_map=device)
    if kind == "aligned":
        spec = parse_spec(tspec)
        return (LlamaForCausalLM(tcfg, device).init_aligned(spec, attn_keys=args.budget),
                Draft68M(dcfg, device).init_aligned(spec, attn_keys=256))
    return (LlamaForCausalLM(tcfg, device).init_random(int(tspec.split(":")[1])),
            Draft68M(dcfg, device).init_random(int(dspec.split(":")[1])))


def build_engine(args, device, target, draft):
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache, StreamingLLMEvictionCache
    from triforce_amd.utils.graph_infer import GraphInferenceEngine
    cache = FlashSimpleCache(target, args.prefill + args.gen_cap + 16)
    gcache = RetrievalCache(target, max_budget=args.budget, prefill=args.prefill, gamma=args.gamma,
                            chunk_size=args.chunk_size)
    dcache = StreamingLLMEvictionCache(draft, start_size=16, recent_size=256 - 16 - args.gamma, gamma=args.gamma)
    ge = GraphInferenceEngine(target, cache, gcache, draft, dcache)
    if args.no_graphs:
        ge.initialize_eager(args.gamma, probs=True, temperature=args.temp, top_p=args.top_p)
    else:
        ge.initialize_cuda_graph(args.gamma, probs=True, temperature=args.temp, top_p=args.top_p, verbose=False)
    return ge


def do_prefill(run, ge, input_ids, mode):
    """Everything the reference does before time1 (decoding.py:44-62)."""
    eng = ge.engine
    if mode == "real":
        run.prefill(input_ids)
        return
    eng.kv_cache.reset()
    eng.graph_cache.reset()
    eng.draft_cache.reset()
    P = input_ids.shape[1]
    g = torch.Generator(device=eng.model.device).manual_seed(1234)
    for l in range(eng.kv_cache.layers):             # synthetic prefix KV, layer by layer (bounded temporaries)
        eng.kv_cache.k[l, :, :P - 1].normal_(generator=g)
        eng.kv_cache.v[l, :, :P - 1].normal_(generator=g)
    eng.kv_cache.seq_len = P - 1
    logits = ge.inference(input_ids=input_ids[:, -1:])           # last prompt token: builds the retrieval cache
    ge.graph_draft_prefill(input_ids=input_ids)
    run.calibrate_aligned()
    run.start(logits)


def _timed(fn, n):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


def stage_latencies(ge, args, device):
    """Per-stage latency (us) of the model calls of a step as the loop issues them (graph replays where captured),
    HIP events on the launch stream."""
    eng = ge.engine
    gamma = args.gamma
    S = eng.kv_cache.seq_len
    ids = torch.full((1, gamma + 1), 100, dtype=torch.long, device=device)
    pos = torch.arange(S, S + gamma + 1, device=device).unsqueeze(0)
    # draft step: the replay the loop issues (inner-iteration graphs and the catch-up forward run the draft over the shared
    # token buffer: no input copy, no output clone); `draft_step_with_io_us` is graph_draft_inference with both (two more
    # launches: the figure quoted as draft_step_us up to round 5)
    with_io = _timed(lambda: ge.graph_draft_inference(ids[:, :3], gamma_offset=2), 20)
    if getattr(ge, "tok_buf", None) is not None and hasattr(ge, "replay_draft"):
        with torch.inference_mode():                           # (the engine's static buffers are inference tensors)
            ge.tok_buf[:, :3].copy_(ids[:, :3])
        replay_only = _timed(lambda: ge.replay_draft(2), 20)
    else:
        replay_only = with_io
    out = {"draft_step_us": replay_only, "draft_step_with_io_us": with_io,
           "retrieval_verify_us": _timed(lambda: ge.graph_verify(ids, pos), 5)}

    def tv(eager):
        def f():
            ge.verify_probs(ids, args.temp, args.top_p, eager=eager)
            eng.kv_cache.seq_len = S                   # roll the probe back
        return f
    out["target_verify_us"] = _timed(tv(False), 3)
    out["target_verify_eager_us"] = _timed(tv(True), 3)
    return {k: round(v, 1) for k, v in out.items()}


def autoregressive_baseline(ge, args, first_token):
    """The reference's autoregressive loop (decoding.py:14-37) on the same engine and cache: one full-cache forward of
    one token (hipGraph when captured), temperature / top-p, sample — per token, no host sync inside the loop."""
    from triforce_amd.utils.sampling import UniformSource, norm_logits, sample
    eng = ge.engine
    S = eng.kv_cache.seq_len
    rng = UniformSource(eng.model.device, seed=1)
    tok = torch.tensor([[int(first_token)]], dtype=torch.long, device=eng.model.device)

    def loop(n):
        t = tok
        for _ in range(n):
            logits = ge.decode_step(t)
            t = sample(norm_logits(logits[:, -1, :], temperature=args.temp, top_k=-1, top_p=args.top_p), rng=rng)
        return t
    loop(2)
    torch.cuda.synchronize()
    t0 = time.time()
    loop(args.ar_steps)
    torch.cuda.synchronize()
    dt = time.time() - t0
    eng.kv_cache.seq_len = S
    return args.ar_steps / dt


def cpu_baseline(args, tokens_per_step, inner_per_step):
    """CPU oracle ('port') on this host: one target layer at full cfg shape + lm_head + one retrieval-verify
    layer + one draft forward, extrapolated to a full step.  Bounded to ~10-30 s of CPU work."""
    from oracle import ref_ops as R
    tcfg, dcfg = target_config(args.target)
    H, D, hid, I, L, V = (tcfg.num_attention_heads, tcfg.head_dim, tcfg.hidden_size, tcfg.intermediate_size,
                          tcfg.num_hidden_layers, tcfg.vocab_size)
    q_t, q_r = args.gamma + 2, args.gamma + 1
    S, Rb = args.prefill + q_t, args.budget + args.gamma + 1
    torch.manual_seed(0)
    t0 = time.time()
    kv = torch.empty(S, H, D, dtype=torch.float16).normal_()
    w = {n: (torch.empty(o, i, dtype=torch.float16).normal_() * 0.02) for n, (o, i) in
         dict(qkv=(3 * hid, hid), o=(hid, hid), gu=(2 * I, hid), d=(hid, I), head=(V, hid)).items()}
    setup = time.time() - t0

    def tm(fn):
        t = time.time()
        fn()
        return time.time() - t

    def gemms(rows):
        x = torch.randn(rows, hid).half()
        h = R.rms_norm(x, torch.ones(hid, dtype=torch.float16), 1e-5)
        R.linear(h, w["qkv"])
        R.linear(h, w["o"])
        a = R.linear(h, w["gu"])
        R.linear(R.silu_mul(a[:, :I], a[:, I:]), w["d"])

    scale = R.softmax_scale_for(D)
    qt, qr = torch.randn(q_t, H, D).half(), torch.randn(q_r, H, D).half()
    gemms(q_r)                                                        # warm the CPU GEMM path
    t_attn_full = tm(lambda: R.attn_kvcache(qt, kv, kv, scale))
    t_attn_retr = tm(lambda: R.attn_kvcache(qr, kv[:Rb], kv[:Rb], scale))
    t_gemm_t, t_gemm_r = tm(lambda: gemms(q_t)), tm(lambda: gemms(q_r))
    t_head = tm(lambda: R.norm_logits(R.linear(torch.randn(q_r, hid).half(), w["head"]).float(), args.temp, -1, args.top_p))
    # draft forward (2 layers, hidden 768) ~ 87 MB of weights: time the lm_head-sized part + layers
    dw = (torch.empty(dcfg.vocab_size, dcfg.hidden_size, dtype=torch.float16).normal_() * 0.02)
    t_draft = tm(lambda: R.linear(torch.randn(4, dcfg.hidden_size).half(), dw)) * (87.0 / 49.0)
    target_fwd = L * (t_attn_full + t_gemm_t) + t_head
    retr_fwd = L * (t_attn_retr + t_gemm_r) + t_head
    step = target_fwd + inner_per_step * retr_fwd + (inner_per_step + 1) * t_draft
    return {"value": round(tokens_per_step / step, 4), "unit": "tokens/s", "cores": torch.get_num_threads(),
            "kind": "port",
            "sample": (f"oracle (torch CPU) timed for 1 of {L} target layers at full shape (attention q={q_t} x S={S} "
                       f"keys + the 4 GEMMs), lm_head+top-p, 1 retrieval-verify layer (R={Rb}) and the draft GEMM; "
                       f"step = target fwd + {inner_per_step:.2f} x retrieval fwd + {inner_per_step + 1:.2f} x draft, "
                       f"extrapolated x{L} layers; {setup + t_attn_full + t_attn_retr + t_gemm_t + t_gemm_r + t_head:.1f} s "
                       f"of CPU work; est. {step:.1f} s per step"),
            "step_seconds_est": round(step, 2)}


def eager_comparator(ge, args, inner_per_step, tokens_per_step, device):
    """Same-hardware UN-TUNED comparator: the reference's algorithm as plain eager PyTorch-ROCm ops on
    this GPU — the oracle's op-by-op restatement (fp32 softmax attention where the reference calls flash-attn, which
    does not exist for this platform; F.linear; sort-based top-p) over the product's own weights and KV caches (views,
    nothing copied).  Baseline leg only: the oracle is the thing timed here, never the product path."""
    from oracle import ref_model as M
    from oracle import ref_ops as R
    eng = ge.engine

    def state_dict(W):
        hd = W.H * W.D
        sd = {"model.embed_tokens.weight": W.embed, "model.norm.weight": W.norm, "lm_head.weight": W.lm_head.w}
        for i in range(W.L):
            p = f"model.layers.{i}."
            qkv, gu = W.wqkv[i].w, W.wgu[i].w
            sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.k_proj.weight"] = qkv[:hd], qkv[hd:2 * hd]
            sd[p + "self_attn.v_proj.weight"], sd[p + "self_attn.o_proj.weight"] = qkv[2 * hd:], W.wo[i].w
            sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"] = gu[:gu.shape[0] // 2], gu[gu.shape[0] // 2:]
            sd[p + "mlp.down_proj.weight"] = W.wd[i].w
            sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = W.ln1[i], W.ln2[i]
        return sd

    def view_cache(cls, src, **attrs):
        c = object.__new__(cls)
        c.key_cache, c.value_cache = src.k.permute(0, 2, 1, 3), src.v.permute(0, 2, 1, 3)     # (L, T, H, D) views
        c.layers = src.layers
        for k, v in attrs.items():
            setattr(c, k, v)
        return c

    def timed(fn, n=2):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    gamma = args.gamma
    with torch.device(device):                               # the oracle builds its index tensors with default factories
        tcfg, dcfg = eng.model.config.to_dict(), eng.draft.config.to_dict()
        ot, od = M.OracleTarget(tcfg, state_dict(eng.model.weights)), M.OracleDraft(dcfg, state_dict(eng.draft.weights))
        S = eng.kv_cache.seq_len
        okv = view_cache(M.FullCache, eng.kv_cache, max_budget=eng.kv_cache.max_budget, seq_len=S)
        gc_ = eng.graph_cache
        ogc = view_cache(M.RetrievalCacheO, gc_, chunk_size=gc_.chunk_size, prefill=gc_.prefill, gamma=gamma,
                         chunks=gc_.chunks, select_sets=gc_.select_sets, max_budget=gc_.max_budget,
                         real_budget=gc_.real_budget, init_graph=True, last_scores=[None] * gc_.layers,
                         last_idx=[None] * gc_.layers)
        dc = eng.draft_cache
        odc = view_cache(M.StreamingCacheO, dc, gamma=gamma, start_size=dc.start_size, recent_size=dc.recent_size,
                         real_budget=dc.real_budget, seq_len=dc.start_size + dc.recent_size)
        ids = torch.full((1, gamma + 2), 100, dtype=torch.long)
        pos = torch.arange(S, S + gamma + 1).unsqueeze(0)

        def ar():
            okv.seq_len = S
            lg = ot.forward(ids[:, :1], okv, None)
            R.norm_logits(lg[0], args.temp, -1, args.top_p)

        def tv():
            okv.seq_len = S
            lg = ot.forward(ids, okv, None)
            R.norm_logits(lg[0], args.temp, -1, args.top_p)

        def rv():
            lg = ot.forward(ids[:, :gamma + 1], okv, ogc, position_ids=pos, spec=True)
            R.norm_logits(lg[0], args.temp, -1, args.top_p)

        def dr():
            lg = od.forward(ids[:, :3], odc, odc, gamma_offset=2)
            R.norm_logits(lg[0], args.temp, -1, args.top_p)

        t_ar, t_tv, t_rv, t_dr = timed(ar), timed(tv), timed(rv), timed(dr, 3)
        okv.seq_len = S
    step_ms = t_tv + inner_per_step * (t_rv + t_dr) + t_dr
    return {"what": "the reference's algorithm as plain eager PyTorch-ROCm ops (oracle restatement, fp32 softmax "
                    "attention in place of flash-attn, F.linear, sort-based top-p) on this GPU, product weights and KV "
                    "caches shared as views; stage latencies by HIP events, step composed with the measured inner count",
            "ar_step_ms": round(t_ar, 2), "ar_tokens_per_s": round(1e3 / t_ar, 2),
            "target_verify_ms": round(t_tv, 2), "retrieval_verify_ms": round(t_rv, 2), "draft_step_ms": round(t_dr, 3),
            "triforce_step_ms_est": round(step_ms, 2), "triforce_tokens_per_s_est": round(tokens_per_step / step_ms * 1e3, 2)}


def baseline_config_label(target, prefill, budget, gamma, on_chip, layers, world):
    """Which BASELINE.json config the PARAMETERS of this run are (the label on the JSON line must name what ran)."""
    offload = 0 <= on_chip < layers
    if (prefill, budget, gamma) == (124928, 4096, 6) and not offload:
        if target == "llama-7B-128K":
            return "BASELINE configs[1]" + ("" if world == 1 else f" shapes sharded TP={world}")
        if target == "lwm-128K":
            return "BASELINE configs[2]" + ("" if world == 1 else f" shapes sharded TP={world}")
    if (prefill, budget, gamma) == (130048, 12288, 16):
        if target == "llama-7B-128K":
            return "BASELINE configs[3]" + (" (offloading_TP, TP=2)" if world == 2 else
                                            f" parameters at world size {world}" + (" (offloading tier)" if offload else ""))
        if target == "llama-13B-128K":
            return "BASELINE configs[4]" + ("" if world == 8 else f" parameters at world size {world}")
    return "custom (not a BASELINE.json config)"


def forward_bytes(tcfg, keys, world=1):
    """Algorithmic HBM bytes of ONE decode-sized forward of this rank: every layer's weight shard once
    + the K and V rows it attends over + the replicated lm_head."""
    hid, I, L, V = tcfg.hidden_size, tcfg.intermediate_size, tcfg.num_hidden_layers, tcfg.vocab_size
    H, D = tcfg.num_attention_heads // world, tcfg.head_dim
    w_layer = (3 * H * D * hid + H * D * hid + 3 * (I // world) * hid) * 2
    kv_layer = 2 * keys * H * D * 2
    return L * (w_layer + kv_layer) + V * hid * 2, w_layer, kv_layer


def _stage_row(stage, byts, us, how):
    gbps = byts / (us * 1e-6) / 1e9
    return {"stage": stage, "bound": "hbm", "algorithmic_bytes": int(byts), "us": round(us, 1), "achieved": round(gbps, 1),
            "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(gbps / HBM_PEAK_GBPS, 4), "measured": how}


def retrieval_build_rooflines(ge, args, device):
    """Chunk scoring / top-k / gather of ONE layer's retrieval build at the run's shapes, each kernel timed with HIP
    events on the launch stream over different layers of the real KV cache (cold L2 / Infinity Cache) — north_star's
    'achieved HBM GB/s on the retrieval gather'."""
    from triforce_amd import ops
    eng = ge.engine
    kv, gc = eng.kv_cache, eng.graph_cache
    H, D = kv.num_heads, kv.head_dim
    L = kv.layers
    q = torch.randn(H, D, device=device, dtype=torch.float16)
    chunks, chunk, sets = gc.chunks, gc.chunk_size, gc.select_sets
    lay = [0]

    def nxt():
        lay[0] = (lay[0] + 5) % L
        return kv.layer_kv(lay[0])

    scores = ops.retrieval_score(nxt()[0], q, chunks, chunk)
    idx = ops.retrieval_topk(scores, sets)
    dk, dv = torch.empty(H, sets * chunk, D, device=device, dtype=torch.float16), \
        torch.empty(H, sets * chunk, D, device=device, dtype=torch.float16)
    t_score = _timed(lambda: ops.retrieval_score(nxt()[0], q, chunks, chunk), 6)
    t_topk = _timed(lambda: ops.retrieval_topk(scores, sets), 6)

    def gather():
        kl, vl = nxt()
        ops.retrieval_gather(kl, vl, idx, dk, dv, chunk)
    t_gather = _timed(gather, 6)
    P = chunks * chunk
    rows = [_stage_row("retrieval_score (chunk means + q.k per chunk, one layer)", P * H * D * 2, t_score, "HIP events, 6 launches over distinct layers"),
            _stage_row("retrieval_gather (selected chunks K and V -> retrieval cache, one layer)", 4 * sets * chunk * H * D * 2,
                       t_gather, "HIP events, 6 launches over distinct layers")]
    rows.append({"stage": "retrieval_topk (radix select per head, one layer)", "bound": "latency", "us": round(t_topk, 1),
                 "measured": "HIP events, 6 launches"})
    return rows


def pmc_layer_traffic(tcfg, slots, rows):
    """HBM traffic / algorithmic bytes of every kernel of one retrieval-verify decoder layer from the committed
    rocprofv3 --pmc passes over tools/pmc_layer.py (same counters and corrections as pmc_traffic), when that file was
    measured at this run's widths; else None."""
    import glob
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_retrieval_verify_layer*.json")), reverse=True):
        try:
            j = json.load(open(f))
            sh = j["shape"]
            if (sh["hidden"], sh["inter"], sh["heads"], sh["head_dim"], sh["slots"], sh["rows"]) == \
                    (tcfg.hidden_size, tcfg.intermediate_size, tcfg.num_attention_heads, tcfg.head_dim, slots, rows):
                return {"traffic_over_algorithmic": {k["kernel"]: k["traffic_over_algorithmic"] for k in j["kernels"]},
                        "traffic_source": os.path.relpath(f, ROOT)}
        except Exception:
            continue
    return None


def pmc_traffic(alg_bytes, H, D):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 --pmc passes (FETCH_SIZE and
    WRITE_SIZE collected in separate runs, KiB units, FETCH_SIZE doubled for gfx950 — MI355X_MICROARCH.md §HBM).
    PMC counters cannot be read from inside this process; the latest profiles/*pmc_attn*.json is used when it
    was measured on the same shape (H, D, key count within 0.1%), else traffic stays null."""
    import glob
    import re

    def order(path):        # r03a < r03b < ... < r03 (the un-suffixed file is the final measurement of a round)
        m = re.match(r"r(\d+)([a-z]?)_", os.path.basename(path))
        return (int(m.group(1)), m.group(2) or "~") if m else (-1, "")
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_attn*.json")), key=order):
        try:
            j = json.load(open(f))
        except Exception:
            continue
        sh = j.get("shape", {})
        if sh.get("H") == H and sh.get("D") == D and abs(j["algorithmic_bytes_per_launch"] / alg_bytes - 1) < 1e-3:
            best = (f, j)
    if best is None:
        return {"traffic": None}
    f, j = best
    return {"traffic": j["traffic_bytes_per_launch"], "traffic_unit": "bytes/launch",
            "traffic_source": os.path.relpath(f, ROOT), "traffic_measured_on": j.get("measured_on"),
            "traffic_over_algorithmic": j["traffic_over_algorithmic"]}


def attn_roofline(timer, retrieval_rows, H, D):
    """Live roofline of the dominant kernel — target-verify attention over the full KV (the sampled launches with
    more keys than the retrieval cache holds).  H = heads on THIS rank.  HIP events on the launch stream."""
    from triforce_amd import ops
    full = [(a.elapsed_time(b) * 1e-3, sk) for (a, b, sk, _, _) in (timer or []) if sk > retrieval_rows]
    if not full:
        return None
    dur = sum(d for d, _ in full) / len(full)
    byts = sum(2 * sk * H * D * 2 for _, sk in full) / len(full)
    achieved = byts / dur / 1e9
    roof = {"bound": "hbm", "kernel": "attn_split_kernel<128,1> / attn_split_q2_kernel<128> above 16 rows (split merge inside "
                                      "the launch) via tf_attn_decode_fused",
            "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": None,
            "launches": len(full), "launches_sampled_every": ops.ATTN_TIMER_EVERY,
            "avg_launch_us": round(dur * 1e6, 1), "algorithmic_bytes_per_launch": int(byts)}
    roof.update(pmc_traffic(byts, H, D))
    return roof


def block_stats(stamps, blocks=10):
    """mean / stdev of ms per step over `blocks` equal blocks of the timed steps (host stamps behind each step's record read):
    what a sub-1 % claim has to be read against.  None below 2 steps per block."""
    n = len(stamps) - 1
    if n < 2 * blocks:
        return None
    per = n // blocks
    ms = [(stamps[(b + 1) * per] - stamps[b * per]) / per * 1e3 for b in range(blocks)]
    mean = sum(ms) / blocks
    sd = (sum((x - mean) ** 2 for x in ms) / (blocks - 1)) ** 0.5
    return {"blocks": blocks, "steps_per_block": per, "mean": round(mean, 3), "stdev": round(sd, 3), "min": round(min(ms), 3),
            "max": round(max(ms), 3), "rel_stdev": round(sd / mean, 5)}


def operating_points(label_cfg):
    """Other points of the acceptance dial, from the newest committed sweep of this workload (tools/acceptance_sweep.py: one
    prefill, nine (draft, retrieval) acceptance settings): three of them ride in the line beside the configured one."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*acceptance_sweep*.json")))
    for f in reversed(files):
        try:
            j = json.load(open(f))
            pts = j["points"]
        except Exception:
            continue
        want = [(0.5, 0.8), (0.7, 0.9), (0.9, 0.95), (0.9, 0.96)]
        pick = [p for p in pts if (p.get("requested_draft_acc"), p.get("requested_retrieval_acc")) in want]
        if not pick:
            continue
        keys = ("requested_draft_acc", "requested_retrieval_acc", "tokens_per_s", "tokens_per_step", "ms_per_step", "avg_accepted_len",
                "per_token_acceptance_target", "per_token_acceptance_middle", "inner_iterations_per_step")
        return {"source": os.path.relpath(f, ROOT), "measured_on": j.get("measured_on"), "workload": j.get("workload", label_cfg),
                "points": [{k: p[k] for k in keys if k in p} for p in pick]}
    return None


def timed_steps(run, steps, eager_every=0, sample_attn=False):
    """Exactly ``steps`` outer iterations bracketed by device syncs -> dict of counters over the timed region.
    eager_every = N > 0: every N-th target verify runs eagerly (instead of its hipGraph) so that its attention launches
    can be bracketed with HIP events; sample_attn switches the event sampling of eager attention launches on."""
    from triforce_amd import ops
    n0, acc0, dr0, in0 = run.n, run.accepted_count, run.draft_count, run.inner_iters
    rs0, mid0 = run.resample_count, len(run.acc_rate_middle_list)
    run.eager_every = eager_every
    ops.ATTN_TIMER = [] if sample_attn else None
    torch.cuda.synchronize()
    t1 = time.time()
    stamps = [t1]
    last = 0
    for _ in range(steps):
        last = run.step()
        stamps.append(time.time())       # (host clock behind the step's record read: no extra device sync)
    torch.cuda.synchronize()
    t2 = time.time()
    stamps[-1] = t2
    timer, ops.ATTN_TIMER = ops.ATTN_TIMER, None
    run.eager_every = 0
    accepted, drafted = run.accepted_count - acc0, run.draft_count - dr0
    tests = accepted + (run.resample_count - rs0)           # accept tests the target ran (one per examined token)
    mids = run.acc_rate_middle_list[mid0:]
    inner = run.inner_iters - in0
    return dict(seconds=t2 - t1, tokens=run.n - n0, accepted=accepted, drafted=drafted, inner=inner, timer=timer, stamps=stamps,
                per_token_acceptance=accepted / max(tests, 1),
                middle_acceptance=sum(mids) / max(len(mids), 1),
                last_tokens=run.emitted[len(run.emitted) - last:])      # what the last step emitted (step() returns the count)


class VerifyCapture:
    """--dump-outputs: keeps a reference to the probabilities of the latest target verify, whichever of its three forms
    TriForceRunner.step issues (in-place hipGraph replay, ids-as-arguments replay, verify_probs).  Instance attributes
    shadow the engine's methods until remove(); nothing is copied or synchronised inside them."""

    def __init__(self, ge):
        self.probs, self.patched = None, []
        self._wrap(ge, "verify_probs", lambda out: out)
        self._wrap(ge, "verify_probs_ids", lambda out: out[0])
        for tg in ge.target_graphs.values():
            self._wrap(tg, "replay_in_place", lambda out: out)

    def _wrap(self, obj, name, pick):
        fn = getattr(obj, name, None)
        if fn is None:
            return

        def wrapped(*a, **k):
            out = fn(*a, **k)
            if out is not None:
                self.probs = pick(out)
            return out
        setattr(obj, name, wrapped)
        self.patched.append((obj, name))

    def remove(self):
        for obj, name in self.patched:
            delattr(obj, name)
        self.patched = []


def write_outputs(out_dir, tokens, probs):
    """DIR/tokens.npy (float64) and DIR/verify_probs.npy (float32, rows x vocab): about 1 MB for the 7B workload."""
    import numpy as np
    if probs is None:
        raise RuntimeError("--dump-outputs: no target verify was seen in the timed steps")
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"tokens": np.asarray(tokens, dtype=np.float64),
              "verify_probs": probs.detach().float().reshape(-1, probs.shape[-1]).cpu().numpy()}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}


def self_launch(args):
    """``python bench.py --gpus N`` without a launcher: re-execute under torch.distributed.run, one rank per GPU
    (the reference's own launch line: torchrun --nproc_per_node=N test/offloading_TP.py, README.md:62)."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: required for RCCL / P2P buffers on this driver
    return subprocess.call(cmd, env=env)


def full_measurements(result, args, ge, run, m, label, target, draft, kind, input_ids, new_runner, device):
    """--full: everything beyond the headline, measured after the timed steps in this order (each one in runs of its
    own): stage latencies + stage rooflines, the autoregressive baseline, the committed acceptance-sweep points, the
    step overhead, the eager comparator (--eager-comparator), the random-weight run and the CPU baseline."""
    tcfg, dcfg = target_config(args.target)
    seconds, tokens = m["seconds"], m["tokens"]
    value = tokens / seconds
    inner_per_step = m["inner"] / max(args.steps, 1)
    stages = stage_latencies(ge, args, device)
    S_now = ge.engine.kv_cache.seq_len
    rv_bytes, w_layer, rv_kv = forward_bytes(tcfg, args.budget + args.gamma + 1)
    tv_bytes, _, tv_kv = forward_bytes(tcfg, S_now + args.gamma + 2)
    d_bytes = (dcfg.num_hidden_layers * (4 * dcfg.hidden_size ** 2 + 3 * dcfg.intermediate_size * dcfg.hidden_size)
               + dcfg.vocab_size * dcfg.hidden_size) * 2
    how = "HIP events around hipGraph replays on the launch stream (stage_latency_us)"
    roofline_stages = [
        _stage_row(f"retrieval_verify forward ({args.gamma + 1} rows: {tcfg.num_hidden_layers} x ({w_layer / 1e6:.1f} MB weights + "
                   f"{rv_kv / 1e6:.1f} MB retrieval KV) + lm_head)", rv_bytes, stages["retrieval_verify_us"], how),
        _stage_row(f"target_verify forward ({args.gamma + 2} rows: {tcfg.num_hidden_layers} x ({w_layer / 1e6:.1f} MB weights + "
                   f"{tv_kv / 1e6:.1f} MB KV) + lm_head)", tv_bytes, stages["target_verify_us"], how),
        _stage_row("draft step (68M forward, weights once)", d_bytes, stages["draft_step_us"], how)]
    layer_pmc = pmc_layer_traffic(tcfg, ge.engine.graph_cache.real_budget, args.gamma + 1)
    if layer_pmc:                                                  # per-kernel PMC traffic of that stage's layer
        roofline_stages[0].update(layer_pmc)
    try:
        roofline_stages += retrieval_build_rooflines(ge, args, device)
    except Exception as ex:                                        # a probe must never cost the bench line
        roofline_stages.append({"stage": "retrieval build", "failed": f"{type(ex).__name__}: {ex}"[:300]})
    ar_tps = autoregressive_baseline(ge, args, run.next_token)
    result.update({
        "stage_latency_us": stages,
        "ar_baseline_tokens_per_s": round(ar_tps, 2),
        "speedup_vs_autoregressive": round(value / ar_tps, 3),
        "reference_speedup_vs_autoregressive": {"value": REFERENCE_SPEEDUP, "hardware": "1x A100, trained weights",
                                                "source": "reference README.md:49-55"},
        "roofline_stages": roofline_stages,
    })
    if kind == "aligned":
        op = operating_points(label)
        if op is not None:
            result["operating_points"] = op
    # what a step costs beyond its model calls (accept kernels, cache fix-ups, host round trips); the eager verifies
    # sampled for the roofline are priced at their own latency
    n_eager = (args.steps // args.roofline_every) if (args.roofline_every > 0 and not args.no_graphs) else 0
    tv_mean = (stages["target_verify_us"] * (args.steps - n_eager) + stages["target_verify_eager_us"] * n_eager) / max(args.steps, 1)
    modelled = tv_mean + inner_per_step * (stages["retrieval_verify_us"] + stages["draft_step_us"]) + stages["draft_step_us"]
    result["step_overhead_us"] = round(max(0.0, seconds / args.steps * 1e6 - modelled), 1)

    if args.eager_comparator:
        try:
            result["eager_torch_comparator"] = eager_comparator(ge, args, inner_per_step, tokens / args.steps, device)
            e = result["eager_torch_comparator"]
            e["product_speedup_vs_eager_triforce"] = round(value / e["triforce_tokens_per_s_est"], 2)
            e["product_ar_speedup_vs_eager_ar"] = round(ar_tps / e["ar_tokens_per_s"], 2)
        except Exception as ex:
            result["eager_torch_comparator"] = {"failed": f"{type(ex).__name__}: {ex}"[:400]}
        torch.cuda.empty_cache()
    if args.random_steps > 0 and kind != "random":
        # the round-1 regime, same process, same graphs: weights re-drawn IN PLACE as N(0, 0.02), prompt re-prefilled
        target.weights.overwrite_random_(args.seed + 1)
        draft.weights.overwrite_random_(args.seed + 2)
        run2 = new_runner(args.seed + 7)
        do_prefill(run2, ge, input_ids, args.prefill_mode)
        for _ in range(2):
            run2.step()
        r = timed_steps(run2, args.random_steps)
        result["random_weights"] = {
            "tokens_per_s": round(r["tokens"] / r["seconds"], 3), "steps": args.random_steps,
            "ms_per_step": round(r["seconds"] / args.random_steps * 1e3, 3),
            "acceptance_rate": round(r["accepted"] / max(r["drafted"], 1), 4),
            "tokens_per_step": round(r["tokens"] / args.random_steps, 3),
            "inner_iterations_per_step": round(r["inner"] / args.random_steps, 3),
            "note": "random-init N(0,0.02) weights: draft and target disagree on ~every token (worst case of the loop)"}
    if not args.no_cpu_baseline:
        try:
            result["cpu_baseline"] = cpu_baseline(args, tokens / args.steps, inner_per_step)
        except Exception as ex:                                    # host too small for the sample: report, don't fake
            result["cpu_baseline"] = {"value": None, "unit": "tokens/s", "cores": torch.get_num_threads(),
                                      "kind": "port", "sample": f"failed: {type(ex).__name__}: {ex}"}


def main():
    args = parse()
    if args.dump_outputs and (args.gpus > 1 or args.engine == "tp" or args.on_chip >= 0
                              or os.environ.get("TRIFORCE_BENCH_FORCE_TP") == "1"):
        raise SystemExit("--dump-outputs: single-GPU engine only (--gpus 1, no --engine tp / --on-chip)")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus}")
    if world > 1 or args.engine == "tp" or args.on_chip >= 0 or os.environ.get("TRIFORCE_BENCH_FORCE_TP") == "1":
        from bench_tp import run_tp                  # tensor-parallel decode (heads sharded, RCCL all-reduce)
        return run_tp(args, rank, world, local)
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)

    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.sampling import UniformSource

    t_setup = time.time()
    kind, tspec, dspec, wlabel = resolve_weights(args)
    target, draft = load_models(args, device, kind, tspec, dspec)
    ge = build_engine(args, device, target, draft)
    tcfg, _ = target_config(args.target)
    gen = torch.Generator().manual_seed(args.seed)
    input_ids = torch.randint(3, tcfg.vocab_size, (1, args.prefill), generator=gen).to(device)

    def new_runner(seed):
        return TriForceRunner(_Tok(), ge, args.gamma, top_k=-1, top_p=args.top_p, temperature=args.temp,
                              rng=UniformSource(device, seed=seed), rebuild_every=args.rebuild_every)

    run = new_runner(args.seed)
    torch.cuda.synchronize()
    t0 = time.time()
    do_prefill(run, ge, input_ids, args.prefill_mode)
    torch.cuda.synchronize()
    t_prefill = time.time() - t0

    for _ in range(args.warmup):
        run.step()
    capture = VerifyCapture(ge) if args.dump_outputs else None
    # graphs: every --roofline-every-th verify is eager and sampled; --no-graphs: every verify is eager already
    m = timed_steps(run, args.steps, 0 if args.no_graphs else args.roofline_every,
                    sample_attn=args.no_graphs or args.roofline_every > 0)
    if capture is not None:
        capture.remove()
        write_outputs(args.dump_outputs, m["last_tokens"], capture.probs)
    seconds, tokens = m["seconds"], m["tokens"]
    value = tokens / seconds
    roof = attn_roofline(m["timer"], args.budget + args.gamma + 1, tcfg.num_attention_heads, tcfg.head_dim)

    label = baseline_config_label(args.target, args.prefill, args.budget, args.gamma, -1, tcfg.num_hidden_layers, 1)
    inner_per_step = m["inner"] / max(args.steps, 1)
    cal = (target.weights.aligned or {}).get("calibration") if kind == "aligned" else None
    result = {
        "metric": metric_label(args.target, args.prefill),
        "value": round(value, 3), "unit": "tokens/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(seconds / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "f16", "data": "synthetic",
        "config": {"workload": f"{label}: {tcfg._name_or_path} on-chip TriForce decode, prefill "
                               f"{args.prefill}, budget {args.budget}, chunk {args.chunk_size}, gamma {args.gamma}, "
                               f"T={args.temp}, top_p={args.top_p}, 1xMI355X",
                   "prefill_mode": args.prefill_mode, "weights": wlabel, "weights_kind": kind,
                   "hipgraphs": not args.no_graphs, "target_verify_graph": bool(ge.target_graphs),
                   "retrieval_rebuild_every": args.rebuild_every},
        "avg_accepted_len": round(m["accepted"] / max(m["drafted"], 1) * args.gamma, 4),
        "acceptance_rate": round(m["accepted"] / max(m["drafted"], 1), 4),
        "per_token_acceptance_target": round(m["per_token_acceptance"], 4),
        "per_token_acceptance_middle": round(m["middle_acceptance"], 4),
        "tokens": tokens, "tokens_per_step": round(tokens / args.steps, 3),
        "drafted_per_step": round(m["drafted"] / max(args.steps, 1), 3),
        "inner_iterations_per_step": round(inner_per_step, 3),
        "prefill_seconds": round(t_prefill, 2), "setup_seconds": round(t0 - t_setup, 2),
        "kv_seq_len": ge.engine.kv_cache.seq_len,
        "roofline": roof, "full": args.full,
    }
    bs = block_stats(m["stamps"])
    if bs is not None:
        result["ms_per_step_blocks"] = bs
    dp = getattr(draft, "_persist", None)
    result["draft_forward"] = {
        "form": "one launch: tf_draft_forward_68m_persist, 256 co-resident workgroups, arrival counters + READY flags"
                if dp is not None else "13-launch chain: tf_draft_forward_68m",
        "error_word": dp.error() if dp is not None else None,
        "draft_step_us_is": "the hipGraph replay the loop issues (shared token buffer); draft_step_with_io_us adds the input "
                            "copy and the output clone of graph_draft_inference (what rounds 1-5 quoted as draft_step_us)"}
    if kind == "aligned":
        # the headline is CONDITIONAL on a dial: say so next to it (trained checkpoints are not available offline)
        result["value_note"] = (f"configured-acceptance scenario: synthetic weights {wlabel} SET the draft->retrieval and "
                                "retrieval->target acceptance rates (models/aligned.py); tokens/s and avg_accepted_len follow "
                                "from that dial — stage_latency_us, roofline* and random_weights do not depend on it; other "
                                "operating points: `operating_points` with --full (newest profiles/*acceptance_sweep*.json); "
                                "not comparable to the reference's trained-weights 2.2x")
    elif kind == "random":
        result["value_note"] = "random-init weights: acceptance ~0, the loop's worst case (gamma inner iterations per token)"
    if cal is not None:
        result["aligned_calibration"] = cal
    if args.full:
        full_measurements(result, args, ge, run, m, label, target, draft, kind, input_ids, new_runner, device)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
