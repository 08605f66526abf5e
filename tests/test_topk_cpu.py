"""Top-k on the target tier, the parts that need no GPU: the C ABI of tf_topk_topp_probs, the torch
fallback of norm_logits that CPU tensors keep, and the host routing of ``top_k`` through GraphInferenceEngine and the decode
loop on the CPU backend (cpu_ops).  The kernel itself is checked in tests/test_gpu_topk.py."""
import ctypes
import os
import re

import pytest
import torch

from oracle import ref_ops as R
from tests import helpers as Hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP_TOL = 8e-3        # as tests/test_gpu_e2e.py: an emitted token may trail the target's argmax by ~2 fp16 spacings


def test_symbol_is_declared_bound_exported_and_rejects_null_arguments():
    from triforce_amd import hip
    src = open(os.path.join(ROOT, "include", "triforce_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+tf_topk_topp_probs\s*\(", decl), "include/triforce_hip.h does not declare tf_topk_topp_probs"
    assert "tf_topk_topp_probs" in hip.SIGNATURES
    lib = hip.lib()
    assert hasattr(lib, "tf_topk_topp_probs"), "libtriforce_hip.so does not export tf_topk_topp_probs"
    null = ctypes.c_void_p(0)
    assert lib.tf_topk_topp_probs(null, null, 8, 32000, 0.6, 50, 0.9, null) == -22
    # every other argument check comes before any launch too (no device is touched: this runs without one)
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for rows, V, T, k, P in [(0, 8, 0.6, 2, 0.9), (1, 0, 0.6, 2, 0.9), (1, 8, 0.0, 2, 0.9), (1, 8, float("nan"), 2, 0.9),
                             (1, 8, 0.6, 0, 0.9), (1, 8, 0.6, -1, 0.9), (1, 8, 0.6, 2, 0.0), (1, 8, 0.6, 2, float("nan"))]:
        assert lib.tf_topk_topp_probs(p, p, rows, V, T, k, P, null) == -22, (rows, V, T, k, P)
    assert lib.tf_topk_topp_probs(p, p, 1, 32769, 0.6, 2, 0.9, null) == -34


@pytest.mark.parametrize("T,P", [(0.6, 0.9), (1.0, 1.0), (1.0, 1e-9)])
def test_norm_logits_cpu_fallback_equals_the_oracle(T, P):
    """CPU tensors keep the torch restatement (topk + stable sort): exactly the oracle's norm_logits, ties at the k-th value
    included."""
    from triforce_amd.utils.sampling import norm_logits
    V = 96
    gen = torch.Generator().manual_seed(7)
    lg = torch.randn(5, V, generator=gen) * 2.5
    lg[1] = lg[1].half().float()
    lg[2, 10:16] = lg[2].sort(descending=True).values[4]        # six equal values straddling rank 5
    lg[3] = 0.0
    for k in (1, 5, V, V + 3):
        got = norm_logits(lg.clone(), temperature=T, top_k=k, top_p=P)
        want = R.norm_logits(lg.clone(), T, k, P)
        assert torch.equal(got, want), (k, T, P)


def test_top_k_1_on_the_target_tier_emits_the_greedy_stream(cpu_ops):
    """An engine built with ``top_k=1`` and TriForce(top_k=1, temperature=1, top_p=1): the target's distribution is one-hot up to
    exact logit ties while both draft tiers keep sampling at temperature 1 WITHOUT top-k (as in the reference), so whatever
    they propose, speculative sampling must emit the target's greedy stream.  Stated as tests/test_session_cpu.py states it
    (exact fp16 ties between the 1-row and the 7-row forward): every teacher-forced gap within GAP_TOL, at most 2 non-zero."""
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache, StreamingLLMEvictionCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as LlamaForCausalLM_68M
    from triforce_amd.utils.decoding import TriForce, TriForceRunner
    from triforce_amd.utils.graph_infer import GraphInferenceEngine
    from triforce_amd.utils.sampling import Filters, UniformSource
    from oracle import specs
    g = Hh.load_golden("small_gamma6")
    gamma = g["gamma"]
    tsd = specs.random_state_dict(g["tcfg"], g["tseed"], head_std=g.get("head_std", 0.05))
    dsd = specs.random_state_dict(g["dcfg"], g["dseed"], head_std=g.get("head_std", 0.05))
    target = LlamaForCausalLM.from_state_dict(LlamaConfig.from_dict(g["tcfg"]), tsd, "cpu")
    draft = LlamaForCausalLM_68M.from_state_dict(LlamaConfig.from_dict(g["dcfg"]), dsd, "cpu")
    ge = GraphInferenceEngine(target, FlashSimpleCache(target, g["prefill"] + g["gen_len"] + 16),
                              RetrievalCache(target, max_budget=g["budget"], prefill=g["prefill"], gamma=gamma, chunk_size=g["chunk"]),
                              draft, StreamingLLMEvictionCache(draft, start_size=16, recent_size=256 - 16 - gamma, gamma=gamma))
    assert ge.target_filters.top_k == -1
    ge.initialize_eager(gamma, probs=True, temperature=1.0, top_p=1.0, top_k=1)
    assert ge.target_filters.top_k == 1 and "top_k" not in ge.sampling            # the draft tiers' capture arguments never see it
    res = TriForce(Hh.FakeTokenizer(), ge, Hh.prompt_of(g), gamma=gamma, max_len=g["gen_len"], top_k=1, top_p=1.0, temperature=1.0,
                   rng=UniformSource("cpu", values=Hh.fixed_uniforms(seed=41)), return_details=True)
    gaps = Hh.teacher_forced_gaps(g, res["tokens"], tsd, dsd)
    print(f"teacher-forced gaps: max {max(gaps):.5f}, {sum(1 for x in gaps if x > 0.0)} of {len(gaps)} not the argmax; "
          f"acceptance {res['acceptance_rate']:.3f}, resampled {res['resampled']}")
    assert max(gaps) <= GAP_TOL, f"token {gaps.index(max(gaps))} trails the target's argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x != 0.0) <= 2
    assert res["resampled"] > 0                                    # the drafts did propose something else, and it was corrected
    # the routing rule: the engine's captured top-k must equal the runner's (any value <= 0 counts as -1)
    for runner_k, engine_k, match in [(1, 1, True), (-1, 1, False), (1, -1, False), (0, -1, True), (-1, 0, True), (20, 50, False)]:
        ge.initialize_eager(gamma, probs=True, temperature=1.0, top_p=1.0, top_k=engine_k)
        run = TriForceRunner(Hh.FakeTokenizer(), ge, gamma, top_k=runner_k, top_p=1.0, temperature=1.0)
        assert run._served() is match, (runner_k, engine_k)
        assert ge.serves(Filters(1.0, 1.0, runner_k)) is match
