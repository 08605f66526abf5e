"""Vocabularies above 32 768, the parts that need no GPU: the C ABI and every argument gate of
tf_topp_probs_large / tf_topk_topp_probs_large, the routing of norm_logits between the fused kernels, their _large forms and the
torch restatement, the model shapes, and the decode loop on the CPU backend at V = 40 000.  The kernels themselves are checked
in tests/test_gpu_large_vocab.py."""
import copy
import ctypes
import os
import re

import pytest
import torch

from oracle import ref_ops as R
from tests import helpers as Hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP_TOL = 8e-3        # as tests/test_topk_cpu.py: an emitted token may trail the target's argmax by ~2 fp16 spacings
EINVAL, ENOSPC, ERANGE = -22, -28, -34


def _ws_bytes(rows, V):
    return rows * (((V + 4095) >> 12) * 4096 * 2) * 4


def test_entry_points_are_declared_bound_exported_and_gate_every_argument_before_launching():
    from triforce_amd import hip, ops
    src = open(os.path.join(ROOT, "include", "triforce_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = hip.lib()
    for name in ("tf_topp_probs_large", "tf_topk_topp_probs_large"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", decl), f"include/triforce_hip.h does not declare {name}"
        assert name in hip.SIGNATURES
        assert hasattr(lib, name), f"libtriforce_hip.so does not export {name}"
    # the workspace size is a header macro; ops restates it
    m = re.search(r"#define\s+TF_TOPP_LARGE_WS_BYTES\(rows, V\)\s+(.*)", decl)
    assert m and "4095" in m.group(1) and "4096 * 2" in m.group(1)
    assert re.search(r"#define\s+TF_TOPP_LARGE_MAX_VOCAB\s+262144\b", decl)
    for rows, V in [(1, 1), (1, 4096), (1, 4097), (8, 128256), (32, 262144)]:
        assert ops.topp_large_ws_bytes(rows, V) == _ws_bytes(rows, V)
    assert ops.TOPP_LARGE_MAX_VOCAB == 262144 and ops.TOPP_MAX_VOCAB == 32768

    # no device is touched below: host buffers stand in for device pointers, every call must return before any launch
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    aligned = ctypes.c_void_p((p.value + 15) & ~15)
    null = ctypes.c_void_p(0)
    big = 1 << 40

    def topp(lg=aligned, pr=aligned, rows=1, V=8, T=0.6, P=0.9, ws=aligned, nb=big):
        return lib.tf_topp_probs_large(lg, pr, rows, V, T, P, ws, nb, null)

    def topk(lg=aligned, pr=aligned, rows=1, V=8, T=0.6, k=2, P=0.9, ws=aligned, nb=big):
        return lib.tf_topk_topp_probs_large(lg, pr, rows, V, T, k, P, ws, nb, null)

    nan = float("nan")
    for fn in (topp, topk):
        for kw in (dict(lg=null), dict(pr=null), dict(ws=null), dict(rows=0), dict(rows=-1), dict(rows=33), dict(V=0), dict(V=-5),
                   dict(T=0.0), dict(T=-1.0), dict(T=nan), dict(P=0.0), dict(P=-0.5), dict(P=nan),
                   dict(ws=ctypes.c_void_p(aligned.value + 4))):
            assert fn(**kw) == EINVAL, (fn.__name__, kw)
        assert fn(V=262145) == ERANGE and fn(V=262145, nb=0) == ERANGE and fn(V=1 << 30) == ERANGE
        for rows, V in [(1, 8), (1, 32769), (7, 128256), (32, 262144)]:
            assert fn(rows=rows, V=V, nb=_ws_bytes(rows, V) - 1) == ENOSPC, (fn.__name__, rows, V)
            assert fn(rows=rows, V=V, nb=0) == ENOSPC
        # EINVAL outranks the size gates
        assert fn(V=262145, T=0.0) == EINVAL and fn(rows=0, nb=0) == EINVAL
    for k in (0, -1):
        assert topk(k=k) == EINVAL and topk(k=k, V=262145) == EINVAL
    # the existing entry points keep their limit
    assert lib.tf_topp_probs(aligned, aligned, 1, 32769, 0.6, 0.9, null) == ERANGE
    assert lib.tf_topk_topp_probs(aligned, aligned, 1, 32769, 0.6, 2, 0.9, null) == ERANGE


def test_native_draft_workspace_grows_only_above_the_old_limit():
    from triforce_amd import hip
    lib = hip.lib()
    m = hip.TfDraftModel()
    m.layers, m.hidden, m.heads, m.head_dim, m.inter, m.vocab = 2, 768, 12, 64, 3072, 32000
    base = lib.tf_draft_forward_ws_bytes(ctypes.byref(m), 7)
    m.vocab = 32768
    assert lib.tf_draft_forward_ws_bytes(ctypes.byref(m), 7) == base
    m.vocab = 128256
    assert lib.tf_draft_forward_ws_bytes(ctypes.byref(m), 7) == base + _ws_bytes(1, 128256)
    assert lib.tf_draft_persist_supported(ctypes.byref(m), 1, 100) != 0          # the one-launch form keeps refusing it
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    c = hip.TfDraftCache()
    # a workspace sized for the old layout is refused before anything launches
    assert lib.tf_draft_forward_68m(ctypes.byref(m), ctypes.byref(c), p, 7, 0, 7, p, p, 0.6, 0.9, p, base, null) == ENOSPC


def test_routing_predicate_picks_fused_large_or_torch():
    from triforce_amd import ops
    f32 = torch.float32
    assert ops.topp_route(32768, 0.9) == "fused"
    assert ops.topp_route(32769, 0.9) == "large"
    assert ops.topp_route(262144, 0.9) == "large"
    assert ops.topp_route(262145, 0.9) == "torch"
    assert ops.topp_route(64, 1.0) == "fused" and ops.topp_route(128256, 1e-9) == "large"
    for V in (32768, 32769, 262144, 262145):
        assert ops.topp_route(V, 0.0) == "torch" and ops.topp_route(V, -1.0) == "torch"
        assert ops.topp_route(V, 0.9, is_device=False) == "torch"
        assert ops.topp_route(V, 0.9, dtype=torch.float16) == "torch"
    assert ops.topp_route(40000, 0.9, True, f32) == "large"


def test_per_device_state_is_keyed_by_the_resolved_device_index(monkeypatch):
    """The control block of tf_topp_probs_multi and the workspace of the _large forms are kept per device under one key: a
    tensor on plain "cuda" belongs to the current device, not to device 0."""
    from triforce_amd import ops
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 1)
    assert ops._device_key("cuda") == ops._device_key("cuda:1") == ops._device_key(torch.device("cuda", 1)) == 1
    assert ops._device_key("cuda:0") == 0 != ops._device_key("cuda")
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    assert ops._device_key("cuda") == ops._device_key("cuda:0") == 0 and ops._device_key("cuda:1") == 1


def test_norm_logits_routes_by_the_predicate(monkeypatch):
    """norm_logits hands fp32 device logits to the op the predicate names, with or without top-k, and everything else to the
    torch restatement.  (A stand-in tensor class reports ``is_cuda``: the real kernels run in tests/test_gpu_large_vocab.py.)"""
    from triforce_amd import ops
    from triforce_amd.utils import sampling as S

    class FakeDevice(torch.Tensor):
        is_cuda = True

    calls = []
    for name in ("topp_probs", "topk_topp_probs", "topp_probs_large", "topk_topp_probs_large"):
        monkeypatch.setattr(ops, name, lambda lg, *a, _n=name: (calls.append((_n, lg.shape[-1], a)), "kernel")[1])
    for V, want in [(32768, "topp_probs"), (32769, "topp_probs_large"), (262144, "topp_probs_large")]:
        lg = torch.zeros(1, V).as_subclass(FakeDevice)
        calls.clear()
        assert S.norm_logits(lg, temperature=0.6, top_k=-1, top_p=0.9) == "kernel"
        assert calls == [(want, V, (0.6, 0.9))]
        calls.clear()
        assert S.norm_logits(lg, temperature=0.6, top_k=20, top_p=0.9) == "kernel"
        assert calls == [(want.replace("topp_probs", "topk_topp_probs", 1), V, (0.6, 20, 0.9))]
    calls.clear()
    out = S.norm_logits(torch.zeros(1, 262145).as_subclass(FakeDevice), temperature=0.6, top_k=-1, top_p=0.9)
    assert not calls and torch.is_tensor(out) and out.shape == (1, 262145)
    out = S.norm_logits(torch.zeros(1, 40000), temperature=0.6, top_k=-1, top_p=0.9)            # a CPU tensor
    assert not calls and torch.is_tensor(out)


@pytest.mark.parametrize("T,P", [(0.6, 0.9), (1.0, 1.0), (1.0, 1e-9)])
def test_norm_logits_on_cpu_tensors_of_40000_entries_equals_the_oracle(T, P):
    from triforce_amd.utils.sampling import norm_logits
    V = 40000
    gen = torch.Generator().manual_seed(11)
    lg = torch.randn(4, V, generator=gen) * 2.5
    lg[1] = lg[1].half().float()
    lg[2, 33000:33006] = lg[2].sort(descending=True).values[4]      # six equal values straddling rank 5, past entry 32 768
    lg[3] = 0.0
    for k in (-1, 1, 5, V + 3):
        got = norm_logits(lg.clone(), temperature=T, top_k=k, top_p=P)
        want = R.norm_logits(lg.clone(), T, k, P)
        assert torch.equal(got, want), (k, T, P)


def test_the_oracle_itself_holds_the_rules_on_the_rows_it_referees():
    """tests/test_gpu_large_vocab.py compares the dense rows with the oracle only where the oracle ITSELF stays within the
    comparison rules (values at rtol 2e-6 among them) of the float64 restatement of the same filter; everywhere else the float64
    restatement is the reference (large_vocab_ref.reference_kind has the oracle's measured deviation there).  Checked at the
    larger of the two oracle-refereed shapes."""
    from tests import large_vocab_ref as LR
    V, worst = 40000, 0.0
    for T, k, P in [(0.6, None, 0.9), (0.6, 50, 0.9), (1.0, None, 1.0)]:
        for kind, seed in LR.dense_specs(8, 500 + V % 97)[0]:
            if LR.reference_kind(kind, V) != "oracle":
                continue
            lg, want, _ = LR.reference(kind, V, seed, T, k or V, P)
            f64 = LR.norm_logits_f64(lg, T, k or V, P)
            LR.check_rules(lg, f64.float(), want, T, k or V, P, f"float64 restatement vs oracle: {kind} T={T} k={k} P={P}")
            both = (want > 0) & (f64 > 0)
            worst = max(worst, float(((f64[both] - want[both].double()).abs() / f64[both]).max()))
    print(f"oracle vs float64 restatement at V={V}: max relative deviation {worst:.2e} over all kept entries (rtol 2e-6 with atol 1e-9: entries below 5e-4 sit under the atol)")
    assert LR.reference_kind("ties4096", 32769) == "f64" and LR.reference_kind("sigma1", 128256) == "f64"


def test_zoo_names_the_large_vocabulary_pair():
    from triforce_amd.models import zoo
    t, d = zoo.config("tiny-v128k"), zoo.config(zoo.draft_for("tiny-v128k"))
    tiny, d68 = zoo.config("tiny"), zoo.config("llama-68M")
    assert t.vocab_size == d.vocab_size == 128256 and zoo.draft_for("tiny") == "llama-68M" == zoo.draft_for("llama-7B-128K")
    for a, b in ((t, tiny), (d, d68)):
        for f in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "rms_norm_eps"):
            assert getattr(a, f) == getattr(b, f), f
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "test/on_chip.py --target tiny-v128k --weights random:1 --prefill 2048" in readme


def test_top_k_1_at_40000_entries_emits_the_greedy_stream(cpu_ops):
    """tests/test_topk_cpu.py's end-to-end statement with the tiny pair rebuilt at V = 40 000: TriForce(top_k=1, temperature=1,
    top_p=1) emits the target's greedy stream whatever the drafts propose — every teacher-forced gap within GAP_TOL, at most 2
    non-zero."""
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache, StreamingLLMEvictionCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as LlamaForCausalLM_68M
    from triforce_amd.utils.decoding import TriForce
    from triforce_amd.utils.graph_infer import GraphInferenceEngine
    from triforce_amd.utils.sampling import UniformSource
    from oracle import specs
    g = copy.deepcopy(Hh.load_golden("small_gamma6"))
    g["tcfg"]["vocab_size"] = g["dcfg"]["vocab_size"] = 40000
    g["gen_len"] = 48
    gamma = g["gamma"]
    tsd = specs.random_state_dict(g["tcfg"], g["tseed"], head_std=g.get("head_std", 0.05))
    dsd = specs.random_state_dict(g["dcfg"], g["dseed"], head_std=g.get("head_std", 0.05))
    target = LlamaForCausalLM.from_state_dict(LlamaConfig.from_dict(g["tcfg"]), tsd, "cpu")
    draft = LlamaForCausalLM_68M.from_state_dict(LlamaConfig.from_dict(g["dcfg"]), dsd, "cpu")
    assert target.config.vocab_size == 40000
    ge = GraphInferenceEngine(target, FlashSimpleCache(target, g["prefill"] + g["gen_len"] + 16),
                              RetrievalCache(target, max_budget=g["budget"], prefill=g["prefill"], gamma=gamma, chunk_size=g["chunk"]),
                              draft, StreamingLLMEvictionCache(draft, start_size=16, recent_size=256 - 16 - gamma, gamma=gamma))
    ge.initialize_eager(gamma, probs=True, temperature=1.0, top_p=1.0, top_k=1)
    res = TriForce(Hh.FakeTokenizer(), ge, Hh.prompt_of(g), gamma=gamma, max_len=g["gen_len"], top_k=1, top_p=1.0, temperature=1.0,
                   rng=UniformSource("cpu", values=Hh.fixed_uniforms(seed=41)), return_details=True)
    assert max(res["tokens"]) < 40000 and max(res["tokens"]) >= 0
    gaps = Hh.teacher_forced_gaps(g, res["tokens"], tsd, dsd)
    print(f"V=40000 teacher-forced gaps: max {max(gaps):.5f}, {sum(1 for x in gaps if x > 0.0)} of {len(gaps)} not the argmax; "
          f"acceptance {res['acceptance_rate']:.3f}, resampled {res['resampled']}")
    assert max(gaps) <= GAP_TOL, f"token {gaps.index(max(gaps))} trails the target's argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x != 0.0) <= 2
    assert res["resampled"] > 0
