"""Min-p on the target tier, the parts that need no GPU: the C ABI and every argument gate of tf_minp_probs
/ tf_minp_probs_large, the torch fallback of norm_logits against the float64 restatement (tests/minp_ref.py), the routing of
``min_p`` through GraphInferenceEngine, the decode loop on the CPU backend (cpu_ops) and the command line.  The kernels are
checked in tests/test_gpu_minp.py."""
import ctypes
import os
import re

import pytest
import torch

from tests import helpers as Hh
from tests import minp_ref as MR

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
    for name in ("tf_minp_probs", "tf_minp_probs_large"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", decl), f"include/triforce_hip.h does not declare {name}"
        assert name in hip.SIGNATURES
        assert hasattr(lib, name), f"libtriforce_hip.so does not export {name}"
    assert len(hip.SIGNATURES["tf_minp_probs"][1]) == 9 and len(hip.SIGNATURES["tf_minp_probs_large"][1]) == 11
    assert callable(ops.minp_probs) and callable(ops.minp_probs_large)
    assert "tf_minp_probs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()

    # no device is touched below: host buffers stand in for device pointers, every call must return before any launch
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    aligned = ctypes.c_void_p((p.value + 15) & ~15)
    null = ctypes.c_void_p(0)
    big = 1 << 40

    def small(lg=aligned, pr=aligned, rows=1, V=8, T=0.6, k=2, P=0.9, m=0.1):
        return lib.tf_minp_probs(lg, pr, rows, V, T, k, P, m, null)

    def large(lg=aligned, pr=aligned, rows=1, V=8, T=0.6, k=2, P=0.9, m=0.1, ws=aligned, nb=big):
        return lib.tf_minp_probs_large(lg, pr, rows, V, T, k, P, m, ws, nb, null)

    nan = float("nan")
    common = (dict(lg=null), dict(pr=null), dict(rows=0), dict(rows=-1), dict(V=0), dict(V=-5), dict(T=0.0), dict(T=-1.0),
              dict(T=nan), dict(P=0.0), dict(P=-0.5), dict(P=nan), dict(m=0.0), dict(m=-0.1), dict(m=nan), dict(m=1.0000001),
              dict(m=2.0))
    for fn in (small, large):
        for kw in common:
            assert fn(**kw) == EINVAL, (fn.__name__, kw)
            for k in (-1, 0, 8, 100):                               # every top_k is legal: <= 0 and >= V mean "no top-k filter"
                assert fn(**dict(kw, k=k)) == EINVAL, (fn.__name__, kw, k)
    assert small(V=32769) == ERANGE and small(V=1 << 30) == ERANGE and small(V=32769, k=-1) == ERANGE
    assert small(V=32769, m=0.0) == EINVAL and small(V=32769, T=0.0) == EINVAL          # EINVAL outranks the size gate
    for kw in (dict(ws=null), dict(ws=ctypes.c_void_p(aligned.value + 4)), dict(rows=33)):
        assert large(**kw) == EINVAL, kw
    assert large(V=262145) == ERANGE and large(V=262145, nb=0) == ERANGE and large(V=1 << 30) == ERANGE
    assert large(V=262145, m=0.0) == EINVAL and large(rows=0, nb=0) == EINVAL and large(m=1.5, nb=0) == EINVAL
    for rows, V in [(1, 8), (1, 32769), (7, 128256), (32, 262144)]:
        for k in (-1, 2):
            assert large(rows=rows, V=V, k=k, nb=_ws_bytes(rows, V) - 1) == ENOSPC, (rows, V, k)
            assert large(rows=rows, V=V, k=k, nb=0) == ENOSPC
    # the entries without min-p keep their gates
    assert lib.tf_topk_topp_probs(aligned, aligned, 1, 8, 0.6, 0, 0.9, null) == EINVAL
    assert lib.tf_topp_probs(aligned, aligned, 1, 32769, 0.6, 0.9, null) == ERANGE


def _cpu_rows(V, seed):
    gen = torch.Generator().manual_seed(seed)
    lg = torch.randn(6, V, generator=gen) * 2.5
    lg[1] = lg[1].half().float()
    lg[2, 10:16] = lg[2].sort(descending=True).values[4]            # six equal values straddling rank 5
    lg[3] = 0.0
    lg[4, 20:23] = lg[4].max() + 1.0                                # three equal maxima
    lg[5, 30:34] = lg[5].max() - 1.5                                # a tie group 1.5 below the maximum: e = 0.22 at T = 1
    return lg


@pytest.mark.parametrize("P", [1.0, 0.9])
@pytest.mark.parametrize("k", [-1, 5])
@pytest.mark.parametrize("min_p", [0.02, 0.3, 1.0])
def test_norm_logits_torch_fallback_equals_the_float64_restatement(min_p, k, P):
    """CPU tensors take the torch restatement (filter, softmax, mask p < min_p * p_max, renormalise): the support is exactly
    the float64 reference's and the values agree at the project's rtol 2e-6."""
    from triforce_amd.utils.sampling import norm_logits
    for T in (1.0, 0.7):
        lg = MR.nudged(_cpu_rows(96, 7), T, (min_p,))
        got = norm_logits(lg.clone(), temperature=T, top_k=k, top_p=P, min_p=min_p)
        assert got.dtype == torch.float32
        flipped = MR.check(lg, got, T, k, P, min_p, f"cpu fallback T={T} k={k} P={P} min_p={min_p}")
        assert flipped == 0
        if min_p == 1.0:
            third = got[4, 20:23] - torch.tensor(1.0 / 3.0)
            assert float(third.abs().max()) <= 2.0 ** -24           # fp32 softmax, then renormalise: 2 ulps of 1/3
            assert int((got[0] > 0).sum()) == 1 and float(got[0].max()) == 1.0
        grp = got[5, 30:34]
        assert bool((grp > 0).all()) or bool((grp == 0).all()), "a group of equal logits was split"


def test_min_p_zero_is_the_call_without_the_keyword(monkeypatch):
    from triforce_amd import ops
    from triforce_amd.utils import sampling as S
    lg = _cpu_rows(96, 9)
    for T, k, P in [(0.6, -1, 0.9), (1.0, 5, 1.0), (0.8, 20, 0.95), (1.0, -1, 1e-9)]:
        want = S.norm_logits(lg.clone(), temperature=T, top_k=k, top_p=P)
        for m in (0.0, -1.0):
            assert torch.equal(S.norm_logits(lg.clone(), temperature=T, top_k=k, top_p=P, min_p=m), want), (T, k, P, m)
    # fp32 device logits with min_p > 0 go to the two new ops by the routing predicate; min_p <= 0 never reaches them

    class FakeDevice(torch.Tensor):
        is_cuda = True

    calls = []
    for name in ("topp_probs", "topk_topp_probs", "topp_probs_large", "topk_topp_probs_large", "minp_probs", "minp_probs_large"):
        monkeypatch.setattr(ops, name, lambda lg, *a, _n=name: (calls.append((_n, lg.shape[-1], a)), "kernel")[1])
    for V, want in [(32768, "minp_probs"), (32769, "minp_probs_large"), (262144, "minp_probs_large")]:
        dl = torch.zeros(1, V).as_subclass(FakeDevice)
        for k in (-1, 20):
            calls.clear()
            assert S.norm_logits(dl, temperature=1.0, top_k=k, top_p=1.0, min_p=0.3) == "kernel"
            assert calls == [(want, V, (1.0, k, 1.0, 0.3))]
            calls.clear()
            assert S.norm_logits(dl, temperature=1.0, top_k=k, top_p=1.0, min_p=0.0) == "kernel"
            assert len(calls) == 1 and not calls[0][0].startswith("minp")
    calls.clear()
    out = S.norm_logits(torch.zeros(1, 262145).as_subclass(FakeDevice), temperature=1.0, top_k=-1, top_p=1.0, min_p=0.3)
    assert not calls and torch.is_tensor(out)
    out = S.norm_logits(torch.zeros(1, 64).as_subclass(FakeDevice), temperature=1.0, top_k=-1, top_p=0.0, min_p=0.3)
    assert not calls and torch.is_tensor(out)                       # top_p <= 0: the torch restatement


def test_filters_normalise_once_and_compare_by_field():
    from triforce_amd.utils.sampling import Filters
    assert Filters(.6, .9, 0, -1.0) == Filters(.6, .9, -1, 0.0) == Filters(.6, .9)
    assert hash(Filters(.6, .9, 0, -1.0)) == hash(Filters(.6, .9)) and len({Filters(.6, .9, -5), Filters(.6, .9, 0, -0.0)}) == 1
    f = Filters(.6, .9, -7, -0.5)
    assert (f.temperature, f.top_p, f.top_k, f.min_p) == (.6, .9, -1, 0.0)
    for other in (Filters(.7, .9), Filters(.6, .8), Filters(.6, .9, 5), Filters(.6, .9, min_p=.1), Filters(.6, .9, 5, .1)):
        assert other != Filters(.6, .9)
    assert [Filters(.6, .9, k, m).target_only for k, m in [(-1, 0.0), (0, -1.0), (5, 0.0), (-1, 0.1), (5, 0.1)]] \
        == [False, False, True, True, True]
    # as keywords of norm_logits: ``min_p`` only when it is on
    assert Filters(.6, .9, 0).kw() == dict(temperature=.6, top_k=-1, top_p=.9)
    assert Filters(.6, .9, 5, .1).kw() == dict(temperature=.6, top_k=5, top_p=.9, min_p=.1)
    with pytest.raises(Exception):
        f.top_k = 3                                                 # frozen


def test_dist_engine_serves_no_target_only_filter():
    """The tensor-parallel engine normalises at whatever temperature / top-p it is handed and has no top-k or min-p: its
    verify_probs_ids answers None for either, before the ``llm`` is touched."""
    import types
    from triforce_amd.utils.decoding import _DistEngine
    from triforce_amd.utils.sampling import Filters

    class Llm:
        temperature, top_p, device, draft = 0.6, 0.9, "cpu", None
        config = types.SimpleNamespace(model_config=None)
        kv_cache = retrieval_cache = draft_cache = None

        def verify_probs_ids(self, *a, **kw):
            raise AssertionError("the llm was called")
    ge = _DistEngine(Llm())
    assert ge.verify_probs_ids([1, 2, 3], 0.6, 0.9, top_k=5) is None
    assert ge.verify_probs_ids([1, 2, 3], 0.6, 0.9, min_p=0.1) is None
    assert ge.verify_probs_ids([1, 2, 3], temperature=0.6, top_k=5, top_p=0.9, min_p=0.1) is None
    with pytest.raises(AssertionError, match="the llm was called"):
        ge.verify_probs_ids([1, 2, 3], 0.7, 0.8, top_k=0, min_p=-1.0)      # no filter of the target's own: handed on
    assert ge.serves(Filters(0.7, 0.8)) and not ge.serves(Filters(0.6, 0.9, 5)) and not ge.serves(Filters(0.6, 0.9, min_p=0.1))


def test_only_on_chip_takes_the_min_p_flag():
    from triforce_amd.utils import cli
    assert any(row[0] == "--min_p" for row in cli.SCRIPT_OWN["on_chip"])
    for script, rows in cli.SCRIPTS.items():
        assert all(row[0] != "--min_p" for row in rows), script
    assert cli.parse("on_chip", []).min_p == 0.0
    assert cli.parse("on_chip", ["--min_p", "0.05"]).min_p == 0.05
    for script in ("offloading", "offloading_TP", "offloading_seqouia"):
        with pytest.raises(SystemExit):
            cli.parse(script, ["--min_p", "0.05"])
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--min_p" in readme


def test_min_p_1_on_the_target_tier_emits_the_greedy_stream(cpu_ops):
    """An engine built with ``min_p=1.0`` and TriForce(min_p=1.0, temperature=1, top_p=1): the target's distribution keeps only
    the row maxima while both draft tiers keep sampling at temperature 1 unfiltered, so whatever they propose, speculative
    sampling must emit the target's greedy stream — stated as tests/test_topk_cpu.py states it for top_k = 1.  Then the match
    rule over runner and engine ``min_p`` pairs."""
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
    assert ge.target_filters.min_p == 0.0
    ge.initialize_eager(gamma, probs=True, temperature=1.0, top_p=1.0, min_p=1.0)
    assert ge.target_filters == Filters(1.0, 1.0, -1, 1.0) and "min_p" not in ge.sampling     # the draft tiers' capture arguments never see it
    res = TriForce(Hh.FakeTokenizer(), ge, Hh.prompt_of(g), gamma=gamma, max_len=g["gen_len"], top_p=1.0, temperature=1.0,
                   min_p=1.0, rng=UniformSource("cpu", values=Hh.fixed_uniforms(seed=41)), return_details=True)
    gaps = Hh.teacher_forced_gaps(g, res["tokens"], tsd, dsd)
    print(f"teacher-forced gaps: max {max(gaps):.5f}, {sum(1 for x in gaps if x > 0.0)} of {len(gaps)} not the argmax; "
          f"acceptance {res['acceptance_rate']:.3f}, resampled {res['resampled']}")
    assert max(gaps) <= GAP_TOL, f"token {gaps.index(max(gaps))} trails the target's argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x != 0.0) <= 2
    assert res["resampled"] > 0                                    # the drafts did propose something else, and it was corrected
    # the routing rule: the engine's captured min-p must equal the runner's (any value <= 0 counts as 0), next to the top-k rule
    for runner_m, engine_m, match in [(0.3, 0.3, True), (0.0, 0.3, False), (0.3, 0.0, False), (-1.0, 0.0, True), (0.0, -2.0, True),
                                      (0.05, 0.3, False), (1.0, 1.0, True)]:
        ge.initialize_eager(gamma, probs=True, temperature=1.0, top_p=1.0, top_k=20, min_p=engine_m)
        run = TriForceRunner(Hh.FakeTokenizer(), ge, gamma, top_k=20, top_p=1.0, temperature=1.0, min_p=runner_m)
        assert run._served() is match and ge.serves(run.filters) is match, (runner_m, engine_m)
        assert run.filters.top_k == ge.target_filters.top_k == 20   # (the top-k half of the rule holds throughout)
        assert ge.serves(Filters(1.0, 1.0, 20, runner_m)) is match
        assert ge.serves(Filters(1.0, 1.0, 20, min_p=runner_m)) is match
        assert ge.serves(Filters(1.0, 1.0, 20)) is (engine_m <= 0)  # callers that pass no min_p mean "none"
        assert ge.serves(Filters(1.0, 1.0, 21, runner_m)) is False
    # an engine without the attribute (tensor-parallel, Sequoia, stubs) captured without min-p

    class Bare:
        engine = ge.engine
        sampling = ge.sampling
    run = TriForceRunner(Hh.FakeTokenizer(), ge, gamma, top_p=1.0, temperature=1.0, min_p=0.3)
    run.ge = Bare()
    assert run._served() is False                                  # no ``serves``: captured without top-k and min-p
    run.filters = Filters(1.0, 1.0, min_p=0.0)
    assert run._served() is True
