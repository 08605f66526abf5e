"""Per-token log-probabilities without a GPU: the C ABI's argument gates, and the HOST logic — prompt
scoring through the chunked prefill's head, generation scoring on every verify route of TriForceRunner, extend(), the
autoregressive loop, the refusals — with every HIP op swapped for its oracle restatement (cpu_ops) and
ops.token_logprobs for the torch restatement below.  The kernel itself is checked in tests/test_gpu_logprobs.py."""
import ctypes
import os
import re

import pytest
import torch

from tests import helpers as Hh
from tests import logprobs_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLED = dict(top_k=-1, top_p=0.9, temperature=0.6)


def token_logprobs_cpu(logits, targets=None, out=None, lse=None):
    """ops.token_logprobs restated in fp32 torch: x[t] - max - log sum exp(x - max); a target outside [0, V) gives 0."""
    assert logits.dtype == torch.float32 and logits.dim() == 2
    rows, V = logits.shape
    m = logits.max(dim=1).values
    logs = torch.log(torch.exp(logits - m[:, None]).sum(dim=1))
    if lse is not None:
        lse.copy_(m + logs)
    if targets is None:
        assert lse is not None
        return lse
    t = torch.as_tensor(targets, dtype=torch.long).reshape(-1)
    assert t.numel() == rows
    ok = (t >= 0) & (t < V)
    val = (logits.gather(1, t.clamp(0, V - 1)[:, None])[:, 0] - m) - logs
    val = torch.where(ok, val, torch.zeros_like(val))
    if out is None:
        out = torch.empty(rows, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.numel() == rows
    out.copy_(val)
    return out


@pytest.fixture
def lp_ops(cpu_ops, monkeypatch):
    """cpu_ops + the restatement, and score blocks of 48 rows so that blocks end inside the CPU's 128-row chunks."""
    monkeypatch.setattr(cpu_ops, "token_logprobs", token_logprobs_cpu)
    monkeypatch.setattr(cpu_ops, "SCORE_BLOCK_ROWS", 48)
    return cpu_ops


# ---- ABI --------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    from triforce_amd import hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "triforce_hip.h")).read(), flags=re.S)
    for name in ("tf_token_logprobs", "tf_token_logprobs_ids"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/triforce_hip.h"
        assert name in hip.SIGNATURES and hip.SIGNATURES[name][0] is ctypes.c_int
        assert hasattr(hip.lib(), name)
    assert len(hip.SIGNATURES["tf_token_logprobs"][1]) == 8


def test_bad_arguments_are_rejected_before_any_launch():
    """Every TF_EINVAL case of the header, through the C ABI on a machine without a device: one bad argument per call, the
    rest valid host stand-ins that a launch would have to read (none may be reached)."""
    from triforce_amd import hip
    lib = hip.lib()
    buf = (ctypes.c_float * 64)()
    ids = (ctypes.c_int64 * 32)(*range(32))
    p, t, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ids, ctypes.c_void_p), ctypes.c_void_p(0)
    f = lib.tf_token_logprobs
    assert f(null, 8, t, 2, 8, p, p, null) == -22                   # NULL logits
    assert f(p, 8, t, 0, 8, p, p, null) == -22                      # rows < 1
    assert f(p, 8, t, -3, 8, p, p, null) == -22
    assert f(p, 8, t, 2, 0, p, p, null) == -22                      # V < 1
    assert f(p, 7, t, 2, 8, p, p, null) == -22                      # row_stride < V
    assert f(p, 8, t, 2, 8, null, null, null) == -22                # no output at all
    assert f(p, 8, null, 2, 8, p, null, null) == -22                # logprob without targets and no lse
    assert f(p, 8, t, 2, 8, null, null, null) == -22                # targets without logprob and no lse
    g = lib.tf_token_logprobs_ids
    assert g(null, 8, t, 2, 8, p, null, null) == -22
    assert g(p, 8, null, 2, 8, p, null, null) == -22                # NULL host ids
    assert g(p, 8, t, 2, 8, null, p, null) == -22                   # NULL logprob
    assert g(p, 8, t, 0, 8, p, null, null) == -22
    assert g(p, 8, t, 33, 8, p, null, null) == -22                  # more ids than kernel arguments
    assert g(p, 8, t, 2, 0, p, null, null) == -22
    assert g(p, 7, t, 2, 8, p, null, null) == -22


def test_op_refuses_cpu_tensors():
    from triforce_amd import hip, ops
    x = torch.zeros(2, 8)
    with pytest.raises(hip.TriforceHipError):
        ops.token_logprobs(x, torch.zeros(2, dtype=torch.long))
    with pytest.raises(hip.TriforceHipError):
        ops.token_logprobs(x, [1, 2])
    with pytest.raises(hip.TriforceHipError):
        ops.token_logprobs(x, None, lse=torch.zeros(2))


# ---- host logic -------------------------------------------------------------------------------------------------------
def _golden(**over):
    return dict(Hh.load_golden("small_gamma6"), **over)


def _rng():
    from triforce_amd.utils.sampling import UniformSource
    return UniformSource("cpu", values=Hh.fixed_uniforms())


def test_prompt_logprobs_equal_the_oracles(lp_ops):
    """n - 1 values, equal to log_softmax of the oracle's full-prompt logits at the next ids; the prompt crosses the CPU's
    128-row chunks and the 48-row score blocks end inside them.  The logits prefill() hands to start() are unchanged: the
    first token is the one a prefill without scoring samples."""
    from triforce_amd.utils.decoding import TriForceRunner
    g = _golden()
    prompt = Hh.prompt_of(g)
    n = prompt.shape[1]
    assert n - 1 > 2 * 128 and (n - 1) % 48 != 0 and 128 % 48 != 0
    first = []
    for score in (True, False):
        run = TriForceRunner(Hh.FakeTokenizer(), Hh.build_product(g, "cpu"), g["gamma"], rng=_rng(), prompt_logprobs=score,
                             **SAMPLED)
        run.prefill(prompt)
        first.append(run.next_token)
        if score:
            got = run.stats(1.0)["prompt_logprobs"]
            assert got.dtype == torch.float32 and tuple(got.shape) == (n - 1,) and not got.is_cuda
            LR.check(got, *LR.prompt_reference(g, prompt), "cpu prompt_logprobs")
        else:
            assert "prompt_logprobs" not in run.stats(1.0)
    assert first[0] == first[1]


# The random draft and target of small_gamma6 agree on ~5 % of the drafted tokens, so a run on plain uniforms holds rejection
# steps only.  The fourth powers of the same numbers at T = 1 / top-p 1 (every probability positive, most accept draws close
# to 0) give all-accepted steps.
ACCEPTING = dict(top_k=-1, top_p=1.0, temperature=1.0)


class NoEosTokenizer(Hh.FakeTokenizer):
    """The reference stops at an accepted eos; this loop goes on, and from such a step on the rows in the full cache are no
    longer exactly the emitted stream (TriForceRunner.step, reason 2).  The values then follow the cache, so the
    teacher-forced comparison — which feeds the emitted stream — runs without an eos id."""
    eos_token_id = None


def accepting_uniforms():
    return [u ** 4 for u in Hh.fixed_uniforms()]


@pytest.mark.parametrize("mode", ["rejecting", "accepting"])
def test_triforce_logprobs_same_tokens_and_teacher_forced_values(lp_ops, mode):
    """logprobs=True emits the stream logprobs=False emits under the same uniforms, one value per token, each the
    oracle's teacher-forced value; one run holds rejection steps, the other all-accepted steps."""
    from triforce_amd.utils.decoding import TriForce
    from triforce_amd.utils.sampling import UniformSource
    g = _golden()
    prompt, tok = Hh.prompt_of(g), NoEosTokenizer()
    sampling, us = (SAMPLED, Hh.fixed_uniforms()) if mode == "rejecting" else (ACCEPTING, accepting_uniforms())
    kw = dict(gamma=g["gamma"], max_len=40, return_details=True, **sampling)
    tp = dict(temperature=sampling["temperature"], top_p=sampling["top_p"])
    off = TriForce(tok, Hh.build_product(g, "cpu", **tp), prompt, rng=UniformSource("cpu", values=us), **kw)
    on = TriForce(tok, Hh.build_product(g, "cpu", **tp), prompt, rng=UniformSource("cpu", values=us), logprobs=True,
                  prompt_logprobs=True, **kw)
    assert "logprobs" not in off and "prompt_logprobs" not in off
    assert on["tokens"] == off["tokens"] and on["counts"] == off["counts"]
    assert (on["resampled"] if mode == "rejecting" else on["bonus"]) > 0, f"no {mode} step in {on['counts']}"
    assert len(on["logprobs"]) == len(on["tokens"]) == on["n"] + 1
    LR.check(on["logprobs"], *LR.teacher_forced_reference(g, prompt, on["tokens"]), f"cpu TriForce logprobs ({mode})")
    LR.check(on["prompt_logprobs"], *LR.prompt_reference(g, prompt), "cpu TriForce prompt_logprobs")


def _tp():
    return dict(temperature=SAMPLED["temperature"], top_p=SAMPLED["top_p"])


def test_session_ask_scores_each_answer_from_its_own_context(lp_ops):
    """extend() resets the buffer: the answer to a follow-up question carries one value per token, the first scored from
    extend's last-row logits, all equal to the oracle's values behind document + question."""
    from triforce_amd.utils.decoding import TriForceSession
    g = _golden(gen_len=120, budget=320)
    doc = Hh.prompt_of(g)
    q = torch.randint(3, g["tcfg"]["vocab_size"], (1, 9), generator=torch.Generator().manual_seed(5))
    s = TriForceSession(Hh.FakeTokenizer(), Hh.build_product(g, "cpu", **_tp()), g["gamma"], rng=_rng(), logprobs=True, **SAMPLED)
    s.prefill(doc)
    st0 = s.generate(12)
    assert len(st0["logprobs"]) == len(st0["tokens"])
    LR.check(st0["logprobs"], *LR.teacher_forced_reference(g, doc, st0["tokens"]), "cpu session first answer")
    st = s.ask(q, 16)
    assert len(st["logprobs"]) == len(st["tokens"]) == st["n"] + 1
    context = torch.cat([doc[:, :s.document], q], dim=1)
    LR.check(st["logprobs"], *LR.teacher_forced_reference(g, context, st["tokens"]), "cpu session ask")


def test_autoregressive_logprobs(lp_ops):
    from triforce_amd.utils.decoding import Autoregressive
    g = _golden()
    prompt, tok = Hh.prompt_of(g), Hh.FakeTokenizer()
    _, want = Autoregressive(tok, Hh.build_product(g, "cpu"), prompt, max_len=20, rng=_rng(), return_tokens=True, **SAMPLED)
    out = Autoregressive(tok, Hh.build_product(g, "cpu"), prompt, max_len=20, rng=_rng(), logprobs=True, **SAMPLED)
    assert len(out) == 3 and out[1] == want and len(out[2]) == len(want) == 21
    LR.check(out[2], *LR.teacher_forced_reference(g, prompt, out[1]), "cpu Autoregressive logprobs")


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refused_on_the_tensor_parallel_loop_sequoia_and_the_offloaded_cache(cpu_ops):
    import types
    from triforce_amd.models.cache import OffloadingFlashSimpleCache
    from triforce_amd.utils import decoding as D
    from triforce_amd.utils.SpecTree_TP import SpecTree
    tok = Hh.FakeTokenizer()
    llm = types.SimpleNamespace(temperature=0.6, top_p=0.9)
    for kw in (dict(logprobs=True), dict(prompt_logprobs=True)):
        with pytest.raises(NotImplementedError, match="TriForce_Dist"):
            D.TriForce_Dist(tok, llm, torch.zeros(1, 8, dtype=torch.long), **kw)
        with pytest.raises(NotImplementedError, match="_DistEngine"):
            D._DistEngine(llm, **kw)
        with pytest.raises(NotImplementedError, match="SpecTree"):
            SpecTree(None, **kw)
    with pytest.raises(NotImplementedError, match="Baseline_Dist"):
        D.Baseline_Dist(tok, llm, torch.zeros(1, 8, dtype=torch.long), logprobs=True)
    # a runner over a tensor-parallel engine wrapper, and over the host-offloaded full cache
    g = _golden()
    ge = Hh.build_product(g, "cpu")
    with pytest.raises(NotImplementedError, match="SimpleNamespace"):
        D.TriForceRunner(tok, types.SimpleNamespace(engine=ge.engine), g["gamma"], logprobs=True)
    ge.engine.kv_cache = OffloadingFlashSimpleCache.__new__(OffloadingFlashSimpleCache)
    for kw in (dict(logprobs=True), dict(prompt_logprobs=True)):
        with pytest.raises(NotImplementedError, match="OffloadingFlashSimpleCache"):
            D.TriForceRunner(tok, ge, g["gamma"], **kw)
    with pytest.raises(NotImplementedError, match="OffloadingFlashSimpleCache"):
        D.Autoregressive(tok, ge, Hh.prompt_of(g), max_len=4, logprobs=True)
    ok = D.TriForceRunner(tok, Hh.build_product(g, "cpu"), g["gamma"])
    with pytest.raises(NotImplementedError, match="OffloadingFlashSimpleCache"):
        ok.ge.engine.kv_cache = ge.engine.kv_cache
        ok.prefill(Hh.prompt_of(g), prompt_logprobs=True)


def test_on_chip_flag():
    from triforce_amd.utils import cli
    assert cli.parse("on_chip", []).logprobs is False and cli.parse("on_chip", ["--logprobs"]).logprobs is True
    assert "--logprobs" in [f[0] for f in cli.SCRIPT_OWN["on_chip"]]
    assert "--logprobs" not in [f[0] for f in cli.SCRIPTS["on_chip"]]          # the table compared with the reference's
