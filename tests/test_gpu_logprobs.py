"""Per-token log-probabilities on the device: tf_token_logprobs against a float64 log_softmax of the same
fp32 logits, and prompt / generation log-probabilities of the tiny small_gamma6 target — eager and from hipGraphs, every verify
route of TriForceRunner — against the CPU oracle and against each other."""
import ctypes
import math

import pytest
import torch

from tests import helpers as Hh
from tests import logprobs_ref as LR
from tests.test_logprobs_cpu import ACCEPTING, SAMPLED, NoEosTokenizer, accepting_uniforms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------------
KINDS = 6         # row r is of kind (r + shift) % 6: N(0, 1), N(0, 8), N(0, 30), all equal, one entry at +80, -inf entries


def _rows(rows, V, shift, gen):
    """(fp32 logits on the host, targets): every row kind and every target kind; a -inf row's target is a -inf entry."""
    x = torch.randn(rows, V, generator=gen)
    t = torch.randint(0, V, (rows,), generator=gen)
    for r in range(rows):
        kind = (r + shift) % KINDS
        if kind < 3:
            x[r] *= (1.0, 8.0, 30.0)[kind]
        elif kind == 3:
            x[r] = 0.37
        elif kind == 4:
            x[r, (7 * r + 3) % V] = 80.0
        t[r] = (0, V - 1, -1, V, int(t[r]))[(r + shift) % 5]
        if kind == 5 and V >= 4:
            x[r, ::3] = -float("inf")
            t[r] = 3 * ((5 * r) % ((V + 2) // 3))
    return x, t


def _bound(x):
    """Per row: four fp32 spacings at the row's span, 4 * 2^-23 * 2^ceil(log2 max(16, span)), span = max |x_i - max x| over
    the finite entries — the subtraction and logf each round once at that magnitude, and the sum of <= 2^17 terms in (0, 1]
    by per-thread partials and a tree carries a relative error of a few 2^-23."""
    xd = x.double()
    mx = xd.max(dim=1, keepdim=True).values
    span = torch.where(torch.isfinite(xd), (xd - mx).abs(), torch.zeros_like(xd)).max(dim=1).values
    return 4.0 * 2.0 ** -23 * 2.0 ** torch.ceil(torch.log2(span.clamp(min=16.0)))


def _device_view(x, layout):
    """The rows on the device: contiguous; row stride V + 3 (rows not 16-byte aligned: scalar heads and tails); or behind a
    4-byte offset from the allocation."""
    rows, V = x.shape
    stride, off = (V + 3, 0) if layout == "strided" else (V, 1 if layout == "offset" else 0)
    flat = torch.full((rows * stride + off + 8,), float("nan"), device=DEV)
    view = flat.as_strided((rows, V), (stride, 1), off)
    view.copy_(x)
    return view


def _compare(got, want, bound, what):
    got, inf = got.double().cpu(), torch.isinf(want)
    assert torch.equal(got[inf], want[inf]), f"{what}: -inf entries differ"
    used = ((got[~inf] - want[~inf]).abs() / bound[~inf])
    worst = float(used.max()) if used.numel() else 0.0
    Hh.record("token_logprobs", worst, what=what)
    assert worst <= 1.0, f"{what}: row {int(used.argmax())} uses {worst:.2f} of its bound"


SHAPES = [(r, V) for r in (1, 7, 33, 1025) for V in (1, 64, 1000, 4097, 32000, 32768, 128256) if r < 1025 or V <= 4097]


@pytest.mark.parametrize("rows,V", SHAPES)
def test_kernel_matches_float64_log_softmax(rows, V):
    from triforce_amd import ops
    gen = torch.Generator().manual_seed(1000 * rows + V)
    for shift in range(KINDS if rows < KINDS else 1):
        x, t = _rows(rows, V, shift, gen)
        ls = torch.log_softmax(x.double(), dim=1)
        want_lse = torch.logsumexp(x.double(), dim=1)
        ok = (t >= 0) & (t < V)
        want = torch.where(ok, ls.gather(1, t.clamp(0, V - 1)[:, None])[:, 0], torch.zeros(rows, dtype=torch.float64))
        bound = _bound(x)
        for layout in ("contiguous", "strided", "offset"):
            xd = _device_view(x, layout)
            what = f"{rows}x{V} {layout} shift {shift}"
            lp, lse = torch.full((rows,), 7.0, device=DEV), torch.full((rows,), 7.0, device=DEV)
            assert ops.token_logprobs(xd, t.to(DEV), out=lp, lse=lse) is lp
            _compare(lp, want, bound, what + " logprob")
            _compare(lse, want_lse, bound, what + " lse")
            only = ops.token_logprobs(xd, None, lse=torch.empty(rows, device=DEV))                  # targets = NULL
            assert torch.equal(only, lse)
            assert torch.equal(ops.token_logprobs(xd, t.to(DEV)), lp)                              # lse = NULL
            if rows <= 32:                                                                          # ids as kernel arguments
                assert torch.equal(ops.token_logprobs(xd, t.tolist()), lp)
        torch.cuda.synchronize()


def test_entry_points_reject_bad_arguments_on_the_device():
    from triforce_amd import hip
    lib = hip.lib()
    x, lp = torch.zeros(2, 8, device=DEV), torch.zeros(2, device=DEV)
    t = torch.zeros(2, dtype=torch.long, device=DEV)
    ids = (ctypes.c_int64 * 32)()
    p, o, tt, null = (ctypes.c_void_p(v) for v in (x.data_ptr(), lp.data_ptr(), t.data_ptr(), 0))
    f, g = lib.tf_token_logprobs, lib.tf_token_logprobs_ids
    for args in ((null, 8, tt, 2, 8, o, o), (p, 8, tt, 0, 8, o, o), (p, 8, tt, 2, 0, o, o), (p, 7, tt, 2, 8, o, o),
                 (p, 8, tt, 2, 8, null, null), (p, 8, null, 2, 8, o, null)):
        assert f(*args, null) == -22, args
    for args in ((null, 8, ids, 2, 8, o, null), (p, 8, null, 2, 8, o, null), (p, 8, ids, 2, 8, null, o),
                 (p, 8, ids, 33, 8, o, null), (p, 8, ids, 0, 8, o, null), (p, 7, ids, 2, 8, o, null)):
        assert g(*args, null) == -22, args
    torch.cuda.synchronize()
    assert float(lp.abs().sum()) == 0.0                               # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# 2. end to end on small_gamma6
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_blocks():
    """Prefill chunks of 128 rows and score blocks of 48: the 999 scored rows cross chunks, blocks end inside chunks."""
    from triforce_amd import ops
    from triforce_amd.utils import graph_infer
    mp = pytest.MonkeyPatch()
    mp.setattr(graph_infer, "PREFILL_CHUNK", 128)
    mp.setattr(ops, "SCORE_BLOCK_ROWS", 48)
    yield
    mp.undo()
    _RUNS.clear()                     # the shared runs keep their engines (and captured graphs) alive: drop them with the module


def _engine(mode, graphs):
    s = SAMPLED if mode == "rejecting" else ACCEPTING
    return Hh.build_product(Hh.load_golden("small_gamma6"), DEV, temperature=s["temperature"], top_p=s["top_p"], graphs=graphs)


_RUNS = {}


def _run(mode, graphs, logprobs=True, prompt_logprobs=False, **knobs):
    """A TriForce run on the fixed uniforms of ``mode`` over a FRESH engine (a second prompt on a used engine selects its
    retrieval chunks by another route, as in the reference, and emits another stream) -> (stats, the runner's device-side
    route was active, the engine); computed once per setting and shared."""
    key = (mode, graphs, logprobs, prompt_logprobs, tuple(sorted(knobs.items())))
    if key not in _RUNS:
        _RUNS[key] = _fresh_run(mode, graphs, logprobs, prompt_logprobs, **knobs)
    return _RUNS[key]


def _fresh_run(mode, graphs, logprobs, prompt_logprobs, max_len=40, **knobs):
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.sampling import UniformSource
    g = Hh.load_golden("small_gamma6")
    sampling, us = (SAMPLED, Hh.fixed_uniforms()) if mode == "rejecting" else (ACCEPTING, accepting_uniforms())
    ge = _engine(mode, graphs)
    run = TriForceRunner(NoEosTokenizer(), ge, g["gamma"], rng=UniformSource(DEV, values=us),
                         logprobs=logprobs, prompt_logprobs=prompt_logprobs, rebuild_every=knobs.get("rebuild_every", 0),
                         **sampling)
    run.eager_every = knobs.get("eager_every", 0)
    run.prefill(Hh.prompt_of(g).to(DEV))
    on_device = run._device_sets() is not None
    while run.n < max_len:
        run.step()
    torch.cuda.synchronize()
    return run.stats(1.0), on_device, ge


@pytest.mark.parametrize("mode,graphs", [("rejecting", False), ("rejecting", True), ("accepting", True)])
def test_prompt_and_generation_logprobs_match_the_oracle(small_blocks, mode, graphs):
    """prompt_logprobs against the oracle's full-prompt logits, generation logprobs against its teacher-forced values;
    the same tokens with logprobs on and off; with graphs the captured device-side step (replay_in_place) is the route."""
    g = Hh.load_golden("small_gamma6")
    prompt = Hh.prompt_of(g)
    off, _, _ = _run(mode, graphs, logprobs=False)
    on, on_device, ge = _run(mode, graphs, prompt_logprobs=True)
    assert on_device == graphs, "with graphs the replay_in_place route must be the one tested"
    assert "logprobs" not in off and on["tokens"] == off["tokens"] and on["counts"] == off["counts"]
    assert (on["resampled"] if mode == "rejecting" else on["bonus"]) > 0, f"no {mode} step in {on['counts']}"
    assert len(on["logprobs"]) == len(on["tokens"]) == on["n"] + 1
    what = f"{mode} graphs={graphs}"
    assert tuple(on["prompt_logprobs"].shape) == (prompt.shape[1] - 1,) and on["prompt_logprobs"].dtype == torch.float32
    LR.check(on["prompt_logprobs"], *LR.prompt_reference(g, prompt), f"gpu prompt_logprobs ({what})")
    want, bounds = LR.teacher_forced_reference(g, prompt, on["tokens"])
    LR.check(on["logprobs"], want, bounds, f"gpu TriForce logprobs ({what})")
    # internal consistency across kernels: prompt + stream through a second scored prefill — prefill attention + hipBLASLt
    # head — against the loop's values — decode attention + skinny head
    full = torch.cat([prompt, torch.tensor([on["tokens"]])], dim=1).to(DEV)
    ge.engine.kv_cache.reset()
    again = ge.inference(full[:, :-1], next_ids=full[0, 1:].contiguous())[1].cpu()
    assert again.numel() == full.shape[1] - 1
    LR.check(again[-len(on["tokens"]):], torch.tensor(on["logprobs"], dtype=torch.float64), bounds,
             f"gpu prefill route vs decode route ({what})")


@pytest.mark.parametrize("knob", [dict(eager_every=1), dict(rebuild_every=2)])
def test_eager_and_rebuild_steps_score_like_captured_steps(small_blocks, knob):
    """Every verify eager (the verify_probs route with eager=True), and every second one a retrieval rebuild: the values are
    the oracle's for the run's own stream, and equal to the captured run's wherever the two streams still coincide."""
    g = Hh.load_golden("small_gamma6")
    prompt = Hh.prompt_of(g)
    base, on_device, _ = _run("rejecting", True, prompt_logprobs=True)
    assert on_device
    got, _, _ = _run("rejecting", True, **knob)
    assert len(got["logprobs"]) == len(got["tokens"])
    want, bounds = LR.teacher_forced_reference(g, prompt, got["tokens"])
    LR.check(got["logprobs"], want, bounds, f"gpu TriForce logprobs ({knob})")
    n = Hh.common_prefix(got["tokens"], base["tokens"])
    assert n >= 1
    LR.check(got["logprobs"][:n], torch.tensor(base["logprobs"][:n], dtype=torch.float64), bounds[:n],
             f"gpu {knob} vs captured steps, {n} common tokens")


def test_autoregressive_logprobs_match_the_oracle(small_blocks):
    from triforce_amd.utils.decoding import Autoregressive
    from triforce_amd.utils.sampling import UniformSource
    g = Hh.load_golden("small_gamma6")
    prompt = Hh.prompt_of(g)
    ge = _engine("rejecting", True)
    assert 1 in ge.target_graphs                                         # the captured q_len == 1 step is the one scored
    rng = lambda: UniformSource(DEV, values=Hh.fixed_uniforms())        # noqa: E731
    _, want = Autoregressive(NoEosTokenizer(), ge, prompt.to(DEV), max_len=24, rng=rng(), return_tokens=True, **SAMPLED)
    out = Autoregressive(NoEosTokenizer(), ge, prompt.to(DEV), max_len=24, rng=rng(), logprobs=True, **SAMPLED)
    assert len(out) == 3 and out[1] == want and len(out[2]) == 25
    LR.check(out[2], *LR.teacher_forced_reference(g, prompt, out[1]), "gpu Autoregressive logprobs")


def _finite_run(ge, g, max_len=24):
    from triforce_amd.utils.decoding import TriForce
    prompt = Hh.prompt_of(g).to(DEV)
    st = TriForce(NoEosTokenizer(), ge, prompt, gamma=g["gamma"], max_len=max_len, return_details=True, logprobs=True,
                  prompt_logprobs=True, **SAMPLED)
    lp, plp = torch.tensor(st["logprobs"]), st["prompt_logprobs"]
    assert lp.numel() == len(st["tokens"]) == st["n"] + 1 and plp.numel() == prompt.shape[1] - 1
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(plp).all())
    assert float(lp.max()) <= 0.0 and float(plp.max()) <= 0.0 and float(plp.mean()) > -math.log(g["tcfg"]["vocab_size"]) - 4
    return st


def test_smoke_fp8_kv_cache(small_blocks, monkeypatch):
    """The FP8 KV tier needs nothing: only logits are consumed."""
    import copy
    from triforce_amd.models.cache import KV_CACHE_ENV
    monkeypatch.setenv(KV_CACHE_ENV, "fp8")
    g = copy.deepcopy(Hh.load_golden("small_gamma6"))
    g["tcfg"]["num_attention_heads"] = g["tcfg"]["num_key_value_heads"] = 2        # head_dim 128, the FP8 cache's head size
    ge = Hh.build_product(g, DEV, temperature=SAMPLED["temperature"], top_p=SAMPLED["top_p"], graphs=True)
    assert ge.engine.kv_cache.fp8
    _finite_run(ge, g)


def test_smoke_gqa_target(small_blocks):
    from oracle import specs
    from tests.test_gqa_cpu import gqa_state_dicts
    g = dict(Hh.load_golden("small_gamma6"))
    tcfg = specs.llama_config(512, 768, 2, 4, vocab_size=g["dcfg"]["vocab_size"], max_position_embeddings=4096,
                              rope_scaling=dict(type="yarn", factor=16.0, original_max_position_embeddings=256),
                              name="tiny-yarn-gqa-target")
    g.update(tcfg=tcfg, tseed=711, prefill=512, gen_len=160, budget=256)
    gcfg, gsd, _ = gqa_state_dicts(g["tcfg"], g["tseed"], 2)
    dsd = specs.random_state_dict(g["dcfg"], g["dseed"], head_std=g["head_std"])
    ge = Hh.build_product(dict(g, tcfg=gcfg), DEV, gsd, dsd, temperature=SAMPLED["temperature"], top_p=SAMPLED["top_p"],
                          graphs=True)
    assert ge.engine.model.gqa
    _finite_run(ge, g)
