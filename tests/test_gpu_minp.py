"""Min-p on the device: tf_minp_probs / tf_minp_probs_large against the float64 restatement of the rule
(tests/minp_ref.py), their bit-identity with the kernels without min-p where min-p cannot bite and with each other, graph
replay, and the captured target verify / decode loop with min_p > 0 at 32 000 and 128 256 entries."""
import pytest
import torch

from oracle import specs
from tests import helpers as Hh
from tests import minp_ref as MR
from tests.test_gpu_topk import _rows as _rows11

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP_TOL = 8e-3        # as tests/test_gpu_e2e.py: an emitted token may trail the target's argmax by ~2 fp16 spacings
SMALL_V, LARGE_V = (64, 1000, 4097, 32768), (32769, 128256, 262144)
TINY_MIN_P = 2.0 ** -41                                             # below every top-p boundary: (1 - 0.9) / (2 V) > 1.9e-7


def _ops():
    from triforce_amd import ops
    return ops


def _minp(ops, V):
    return ops.minp_probs if V <= 32768 else ops.minp_probs_large


_BLOCKS = {}


def _block(V, T):
    """The 11 rows of tests/test_gpu_topk.py (k = 50: its tie rows straddle rank 50), N(0, 1) and N(0, 8) rows, and one N(0, 2.5)
    row with a PLANTED GROUP of six equal logits T * ln(10) below the maximum (e = 0.1: inside every min_p <= 0.02 set, outside
    every min_p >= 0.3 one) — guard-banded for every min_p the tests use at this T.  Built once per (V, T), never modified."""
    if (V, T) not in _BLOCKS:
        k = min(50, V - 1)
        gen = torch.Generator().manual_seed(4000 + V)
        extra = torch.randn(3, V, generator=gen) * torch.tensor([[1.0], [8.0], [2.5]])
        extra[2, 0] = float(extra[2].max()) + 0.5                    # (the maximum sits outside the group)
        extra[2, torch.arange(6) * (V // 6) + 1] = float(extra[2, 0]) - T * 2.302585
        lg = torch.cat([_rows11(V, k, 90 + V), extra])
        _BLOCKS[(V, T)] = MR.nudged(lg, T, (0.02, 0.1, 0.3, 1.0))
    return _BLOCKS[(V, T)]


def _cycled(lg, rows):
    return lg[torch.arange(rows) % lg.shape[0]].contiguous()


# ---- (a) bit-identity where min-p cannot bite ---------------------------------------------------------------------------------
@pytest.mark.parametrize("V", SMALL_V + LARGE_V)
def test_a_tiny_min_p_leaves_every_bit_of_the_kernels_without_min_p(V, monkeypatch):
    ops = _ops()
    monkeypatch.setattr(ops, "TOPP_MULTI", False)               # the one-workgroup-per-row tf_topp_probs
    small = V <= 32768
    for rows in (1, 8, 33) if small else (1, 8):
        dl = _cycled(_block(V, 0.6), rows).to(DEV)
        for T in (0.6, 1.0):
            want = ops.topp_probs(dl, T, 0.9) if small else ops.topp_probs_large(dl, T, 0.9)
            k = min(50, V - 1)
            want_k = ops.topk_topp_probs(dl, T, k, 0.9) if small else ops.topk_topp_probs_large(dl, T, k, 0.9)
            fn = _minp(ops, V)
            for kk in (-1, 0, V, V + 5):
                assert torch.equal(fn(dl, T, kk, 0.9, TINY_MIN_P), want), (V, rows, T, kk)
            assert torch.equal(fn(dl, T, k, 0.9, TINY_MIN_P), want_k), (V, rows, T, k)
            if small:                                               # the _large form over the same rows
                assert torch.equal(ops.minp_probs_large(dl, T, -1, 0.9, TINY_MIN_P), want), (V, rows, T)


# ---- (b) min-p alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", SMALL_V + LARGE_V)
def test_b_min_p_alone_has_the_references_support_and_values(V):
    ops = _ops()
    for T in (1.0, 0.7):
        lg = _block(V, T)
        dl = lg.to(DEV)
        group = torch.arange(6) * (V // 6) + 1
        for min_p in (0.02, 0.3):
            got = _minp(ops, V)(dl, T, -1, 1.0, min_p).cpu()
            assert MR.check(lg, got, T, None, 1.0, min_p, f"V={V} T={T} min_p={min_p}") == 0
            grp = got[13, group]
            assert bool((grp > 0).all()) if min_p < 0.1 else bool((grp == 0).all()), f"the planted group at e = 0.1, min_p={min_p}: {grp}"
            assert float(grp.max()) == float(grp.min())


# ---- (c) min_p = 1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", SMALL_V + LARGE_V)
def test_c_min_p_1_keeps_exactly_the_row_maxima(V):
    ops = _ops()
    gen = torch.Generator().manual_seed(5000 + V)
    lg = torch.randn(4, V, generator=gen) * 2.5
    lg[0, V - 3] = float(lg[0].max()) + 0.5                          # a unique maximum
    three = torch.tensor([1, V // 2, V - 1])
    lg[1, three] = float(lg[1].max()) + 0.5                          # three equal maxima across the row
    lg[2] = lg[2].half().float()
    lg[2, 5] = float(lg[2].max()) + 1e-3                             # a unique maximum with a close runner-up
    lg[3, 0] = float("-inf")                                         # a -inf logit is legal
    lg[3, 7] = float(lg[3, 1:].max()) + 2.0
    for T in (1.0, 0.7):
        lgn = MR.nudged(lg, T, (1.0,))
        dl = lgn.to(DEV)
        for k, P in ((-1, 1.0), (5, 1.0), (-1, 0.9)):
            got = _minp(ops, V)(dl, T, k, P, 1.0).cpu()
            for r in (0, 2, 3):
                hot = int(lgn[r].argmax())
                assert float(got[r, hot]) == 1.0 and int((got[r] != 0).sum()) == 1, (V, T, k, P, r)
            if P >= 1.0:                                             # (top_p < 1 may cut equal maxima in index order before min-p)
                assert int((got[1] != 0).sum()) == 3
                third = got[1, three]
                assert float((third - torch.tensor(1.0 / 3.0)).abs().max()) <= 2.0 ** -25, third     # 1 ulp of 1/3


# ---- (d) composition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", SMALL_V + LARGE_V)
def test_d_top_k_top_p_and_min_p_compose_in_hf_order(V):
    ops = _ops()
    k = min(50, V - 1)
    flipped = 0
    for T in (1.0, 0.7):
        lg = _block(V, T)
        got = _minp(ops, V)(lg.to(DEV), T, k, 0.9, 0.1).cpu()
        flipped += MR.check(lg, got, T, k, 0.9, 0.1, f"V={V} T={T} k={k} P=0.9 min_p=0.1", flips=2)
    print(f"V={V}: {flipped} rows with a top-p boundary flip")


# ---- (e) small against large --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1000, 32768])
def test_e_large_form_is_bit_identical_to_the_small_one(V):
    ops = _ops()
    for rows in (1, 8):
        dl = _cycled(_block(V, 1.0), rows).to(DEV)
        for T, k, P, m in [(1.0, -1, 1.0, 0.02), (1.0, -1, 1.0, 0.3), (0.7, 50, 0.9, 0.1), (0.6, -1, 0.9, 0.5), (1.0, 5, 1.0, 1.0),
                           (0.6, 50, 0.95, TINY_MIN_P)]:
            assert torch.equal(ops.minp_probs_large(dl, T, k, P, m), ops.minp_probs(dl, T, k, P, m)), (V, rows, T, k, P, m)


# ---- (f) graph replay ---------------------------------------------------------------------------------------------------------
def test_f_twenty_launches_of_each_form_in_one_graph_give_the_eager_results():
    ops = _ops()
    forms = []                                                       # (name, fn, inputs a / b)
    for V, fn in ((32000, ops.minp_probs), (128256, ops.minp_probs_large)):
        gen = torch.Generator().manual_seed(6000 + V)
        a = (torch.randn(3, V, generator=gen) * 2.5).to(DEV)
        b = (torch.randn(3, V, generator=gen) * 0.5).to(DEV)
        b[0, 11] = 30.0
        for k, P, m in ((-1, 1.0, 0.05), (50, 0.9, 0.3)):
            forms.append((f"V={V} k={k} P={P} min_p={m}", (lambda lg, fn=fn, k=k, P=P, m=m: fn(lg, 1.0, k, P, m)), a, b))
    eager = [(f(a), f(b)) for _, f, a, b in forms]                   # (also sizes the _large workspace outside the capture)
    torch.cuda.synchronize()
    outs = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(20):
            outs.append([f((a, b)[i % 2]) for _, f, a, b in forms])
    for _ in range(2):
        for row in outs:
            for o in row:
                o.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        for i, row in enumerate(outs):
            for j, o in enumerate(row):
                assert torch.equal(o, eager[j][i % 2]), f"launch {i} of {forms[j][0]} differs from the eager result"


# ---- (g) the engine -----------------------------------------------------------------------------------------------------------
def _golden(large):
    if not large:
        return dict(Hh.load_golden("small_gamma6"), gen_len=100, budget=320)
    return dict(tcfg=specs.tiny_target_config(vocab_size=128256, max_pos=131072), dcfg=specs.draft_68m_config(vocab_size=128256),
                tseed=1, dseed=2, pseed=3, head_std=0.05, prefill=2048, gen_len=96, budget=256, chunk=8, gamma=6,
                temperature=0.6, top_p=0.9)


_WEIGHTS = {}


def _weights(large):
    if large not in _WEIGHTS:
        g = _golden(large)
        _WEIGHTS[large] = (g, specs.random_state_dict(g["tcfg"], g["tseed"], head_std=g.get("head_std", 0.05)),
                           specs.random_state_dict(g["dcfg"], g["dseed"], head_std=g.get("head_std", 0.05)))
    return _WEIGHTS[large]


def _engine(large, temperature, top_p, min_p, top_k=-1):
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache, StreamingLLMEvictionCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as LlamaForCausalLM_68M
    from triforce_amd.utils.graph_infer import GraphInferenceEngine
    g, tsd, dsd = _weights(large)
    target = LlamaForCausalLM.from_state_dict(LlamaConfig.from_dict(g["tcfg"]), tsd, DEV)
    draft = LlamaForCausalLM_68M.from_state_dict(LlamaConfig.from_dict(g["dcfg"]), dsd, DEV)
    gamma = g["gamma"]
    ge = GraphInferenceEngine(target, FlashSimpleCache(target, g["prefill"] + g["gen_len"] + 16),
                              RetrievalCache(target, max_budget=g["budget"], prefill=g["prefill"], gamma=gamma, chunk_size=g["chunk"]),
                              draft, StreamingLLMEvictionCache(draft, start_size=16, recent_size=256 - 16 - gamma, gamma=gamma))
    ge.initialize_cuda_graph(gamma, probs=True, temperature=temperature, top_p=top_p, verbose=False, top_k=top_k, min_p=min_p)
    return ge


def _runner(g, ge, min_p, temperature, top_p, seed=77, top_k=-1):
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.sampling import UniformSource
    return TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], top_k=top_k, top_p=top_p, temperature=temperature, min_p=min_p,
                          rng=UniformSource(DEV, values=Hh.fixed_uniforms(seed=seed)))


def _stream(ge, g, min_p, temperature, top_p, n, eager_every=0):
    run = _runner(g, ge, min_p, temperature, top_p)
    run.eager_every = eager_every
    run.prefill(Hh.prompt_of(g).to(DEV))
    while run.n < n:
        run.step()
    return list(run.emitted), list(run.counts), run.rng.pos


def _check_captured_rows(lg, got, T, P, min_p, what):
    """The captured verify's probabilities against the reference on the graph's OWN logits.  Those rows cannot be nudged out of
    the guard band, so a row that holds a band entry is compared on its support outside the band only; the others in full."""
    band = MR.in_band(lg, T, min_p)
    clean = ~band.any(-1)
    assert int(clean.sum()) >= 1, f"{what}: every row holds an entry inside the guard band"
    MR.check(lg[clean], got[clean], T, None, P, min_p, what)
    want = MR.minp_f64(lg, T, None, P, min_p)
    assert torch.equal(((got > 0) == (want > 0)) | band, torch.ones_like(band)), f"{what}: support differs outside the guard band"
    return int(clean.sum())


@pytest.mark.parametrize("large", [False, True], ids=["tiny", "tiny-v128k"])
def test_g_captured_target_verify_applies_min_p_and_only_a_matching_runner_uses_it(large, monkeypatch):
    from triforce_amd.utils import decoding as Dm
    from triforce_amd.utils import graph_infer as Gm
    from triforce_amd.utils.decoding import Autoregressive
    from triforce_amd.utils.sampling import UniformSource
    g = _weights(large)[0]
    gamma, T, P, M = g["gamma"], 1.0, 1.0, 0.3
    ge = _engine(large, T, P, M)
    assert ge.target_filters.min_p == M and ge.target_filters.top_k == -1 and "min_p" not in ge.sampling
    prompt = Hh.prompt_of(g).to(DEV)
    run = _runner(g, ge, M, T, P)
    assert run.inner is not None

    def boom(*a, **kw):
        raise AssertionError("the vocabulary was sorted on the host route")
    captures = []
    real_capture = Gm._capture
    if large:
        monkeypatch.setattr(torch, "sort", boom)
        monkeypatch.setattr(torch, "topk", boom)
    run.prefill(prompt)
    monkeypatch.setattr(Gm, "_capture", lambda *a, **kw: (captures.append(1), real_capture(*a, **kw))[1])
    assert run._device_sets() is not None
    while run.n < (32 if large else 24):
        run.step()
    assert not captures, "a graph was captured during the steps"
    assert run._device_sets() is not None and max(run.emitted) < g["tcfg"]["vocab_size"]
    # Autoregressive(min_p=0.3) normalises on the device too: nothing sorts
    calls = []
    real_sort, real_topk = torch.sort, torch.topk
    if not large:
        monkeypatch.setattr(torch, "sort", lambda *a, **kw: (calls.append("sort"), real_sort(*a, **kw))[1])
        monkeypatch.setattr(torch, "topk", lambda *a, **kw: (calls.append("topk"), real_topk(*a, **kw))[1])
    _, toks = Autoregressive(Hh.FakeTokenizer(), ge, prompt, max_len=8, top_p=P, temperature=T, min_p=M,
                             rng=UniformSource(DEV, values=Hh.fixed_uniforms(seed=3)), return_tokens=True)
    assert len(toks) == 9 and not calls, calls
    monkeypatch.undo()
    # verify_probs_ids hands out the graph's out_probs only for the matching (T, top_p, top_k, min_p)
    run = _runner(g, ge, M, T, P)
    run.prefill(prompt)
    checked = 0
    for q_len in (gamma + 1, gamma + 2):
        tg = ge.target_graphs[q_len]
        kv = ge.engine.kv_cache
        S0 = kv.seq_len
        ids = [run.next_token] + [5 + 3 * i for i in range(q_len - 1)]
        assert ge.verify_probs_ids(ids, T, P) is None and ge.verify_probs_ids(ids, T, P, min_p=0.0) is None
        assert ge.verify_probs_ids(ids, T, P, min_p=0.31) is None and ge.verify_probs_ids(ids, T, P, top_k=20, min_p=M) is None
        assert ge.verify_probs_ids(ids, 0.9, P, min_p=M) is None and kv.seq_len == S0
        fast = ge.verify_probs_ids(ids, T, P, min_p=M)
        assert fast is not None and fast[0] is tg.out_probs and fast[1].view(-1).tolist() == ids
        kv.seq_len = S0                                          # (the probe's rows are dropped again)
        checked += _check_captured_rows(tg.logits[0].float().cpu(), tg.out_probs.cpu(), T, P, M, f"captured verify q_len={q_len}")
    assert checked >= 2
    ge.dev_len = None                                            # the probes moved the graphs' device scalars
    # a runner WITHOUT min-p on the same engine: no device-side step, and its verify probabilities are unfiltered
    plain = _runner(g, ge, 0.0, T, P, seed=78)
    plain.prefill(prompt)
    assert plain._device_sets() is None
    seen = []
    real_norm = Dm.norm_logits

    def spy(logits, **kw):
        out = real_norm(logits, **kw)
        seen.append((kw.get("min_p"), int(logits.shape[0]), int((out > 0).sum(-1).min())))
        return out
    monkeypatch.setattr(Dm, "norm_logits", spy)
    plain.step()
    verify = [s for s in seen if s[1] >= gamma + 1]
    assert verify and all(s[0] is None for s in verify), seen
    assert min(s[2] for s in verify) == g["tcfg"]["vocab_size"], f"the min_p=0 runner's verify rows look filtered: {seen}"


def test_g_min_p_session_is_deterministic_and_equals_the_eager_verify_route():
    """Fixed uniforms, a fresh engine each: the min_p = 0.3 session twice, and once with every target verify on the eager route
    (forward + norm_logits -> the same kernel) — identical tokens, accept counts and uniform-stream position."""
    g = _weights(False)[0]
    T, P, M, n = 1.0, 1.0, 0.3, 48
    a = _stream(_engine(False, T, P, M), g, M, T, P, n)
    b = _stream(_engine(False, T, P, M), g, M, T, P, n)
    c = _stream(_engine(False, T, P, M), g, M, T, P, n, eager_every=1)
    assert len(a[1]) >= 8
    assert a == b, f"two identical sessions diverge at token {Hh.common_prefix(a[0], b[0])}"
    assert a[0] == c[0], f"graph and eager verify routes diverge at token {Hh.common_prefix(a[0], c[0])} of {len(a[0])}"
    assert a[1] == c[1] and a[2] == c[2]


@pytest.mark.parametrize("large", [False, True], ids=["tiny", "tiny-v128k"])
def test_g_min_p_1_through_the_on_device_path_emits_the_oracles_greedy_stream(large):
    """min_p = 1 (T = 1, top_p = 1): the target distribution keeps the row maxima only, so whatever the drafts propose the stream
    is the target's greedy stream — every teacher-forced gap within GAP_TOL, at most 2 non-zero (exact fp16 ties between the 1-row
    and the 7-row forward), as tests/test_gpu_topk.py states it for top_k = 1."""
    g, tsd, dsd = _weights(large)
    ge = _engine(large, 1.0, 1.0, 1.0)
    run = _runner(g, ge, 1.0, 1.0, 1.0, seed=5)
    run.prefill(Hh.prompt_of(g).to(DEV))
    assert run._device_sets() is not None
    while run.n < (32 if large else 64):
        run.step()
    stream = list(run.emitted)
    gaps = Hh.teacher_forced_gaps(g, stream, tsd, dsd)
    Hh.note(f"min_p=1 on device (V={g['tcfg']['vocab_size']}): {len(stream)} tokens, max teacher-forced gap {max(gaps):.5f}, "
            f"{sum(1 for x in gaps if x != 0.0)} not the argmax, {run.resample_count} resampled")
    assert max(gaps) <= GAP_TOL, f"token {gaps.index(max(gaps))} trails the target's argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x != 0.0) <= 2
