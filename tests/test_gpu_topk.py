"""Device-side top-k for the target tier: tf_topk_topp_probs against the oracle's sort-based norm_logits,
its bit-identity with tf_topp_probs when top_k filters nothing, and the captured target verify / decode loop with top_k > 0."""
import pytest
import torch

from oracle import ref_ops as R
from oracle import specs
from tests import helpers as Hh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP_TOL = 8e-3        # as tests/test_gpu_e2e.py: an emitted token may trail the target's argmax by ~2 fp16 spacings


def _ops():
    from triforce_amd import ops
    return ops


def _rnd(rows, V, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(rows, V, generator=gen)


def _rows(V, k, seed):
    """The 9 rows of tests/test_gpu_ops.py::test_topp_probs_matches_oracle (random * 2.5 — about 20 logit units, no survivor
    underflows —, an fp16-valued row, ties at the top, an all-equal row, one dominant token) and two more that depend on k:
    row 9 has SIX EQUAL VALUES straddling rank k (ranks k-3 .. k+2), row 10 has -0.0 and +0.0 alternating over the same ranks
    (positive values above, negative below), so the k-th value is a zero of either sign."""
    lg = _rnd(11, V, seed) * 2.5
    lg[1] = lg[1].half().float()
    lg[2, :5] = lg[2].max()
    lg[3] = 0.0
    lg[4, 7] = 30.0
    kk = min(k, V)
    lo, hi = max(0, kk - 3), min(V, kk + 3)
    order = torch.sort(lg[9], descending=True, stable=True).indices
    lg[9, order[lo:hi]] = float(lg[9, order[lo]])
    order = torch.sort(lg[10], descending=True, stable=True).indices
    mag = lg[10].abs() + 0.5
    new = torch.empty(V)
    new[order[:lo]] = mag[order[:lo]]
    new[order[hi:]] = -mag[order[hi:]]
    zeros = torch.zeros(hi - lo)
    zeros[1::2] = -0.0
    new[order[lo:hi]] = zeros
    lg[10] = new
    return lg


def _survivors(lg, T, k):
    """The oracle's top-k survivor set, by its own lines (oracle/ref_ops.py norm_logits: ``logits < kth`` is masked)."""
    x = lg / T
    kth = torch.topk(x, min(k, x.size(-1)))[0][:, [-1]]
    return x >= kth


def _check_against_oracle(lg, got, T, k, P, what):
    """Statements (a)-(e) of the kernel's contract for one (rows, V) block; ``lg`` / ``got`` on the CPU."""
    want = R.norm_logits(lg.clone(), T, k, P)
    S = _survivors(lg, T, k)
    assert torch.isfinite(got).all(), what
    dev = float((got.sum(-1) - 1).abs().max())
    assert dev < 1e-5, f"{what}: a row sums to 1 +- {dev:.2e}"                              # (d)
    assert not bool(((got > 0) & ~S).any()), f"{what}: an entry outside the top-k survivor set is non-zero"   # (b)
    if P < 1e-6:                                                                            # (e)
        assert torch.equal(got, want), what
        return
    for r in range(lg.shape[0]):
        sg, sw = got[r] > 0, want[r] > 0
        if P >= 1.0:
            # (a) the top-k set is exact, ties included.  At top_p = 1.0 nothing is cut by top-p, so the kernel's support must BE
            # the survivor set.  The oracle's own support is the survivor set too, except where its fp32 cumsum over the sorted
            # survivors rounds ABOVE 1.0 before the last rank: `cum > top_p` then drops the rest of the tail (measured on these
            # rows: never up to 1 003 survivors, up to 31 543 dropped entries of 32 768 on the dominant-token row).  That is the
            # sort-based route's rounding, not a top-k statement: such a row is compared on the entries the oracle kept, against
            # the kernel's values renormalised over them, at the same bound.
            assert torch.equal(sg, S[r]), f"{what} row {r}: support differs from the survivor set in {int((sg != S[r]).sum())} entries"
            if torch.equal(sw, S[r]):
                Hh.close(got[r], want[r], what=what, rtol=2e-6, atol=1e-9)
            else:
                assert not bool((sw & ~S[r]).any())
                xs = (lg[r] / T).masked_fill(~S[r], float("-inf"))
                order = torch.sort(xs, descending=True, stable=True)
                cum = torch.cumsum(torch.softmax(order.values, -1), -1)                      # the oracle's fp32 cumsum
                first = int(torch.nonzero(cum > P).flatten()[0]) + 1                         # first sorted rank the oracle removed
                dropped = torch.zeros_like(sw)
                dropped[order.indices[first:]] = True
                assert torch.equal(S[r] & ~sw, dropped & S[r]), f"{what} row {r}: oracle and kernel differ beyond the cumsum tail"
                renorm = (got[r].double() / got[r][sw].double().sum()).float()
                Hh.close(renorm[sw], want[r][sw], what=what + " (oracle tail cut by its fp32 cumsum)", rtol=2e-6, atol=1e-9)
            continue
        if torch.equal(sg, sw):
            Hh.close(got[r], want[r], what=what, rtol=2e-6, atol=1e-9)
            continue
        # (c) the kept set may differ only at the top-p boundary, within rounding of top_p in cumulative mass OVER THE SURVIVORS
        diff = torch.nonzero(sg != sw).flatten()
        assert diff.numel() <= 2, f"{what} row {r}: kept sets differ in {diff.numel()} entries"
        p_full = torch.softmax((lg[r] / T).masked_fill(~S[r], float("-inf")), -1)
        order = torch.sort(p_full, descending=True, stable=True)
        cum = torch.cumsum(order.values.double(), 0)
        ranks = {int(t): i for i, t in enumerate(order.indices.tolist())}
        for t in diff.tolist():
            rk = ranks[t]
            before = float(cum[rk - 1]) if rk > 0 else 0.0
            assert abs(before - P) < 2e-5, f"{what} row {r}: token {t} (rank {rk}) flipped far from the boundary ({before} vs {P})"


def _ks(V):
    return sorted(k for k in {1, 2, 50, 1000, V - 1, V, V + 5} if k <= V + 5)


@pytest.mark.parametrize("V", [64, 1000, 4097, 32000, 32768])
def test_topk_topp_probs_matches_oracle(V):
    """tf_topk_topp_probs vs the oracle's norm_logits(lg, T, k, P) (topk + stable sort).  V = 4097 crosses a slab edge and takes
    the non-vector path; k runs from 1 over the planted tie groups to V - 1, V and V + 5 (no top-k).
    (a) top_p = 1.0: the support IS the oracle's survivor set, every entry tied with the k-th value included, values within rtol
        2e-6 — see _check_against_oracle for the rows where the ORACLE's fp32 cumsum cuts its own tail at top_p = 1.0;
    (b) no entry outside the survivor set is ever non-zero;  (c) top_p < 1: at most 2 entries per row differ, each within 2e-5 of
    the boundary in cumulative mass over the survivors;  (d) rows sum to 1 within 1e-5;  (e) top_p = 1e-9: torch.equal."""
    ops = _ops()
    for k in _ks(V):
        lg = _rows(V, k, 90 + V)
        dl = lg.to(DEV)
        for T, P in [(0.6, 0.9), (0.8, 0.95), (1.0, 1.0), (1.0, 1e-9)]:
            got = ops.topk_topp_probs(dl, T, k, P).cpu()
            _check_against_oracle(lg, got, T, k, P, f"V={V} k={k} T={T} P={P}")


@pytest.mark.parametrize("rows", [1, 7, 8, 33])
def test_no_top_k_is_bit_identical_to_topp_probs_and_rows_are_independent(rows, monkeypatch):
    ops = _ops()
    monkeypatch.setattr(ops, "TOPP_MULTI", False)               # the one-workgroup-per-row tf_topp_probs
    for V in (4097, 32000):
        lg = (_rnd(rows, V, 700 + rows) * 2.5).half().float()
        if rows > 2:
            lg[1] = 0.0
            lg[2, 100:120] = lg[2].max() + 6.0
        dl = lg.to(DEV)
        for T, P in [(0.6, 0.9), (1.0, 1.0), (1.0, 1e-9)]:
            want = ops.topp_probs(dl, T, P)
            for k in (V, V + 5):
                assert torch.equal(ops.topk_topp_probs(dl, T, k, P), want), (rows, V, T, P, k)
        # a row's result does not depend on its neighbours: the same row alone and inside the block (a real top-k: 50)
        block = ops.topk_topp_probs(dl, 0.8, 50, 0.95)
        for r in sorted({0, rows // 2, rows - 1}):
            alone = ops.topk_topp_probs(dl[r:r + 1].clone(), 0.8, 50, 0.95)
            assert torch.equal(alone[0], block[r]), (rows, V, r)


def _golden(**over):
    return dict(Hh.load_golden("small_gamma6"), **dict(dict(gen_len=100, budget=320), **over))


def _engine(g, temperature, top_p, top_k):
    """helpers.build_product by hand, with ``top_k`` for the captured target verifies."""
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache, StreamingLLMEvictionCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as LlamaForCausalLM_68M
    from triforce_amd.utils.graph_infer import GraphInferenceEngine
    tsd = specs.random_state_dict(g["tcfg"], g["tseed"], head_std=g.get("head_std", 0.05))
    dsd = specs.random_state_dict(g["dcfg"], g["dseed"], head_std=g.get("head_std", 0.05))
    target = LlamaForCausalLM.from_state_dict(LlamaConfig.from_dict(g["tcfg"]), tsd, DEV)
    draft = LlamaForCausalLM_68M.from_state_dict(LlamaConfig.from_dict(g["dcfg"]), dsd, DEV)
    gamma = g["gamma"]
    ge = GraphInferenceEngine(target, FlashSimpleCache(target, g["prefill"] + g["gen_len"] + 16),
                              RetrievalCache(target, max_budget=g["budget"], prefill=g["prefill"], gamma=gamma, chunk_size=g["chunk"]),
                              draft, StreamingLLMEvictionCache(draft, start_size=16, recent_size=256 - 16 - gamma, gamma=gamma))
    ge.initialize_cuda_graph(gamma, probs=True, temperature=temperature, top_p=top_p, verbose=False, top_k=top_k)
    return ge


@pytest.fixture(scope="module")
def engine20():
    g = _golden()
    return g, _engine(g, 0.8, 0.95, 20)


def _runner(g, ge, top_k, temperature, top_p, seed=77):
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.sampling import UniformSource
    return TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], top_k=top_k, top_p=top_p, temperature=temperature,
                          rng=UniformSource(DEV, values=Hh.fixed_uniforms(seed=seed)))


def test_captured_target_verify_applies_top_k_and_only_a_matching_runner_uses_it(engine20, monkeypatch):
    from triforce_amd.utils import decoding as Dm
    from triforce_amd.utils import graph_infer as Gm
    g, ge = engine20
    gamma, T, P, K = g["gamma"], 0.8, 0.95, 20
    assert ge.target_filters.top_k == K and "top_k" not in ge.sampling
    prompt = Hh.prompt_of(g).to(DEV)
    run = _runner(g, ge, K, T, P)
    assert run.inner is not None
    captures = []
    real_capture = Gm._capture
    monkeypatch.setattr(Gm, "_capture", lambda *a, **kw: (captures.append(1), real_capture(*a, **kw))[1])
    run.prefill(prompt)
    assert run._device_sets() is not None
    for _ in range(4):
        run.step()
    assert not captures, "a graph was captured during the steps"
    assert run._device_sets() is not None
    # the on-device step replayed the captured verify: its probabilities against the oracle on the graph's OWN logits
    checked = 0
    for q_len in (gamma + 1, gamma + 2):
        tg = ge.target_graphs[q_len]
        kv = ge.engine.kv_cache
        S0 = kv.seq_len
        ids = [run.next_token] + [5 + 3 * i for i in range(q_len - 1)]
        assert ge.verify_probs_ids(ids, T, P) is None and ge.verify_probs_ids(ids, T, P, top_k=0) is None
        assert ge.verify_probs_ids(ids, T, P, top_k=K + 1) is None and kv.seq_len == S0
        fast = ge.verify_probs_ids(ids, T, P, top_k=K)
        assert fast is not None and fast[0] is tg.out_probs and fast[1].view(-1).tolist() == ids
        kv.seq_len = S0                                          # (the probe's rows are dropped again)
        _check_against_oracle(tg.logits[0].float().cpu(), tg.out_probs.cpu(), T, K, P, f"captured verify q_len={q_len}")
        checked += 1
    assert checked == 2
    ge.dev_len = None                                            # the probes moved the graphs' device scalars
    # a runner WITHOUT top-k on the same engine: no device-side step, and its verify probabilities carry no top-k
    plain = _runner(g, ge, -1, T, P, seed=78)
    plain.prefill(prompt)
    assert plain._device_sets() is None
    seen = []
    real_norm = Dm.norm_logits

    def spy(logits, **kw):
        out = real_norm(logits, **kw)
        seen.append((kw.get("top_k"), int(logits.shape[0]), int((out > 0).sum(-1).max())))
        return out
    monkeypatch.setattr(Dm, "norm_logits", spy)
    plain.step()
    verify = [s for s in seen if s[1] >= gamma + 1]
    assert verify and all(s[0] == -1 for s in verify), seen
    # (a top-k filtered row keeps 20 entries plus ties; this near-flat random model keeps hundreds at top_p = 0.95)
    assert max(s[2] for s in verify) > 2 * K, f"the top_k=-1 runner's verify rows look top-k filtered: {seen}"
    assert ge.verify_probs_ids([1] * (gamma + 1), T, P, top_k=-1) is None


def _stream(ge, g, top_k, temperature, top_p, n, eager_every=0):
    run = _runner(g, ge, top_k, temperature, top_p)
    run.eager_every = eager_every
    run.prefill(Hh.prompt_of(g).to(DEV))
    while run.n < n:
        run.step()
    return list(run.emitted), list(run.counts), run.rng.pos


def test_top_k_session_is_deterministic_and_equals_the_eager_verify_route():
    """Fixed uniforms: the top_k=20 session twice (a fresh engine each: a second prompt on one engine legitimately differs, SURVEY
    section 7), and the same runner with every target verify on the eager route (forward + norm_logits -> the same kernel):
    identical tokens, accept counts and uniform-stream position."""
    g = _golden()
    T, P, K, n = 0.8, 0.95, 20, 48
    a = _stream(_engine(g, T, P, K), g, K, T, P, n)
    b = _stream(_engine(g, T, P, K), g, K, T, P, n)
    c = _stream(_engine(g, T, P, K), g, K, T, P, n, eager_every=1)
    assert len(a[1]) >= 8
    assert a == b, f"two identical sessions diverge at token {Hh.common_prefix(a[0], b[0])}"
    assert a[0] == c[0], f"graph and eager verify routes diverge at token {Hh.common_prefix(a[0], c[0])} of {len(a[0])}"
    assert a[1] == c[1] and a[2] == c[2]


def _teacher_forced_logits(g, stream):
    """The CPU oracle's logits row in front of every token of ``stream`` (helpers.teacher_forced_gaps, keeping the rows)."""
    eng, _, _ = Hh.build_oracle(g)
    eng.kv_cache.reset()
    rows = [eng.inference(Hh.prompt_of(g))[0, -1]]
    for i in range(len(stream) - 1):
        rows.append(eng.model.forward(torch.tensor([[stream[i]]]), eng.kv_cache, None)[0, -1])
    return rows


@pytest.mark.parametrize("top_k", [1, 3])
def test_top_k_through_the_on_device_path_is_lossless_and_keeps_the_support(top_k):
    """top_k = 1 (T = 1, top_p = 1): the target distribution is one-hot up to exact fp16 ties, so whatever the drafts propose the
    stream is the target's greedy stream — every teacher-forced gap within GAP_TOL, at most 2 non-zero (tests/test_session_cpu.py).
    top_k = 3: every emitted token's oracle logit is at least the third-largest oracle logit at its position minus GAP_TOL."""
    g = _golden()
    ge = _engine(g, 1.0, 1.0, top_k)
    run = _runner(g, ge, top_k, 1.0, 1.0, seed=5)
    run.prefill(Hh.prompt_of(g).to(DEV))
    assert run._device_sets() is not None
    while run.n < 64:
        run.step()
    stream = list(run.emitted)
    rows = _teacher_forced_logits(g, stream)
    if top_k == 1:
        gaps = [float(r.max() - r[t]) for r, t in zip(rows, stream)]
        Hh.note(f"top_k=1 on device: {len(stream)} tokens, max teacher-forced gap {max(gaps):.5f}, "
                f"{sum(1 for x in gaps if x != 0.0)} not the argmax, {run.resample_count} resampled")
        assert max(gaps) <= GAP_TOL, f"token {gaps.index(max(gaps))} trails the target's argmax by {max(gaps):.4f}"
        assert sum(1 for x in gaps if x != 0.0) <= 2
    else:
        short = [float(torch.topk(r, 3).values[-1] - r[t]) for r, t in zip(rows, stream)]
        Hh.note(f"top_k=3 on device: {len(stream)} tokens, worst distance below the third-largest logit {max(short):.5f}, "
                f"{len(set(stream))} distinct tokens")
        assert max(short) <= GAP_TOL, f"token {short.index(max(short))} lies {max(short):.4f} below the third-largest logit"


def test_autoregressive_with_top_k_never_sorts_the_vocabulary(engine20, monkeypatch):
    from triforce_amd.utils.decoding import Autoregressive
    from triforce_amd.utils.sampling import UniformSource
    g, ge = engine20
    calls = []
    real_sort, real_topk = torch.sort, torch.topk
    monkeypatch.setattr(torch, "sort", lambda *a, **kw: (calls.append("sort"), real_sort(*a, **kw))[1])
    monkeypatch.setattr(torch, "topk", lambda *a, **kw: (calls.append("topk"), real_topk(*a, **kw))[1])
    _, toks = Autoregressive(Hh.FakeTokenizer(), ge, Hh.prompt_of(g).to(DEV), max_len=16, top_k=20, top_p=0.95, temperature=0.8,
                             rng=UniformSource(DEV, values=Hh.fixed_uniforms(seed=3)), return_tokens=True)
    assert len(toks) == 17 and not calls, calls
