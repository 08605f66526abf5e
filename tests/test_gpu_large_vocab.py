"""Vocabularies above 32 768 on the device: tf_topp_probs_large / tf_topk_topp_probs_large bit for bit
against the <= 32 768 kernels (directly below the limit, through -inf padding above it), against the oracle on dense rows up to
262 144 entries, the streamed slices of the sampling / accept kernels, back-to-back graph replays, and the engine at 128 256."""
import pytest
import torch

from oracle import specs
from tests import helpers as Hh
from tests import large_vocab_ref as LR
from tests import test_gpu_topk as TK

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP_TOL = 8e-3        # as tests/test_gpu_e2e.py: an emitted token may trail the target's argmax by ~2 fp16 spacings
SETTINGS = [(0.6, 0.9), (1.0, 1.0), (1.0, 1e-9), (2.0, 0.999)]
NEG_INF = float("-inf")


def _ops():
    from triforce_amd import ops
    return ops


def _rows11(V, k, seed):
    """The 11 rows of tests/test_gpu_topk.py (dominant token, near-flat, planted ties across rank k, +-0.0) with -inf entries
    planted in four of them (a -inf logit is legal: mass 0)."""
    lg = TK._rows(V, k, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    for r in (0, 4, 5, 9):
        lg[r, torch.randperm(V, generator=gen)[:max(1, V // 16)]] = NEG_INF
    lg[4, 7] = 30.0
    return lg


def _blocks(lg, rows):
    """(rows, V) blocks that together hold every row of ``lg``: consecutive rows, cycled."""
    n = lg.shape[0]
    return [lg[(start + torch.arange(rows)) % n].contiguous() for start in range(0, n, rows)]


# ---- (a) below the old limit: bit-identical to the kernels without _large ----------------------------------------------------
@pytest.mark.parametrize("V", [64, 1000, 4097, 32000, 32768])
def test_large_forms_are_bit_identical_to_the_fused_kernels_up_to_32768(V, monkeypatch):
    ops = _ops()
    monkeypatch.setattr(ops, "TOPP_MULTI", False)               # ops.topp_probs -> tf_topp_probs, one workgroup per row
    for rows in (1, 7, 17, 32):
        for blk in _blocks(_rows11(V, 50, 40 + V), rows):
            dl = blk.to(DEV)
            for T, P in SETTINGS:
                assert torch.equal(ops.topp_probs_large(dl, T, P), ops.topp_probs(dl, T, P)), (V, rows, T, P)
        for k in (1, 2, 50, V - 1, V, V + 5):
            for blk in _blocks(_rows11(V, k, 40 + V), rows):
                dl = blk.to(DEV)
                for T, P in SETTINGS:
                    got, want = ops.topk_topp_probs_large(dl, T, k, P), ops.topk_topp_probs(dl, T, k, P)
                    assert torch.equal(got, want), (V, rows, k, T, P, int((got != want).sum()))


def test_large_forms_take_unaligned_bases(monkeypatch):
    """A base that is only 4-byte aligned (a view one float into a buffer) takes the element path: same bits."""
    ops = _ops()
    monkeypatch.setattr(ops, "TOPP_MULTI", False)
    for V in (32000, 40000):
        lg = _rows11(V, 50, 7)[:3]
        buf = torch.empty(3 * V + 1, device=DEV)
        off = buf[1:].view(3, V)
        off.copy_(lg)
        dl = lg.to(DEV)
        assert off.data_ptr() % 16 == 4 and dl.data_ptr() % 16 == 0
        assert torch.equal(ops.topp_probs_large(off, 0.6, 0.9), ops.topp_probs_large(dl, 0.6, 0.9))
        assert torch.equal(ops.topk_topp_probs_large(off, 0.6, 50, 0.9), ops.topk_topp_probs_large(dl, 0.6, 50, 0.9))


# ---- (b) above the limit: a row padded with -inf gives the established kernel's bits ------------------------------------------
@pytest.mark.parametrize("V", [32769, 32772, 65536, 128256, 262144])
def test_padding_with_minus_inf_leaves_every_bit_of_the_fused_kernels_result(V, monkeypatch):
    """-inf entries carry mass 0 and move neither the maximum, Z, tau nor the k-th value (k <= the count of finite entries), so
    the large kernel on a row embedded in -inf must reproduce tf_topp_probs / tf_topk_topp_probs on the row alone."""
    ops = _ops()
    monkeypatch.setattr(ops, "TOPP_MULTI", False)
    gen = torch.Generator().manual_seed(V)
    for V0 in (1000, 32000):
        for k in (None, 1, 50, V0 - 1, V0):
            small = TK._rows(V0, k or 50, 60 + V0)               # finite everywhere: V0 finite entries per row
            at = int(torch.randint(0, V - V0 + 1, (1,), generator=gen))
            big = torch.full((small.shape[0], V), NEG_INF)
            big[:, at:at + V0] = small
            ds, db = small.to(DEV), big.to(DEV)
            for T, P in SETTINGS:
                if k is None:
                    want, got = ops.topp_probs(ds, T, P), ops.topp_probs_large(db, T, P)
                else:
                    want, got = ops.topk_topp_probs(ds, T, k, P), ops.topk_topp_probs_large(db, T, k, P)
                assert torch.equal(got[:, at:at + V0], want), (V, V0, k, T, P, at)
                assert int(torch.count_nonzero(got)) == int(torch.count_nonzero(want)), (V, V0, k, T, P, at)


# ---- (c) dense rows above the limit against the reference ---------------------------------------------------------------------
# The rules are tests/test_gpu_topk.py's, restated in tests/large_vocab_ref.py::check_rules with the reference handed in:
# support, at most 2 boundary flips within 2e-5 of top_p, row sums within 1e-5, values at rtol 2e-6, the reference's own cumsum
# tail at top_p = 1.  The reference is the oracle where the oracle itself holds those rules against the float64 restatement of
# the same filter (V <= 40 000, no huge tie group), else that float64 restatement: large_vocab_ref.reference_kind has the
# oracle's measured deviation per shape, tests/test_large_vocab_cpu.py keeps the oracle-referenced rows honest.
DENSE_SETTINGS = [(0.6, None, 0.9), (0.6, 50, 0.9), (1.0, None, 1.0)]


@pytest.mark.parametrize("V", [32769, 40000, 128256, 262144])
@pytest.mark.parametrize("rows", [1, 8])
def test_dense_rows_match_the_reference(V, rows):
    ops = _ops()
    for block in LR.dense_specs(rows, 500 + V % 97):
        dl = torch.stack([LR.dense_row(kind, V, seed) for kind, seed in block]).to(DEV)
        for T, k, P in DENSE_SETTINGS:
            got = (ops.topp_probs_large(dl, T, P) if k is None else ops.topk_topp_probs_large(dl, T, k, P)).cpu()
            for r, (kind, seed) in enumerate(block):
                lg, want, which = LR.reference(kind, V, seed, T, k or V, P)
                LR.check_rules(lg, got[r:r + 1], want, T, k or V, P, f"V={V} rows={rows} {kind} T={T} k={k} P={P} vs {which}")


def test_norm_logits_takes_the_large_kernels_and_never_sorts(monkeypatch):
    from triforce_amd.utils.sampling import norm_logits
    ops = _ops()
    dl = (LR.dense_row("sigma2.5", 128256, 3).unsqueeze(0)).to(DEV)
    want_p, want_k = ops.topp_probs_large(dl, 0.6, 0.9), ops.topk_topp_probs_large(dl, 0.6, 20, 0.9)
    small = {V: _rows11(V, 5, 9)[:3].to(DEV) for V in (96, 32772)}       # (built here: _rows11 sorts)

    def boom(*a, **kw):
        raise AssertionError("the vocabulary was sorted")
    monkeypatch.setattr(torch, "sort", boom)
    monkeypatch.setattr(torch, "topk", boom)
    assert torch.equal(norm_logits(dl, temperature=0.6, top_k=-1, top_p=0.9), want_p)
    assert torch.equal(norm_logits(dl, temperature=0.6, top_k=20, top_p=0.9), want_k)
    # more rows than one launch takes: split over launches, same rows
    many = dl.expand(40, -1).contiguous()
    assert torch.equal(norm_logits(many, temperature=0.6, top_k=-1, top_p=0.9), want_p.expand(40, -1))
    # every kernel cell of the dispatch table is the wrapper it names, called directly: 3 rows at V = 96
    # (fused) and at V = 32 772, the smallest multiple of 4 above the fused limit (large)
    T, P = 0.8, 0.95
    for V, large in [(96, ""), (32772, "_large")]:
        lg = small[V]
        for k in (-1, 5):
            for m in (0.0, 0.1):
                if m > 0:
                    want = getattr(ops, "minp_probs" + large)(lg, T, k, P, m)
                elif k > 0:
                    want = getattr(ops, "topk_topp_probs" + large)(lg, T, k, P)
                else:
                    want = getattr(ops, "topp_probs" + large)(lg, T, P)
                assert torch.equal(norm_logits(lg, temperature=T, top_k=k, top_p=P, min_p=m), want), (V, k, m)


# ---- (d) block_sample above the limit -----------------------------------------------------------------------------------------
def _peaked(V, rows, seed):
    """(rows, V) non-negative rows on the CPU, every entry non-zero: a uniform background holding 0.2 of the mass and 40 heavy
    entries of 0.02 each at random places (the decisions land on those: a margin of 1e-2 in cumulative mass)."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.rand(rows, V, generator=gen) * (0.4 / V) + 1e-9
    for r in range(rows):
        p[r, torch.randperm(V, generator=gen)[:40]] = 0.02
    return p


def _offset_copy(t):
    """The same values behind a base that is one float past a 16-byte boundary (the element-by-element path)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _heavy(values, n):
    """Indices of n heavy entries (mass > 4e-4 of the total) spread over the support."""
    v = values.double() / values.double().sum()
    idx = torch.nonzero(v > 4e-4).flatten()
    assert idx.numel() >= n
    return idx[torch.linspace(0, idx.numel() - 1, n).long()].tolist()


@pytest.mark.parametrize("V", [40000, 128256, 262144])
def test_sample_inverse_cdf_streamed_slices(V):
    ops = _ops()
    p = _peaked(V, 1, 11 + V)[0]
    da, do = p.to(DEV), _offset_copy(p.to(DEV))
    assert da.data_ptr() % 16 == 0
    out = torch.zeros(2, dtype=torch.int64, device=DEV)
    for idx in _heavy(p, 6):
        u = LR.uniform_inside(p, idx)
        ref, margin = LR.inverse_cdf_f64(p, u)
        assert ref == idx and margin > 1e-4
        du = torch.tensor([u], dtype=torch.float32, device=DEV)
        ops.sample_inverse_cdf(da, du, out[0:1])
        ops.sample_inverse_cdf(do, du, out[1:2])
        assert out.tolist() == [idx, idx], (V, idx, out.tolist())
    # any uniform: both paths add in the same order, so they agree bit for bit even where float64 would be a coin toss
    for u in torch.rand(16, generator=torch.Generator().manual_seed(V)).tolist() + [0.0, 0.99999994]:
        du = torch.tensor([u], dtype=torch.float32, device=DEV)
        ops.sample_inverse_cdf(da, du, out[0:1])
        ops.sample_inverse_cdf(do, du, out[1:2])
        assert int(out[0]) == int(out[1]), (V, u, out.tolist())


@pytest.mark.parametrize("V", [40000, 128256, 262144])
def test_middle_accept_cur_streamed_slices(V):
    ops = _ops()
    gamma = 3
    p = _peaked(V, gamma + 1, 21 + V)
    q = _peaked(V, 1, 31 + V)[0]
    for n, accept in [(0, True), (1, False), (2, True)]:
        d = _heavy(q, 3)[1]
        q_d = q.clone()
        p_n = p.clone()
        p_n[n, d] = q_d[d] * (4.0 if accept else 0.25)           # ratio 4 (accepted whatever u) or 0.25
        u_acc = 0.5                                              # margin of the accept test: 0.25 either way
        row = p_n[n + (1 if accept else 0)]
        b = _heavy(row, 5)[2 + n % 2]
        u_s = LR.uniform_inside(row, b)
        ref, margin = LR.inverse_cdf_f64(row, u_s)
        assert ref == b and margin > 1e-4
        recs = []
        for conv in (lambda t: t.to(DEV), lambda t: _offset_copy(t.to(DEV))):
            tokens = torch.full((gamma + 2,), 5, dtype=torch.int64, device=DEV)
            tokens[n + 1] = d
            ubuf = torch.tensor([0.123, 0.9, u_acc, u_s, 0.7], dtype=torch.float32, device=DEV)
            cursor = torch.tensor([1], dtype=torch.int64, device=DEV)
            out = torch.zeros(4, dtype=torch.int64, device=DEV)
            ops.middle_accept_cur(conv(p_n), conv(q_d), tokens, ubuf, cursor, n, gamma, out)
            recs.append((out.tolist(), tokens.tolist(), int(cursor)))
        assert recs[0] == recs[1], (V, n, recs)
        assert recs[0][0] == [1 if accept else 0, b, d, 1] and recs[0][2] == 4, (V, n, recs[0])
        assert recs[0][1][n + 1 + (1 if accept else 0)] == b


@pytest.mark.parametrize("V", [40000, 128256, 262144])
def test_accept_chain_step_streamed_slices(V):
    """Reject at position 1 (the residual max(p - q, 0) is sampled: both operands streamed) and accept everything (the bonus row)."""
    ops = _ops()
    g2 = 3
    p0 = _peaked(V, g2 + 1, 41 + V)
    q0 = _peaked(V, g2, 51 + V)
    for reject_at in (1, None):
        p, q = p0.clone(), q0.clone()
        toks = [_heavy(q[i], 4)[1 + i % 2] for i in range(g2)]
        for i, t in enumerate(toks):
            p[i, t] = q[i, t] * (0.25 if i == reject_at else 4.0)
        if reject_at is None:
            count, row = g2, p[g2]
        else:
            count, row = reject_at, (p[reject_at] - q[reject_at]).clamp_min(0.0)       # fp32, as the kernel subtracts
        nxt = _heavy(row, 5)[3]
        u_s = LR.uniform_inside(row, nxt)
        ref, margin = LR.inverse_cdf_f64(row, u_s)
        assert ref == nxt and margin > 1e-4
        examined = count + 1 if reject_at is not None else count
        us = [0.5] * examined + [u_s] + [0.9] * 4
        recs = []
        for conv in (lambda t: t.to(DEV), lambda t: _offset_copy(t.to(DEV))):
            tok_buf = torch.tensor([9] + toks + [0], dtype=torch.int64, device=DEV)
            ubuf = torch.tensor([0.3] + us, dtype=torch.float32, device=DEV)
            cursor = torch.tensor([1], dtype=torch.int64, device=DEV)
            s_src = torch.tensor([100], dtype=torch.int32, device=DEV)
            out = torch.zeros(4, dtype=torch.int64, device=DEV)
            ops.accept_chain_step(conv(p), conv(q), tok_buf, ubuf, cursor, g2, False, 2, 0, s_src, [], out)
            recs.append((out.tolist(), tok_buf.tolist(), int(cursor)))
        assert recs[0] == recs[1], (V, reject_at, recs)
        assert recs[0][0] == [count, nxt, 0 if reject_at is not None else 1, examined + 1], (V, reject_at, recs[0])
        assert recs[0][1][count + 1] == nxt and recs[0][2] == 1 + examined + 1


# ---- (f) replay hygiene -------------------------------------------------------------------------------------------------------
def test_fifty_back_to_back_launches_in_one_graph_give_the_eager_results():
    """50 launches of each form on ONE workspace inside one captured graph, inputs alternating between a sharp row block and a
    dense one: every launch must give what the same call gives eagerly (a workspace left dirty by its predecessor would not)."""
    ops = _ops()
    V = 128256
    a = torch.stack([LR.dense_row(k, V, 70 + i) for i, k in enumerate(("dominant", "ties4096", "sigma1"))]).to(DEV)
    b = torch.stack([LR.dense_row(k, V, 80 + i) for i, k in enumerate(("near_flat", "sigma8", "sigma2.5"))]).to(DEV)
    eager = {}
    for name, lg in (("a", a), ("b", b)):
        eager[name] = (ops.topp_probs_large(lg, 0.6, 0.9), ops.topk_topp_probs_large(lg, 0.6, 50, 0.9))
    torch.cuda.synchronize()
    outs = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(50):
            name, lg = (("a", a), ("b", b))[i % 2]
            outs.append((name, ops.topp_probs_large(lg, 0.6, 0.9), ops.topk_topp_probs_large(lg, 0.6, 50, 0.9)))
    for _ in range(2):
        for _, p, pk in outs:
            p.fill_(-1.0)
            pk.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        for i, (name, p, pk) in enumerate(outs):
            assert torch.equal(p, eager[name][0]), f"launch {i} (top-p) differs from the eager result"
            assert torch.equal(pk, eager[name][1]), f"launch {i} (top-k + top-p) differs from the eager result"


# ---- (e) the engine at 128 256 entries ----------------------------------------------------------------------------------------
def _golden():
    from triforce_amd.models import zoo
    g = dict(tcfg=specs.tiny_target_config(vocab_size=128256, max_pos=131072), dcfg=specs.draft_68m_config(vocab_size=128256),
             tseed=1, dseed=2, pseed=3, head_std=0.05, prefill=2048, gen_len=96, budget=256, chunk=8, gamma=6,
             temperature=0.6, top_p=0.9)
    for cfg, name in ((g["tcfg"], "tiny-v128k"), (g["dcfg"], zoo.draft_for("tiny-v128k"))):     # the zoo's shapes
        z = zoo.config(name)
        for f in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
                  "max_position_embeddings", "rms_norm_eps"):
            assert getattr(z, f) == cfg[f], (name, f)
    return g


@pytest.fixture(scope="module")
def weights():
    g = _golden()
    return g, specs.random_state_dict(g["tcfg"], g["tseed"], head_std=g["head_std"]), \
        specs.random_state_dict(g["dcfg"], g["dseed"], head_std=g["head_std"])


def _engine(weights, temperature, top_p, top_k):
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache, StreamingLLMEvictionCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as LlamaForCausalLM_68M
    from triforce_amd.utils.graph_infer import GraphInferenceEngine
    g, tsd, dsd = weights
    target = LlamaForCausalLM.from_state_dict(LlamaConfig.from_dict(g["tcfg"]), tsd, DEV)
    draft = LlamaForCausalLM_68M.from_state_dict(LlamaConfig.from_dict(g["dcfg"]), dsd, DEV)
    gamma = g["gamma"]
    ge = GraphInferenceEngine(target, FlashSimpleCache(target, g["prefill"] + g["gen_len"] + 16),
                              RetrievalCache(target, max_budget=g["budget"], prefill=g["prefill"], gamma=gamma, chunk_size=g["chunk"]),
                              draft, StreamingLLMEvictionCache(draft, start_size=16, recent_size=256 - 16 - gamma, gamma=gamma))
    ge.initialize_cuda_graph(gamma, probs=True, temperature=temperature, top_p=top_p, verbose=False, top_k=top_k)
    return ge


def _runner(g, ge, top_k, temperature, top_p, seed=77):
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.sampling import UniformSource
    return TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], top_k=top_k, top_p=top_p, temperature=temperature,
                          rng=UniformSource(DEV, values=Hh.fixed_uniforms(seed=seed)))


def _stream(ge, g, top_k, temperature, top_p, n, eager_every=0):
    run = _runner(g, ge, top_k, temperature, top_p)
    run.eager_every = eager_every
    run.prefill(Hh.prompt_of(g).to(DEV))
    while run.n < n:
        run.step()
    return list(run.emitted), list(run.counts), run.rng.pos


@pytest.mark.parametrize("top_k", [-1, 20])
def test_engine_runs_the_captured_path_without_sorting_the_vocabulary(weights, top_k, monkeypatch):
    from triforce_amd.utils import graph_infer as Gm
    g = weights[0]
    gamma, T, P = g["gamma"], 0.6, 0.9
    ge = _engine(weights, T, P, top_k)
    run = _runner(g, ge, top_k, T, P)
    assert run.inner is not None
    prompt = Hh.prompt_of(g).to(DEV)

    def boom(*a, **kw):
        raise AssertionError("the vocabulary was sorted on the host route")
    captures = []
    real_capture = Gm._capture
    monkeypatch.setattr(torch, "sort", boom)
    monkeypatch.setattr(torch, "topk", boom)
    run.prefill(prompt)
    monkeypatch.setattr(Gm, "_capture", lambda *a, **kw: (captures.append(1), real_capture(*a, **kw))[1])
    assert run._device_sets() is not None
    while run.n < 64:
        run.step()
    assert not captures, "a graph was captured during the steps"
    assert run._device_sets() is not None and len(run.emitted) >= 64 and max(run.emitted) < 128256
    monkeypatch.undo()
    # the captured verify's probabilities against the oracle on the graph's OWN logits, under the rules of the dense rows
    K = top_k if top_k > 0 else 128256
    for q_len in (gamma + 1, gamma + 2):
        tg = ge.target_graphs[q_len]
        S0 = ge.engine.kv_cache.seq_len
        ids = [run.next_token] + [5 + 3 * i for i in range(q_len - 1)]
        fast = ge.verify_probs_ids(ids, T, P, top_k=top_k)
        assert fast is not None and fast[0] is tg.out_probs
        ge.engine.kv_cache.seq_len = S0
        lg = tg.logits[0].float().cpu()
        LR.check_rules(lg, tg.out_probs.cpu(), LR.norm_logits_f64(lg, T, K, P), T, K, P, f"captured verify q_len={q_len} vs f64")
    ge.dev_len = None


@pytest.mark.parametrize("top_k", [-1, 20])
def test_engine_session_is_deterministic_and_equals_the_eager_verify_route(weights, top_k):
    """Fixed uniforms, a fresh engine each: the session twice, and once with every target verify on the eager route (forward +
    norm_logits -> the same kernel) — identical tokens, accept counts and uniform-stream position."""
    g = weights[0]
    T, P, n = 0.6, 0.9, 64
    a = _stream(_engine(weights, T, P, top_k), g, top_k, T, P, n)
    b = _stream(_engine(weights, T, P, top_k), g, top_k, T, P, n)
    c = _stream(_engine(weights, T, P, top_k), g, top_k, T, P, n, eager_every=1)
    assert len(a[1]) >= 4
    assert a == b, f"two identical sessions diverge at token {Hh.common_prefix(a[0], b[0])}"
    assert a[0] == c[0], f"graph and eager verify routes diverge at token {Hh.common_prefix(a[0], c[0])} of {len(a[0])}"
    assert a[1] == c[1] and a[2] == c[2]


def test_engine_top_k_1_emits_the_oracles_greedy_stream(weights):
    g = weights[0]
    ge = _engine(weights, 1.0, 1.0, 1)
    run = _runner(g, ge, 1, 1.0, 1.0, seed=5)
    run.prefill(Hh.prompt_of(g).to(DEV))
    assert run._device_sets() is not None
    while run.n < 48:
        run.step()
    stream = list(run.emitted)
    gaps = Hh.teacher_forced_gaps(g, stream, weights[1], weights[2])
    Hh.note(f"V=128256 top_k=1 on device: {len(stream)} tokens, max teacher-forced gap {max(gaps):.5f}, "
            f"{sum(1 for x in gaps if x != 0.0)} not the argmax, {run.resample_count} resampled")
    assert max(gaps) <= GAP_TOL, f"token {gaps.index(max(gaps))} trails the target's argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x != 0.0) <= 2


def test_native_draft_chain_and_python_issued_draft_agree_bit_for_bit(weights, monkeypatch):
    from triforce_amd.models.cache import StreamingLLMEvictionCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as Draft
    g, _, dsd = weights
    gamma, cfg = g["gamma"], LlamaConfig.from_dict(g["dcfg"])

    def run(native):
        monkeypatch.setenv("TRIFORCE_DRAFT_NATIVE", "1" if native else "0")
        m = Draft.from_state_dict(cfg, dsd, DEV)
        c = StreamingLLMEvictionCache(m, start_size=16, recent_size=256 - 16 - gamma, gamma=gamma)
        assert (m._native_model() is not None) == native
        assert m._persist is None                                      # the one-launch form refuses this vocabulary
        gen = torch.Generator().manual_seed(5)
        outs = []
        for n in (20, 1):
            ids = torch.randint(3, cfg.vocab_size, (1, n), generator=gen).to(DEV)
            outs.append(m.forward(ids, c, None, -1).logits)
        for off in range(gamma + 1):
            ids = torch.randint(3, cfg.vocab_size, (1, off + 1), generator=gen).to(DEV)
            o = m.forward(ids, c, c, off, probs=(0.6, 0.9))
            outs += [o.logits, o.probs]
        torch.cuda.synchronize()
        return outs
    a, b = run(True), run(False)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"output {i} differs between the native chain and the Python-issued draft"
    assert all(abs(float(p.sum()) - 1.0) < 1e-5 for p in a[3::2])
