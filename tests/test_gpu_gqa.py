"""Grouped-query attention on a real MI355X: the four GQA entry points against oracle/ref_ops on the
EXPANDED tensors (K / V heads repeated g times, the reference's repeat_kv), the retrieval build staged as SURVEY section 7
prescribes, and a tiny-gqa-sized target — logits, captured graphs, greedy TriForce, extend() — against the unmodified CPU
oracle run on the expanded multi-head state dict.

Bounds are the project's, restated: split-KV decode attention atol 2e-5 / rtol 1.5e-3 (tests/test_gpu_ops.py DECODE_ATOL /
DECODE_RTOL: P fed as hi + lo fp16, fp32 oracle); logits max(1e-3, 2 fp16 spacings at max |logit|), mean < 1e-3
(tests/test_gpu_e2e.py _logit_check); q|k|v + RoPE the ulp bounds of tests/test_gpu_ops.py test_qkv_rope_fused; retrieval
scores those of test_retrieval_score.  The prefill kernel (tf_attn_prefill's body: P rounded ONCE to fp16, hardware exp2)
keeps the bound the project gives that body, atol 2e-3 / rtol 2e-3 (tests/test_gpu_ops.py ATTN_ATOL / ATTN_RTOL), and is
additionally required to equal tf_attn_prefill on the expanded K / V bit for bit, which no tolerance enters."""
import math

import pytest
import torch

from oracle import ref_model as M
from oracle import ref_ops as R
from oracle import specs
from tests import helpers as Hh
from tests.test_gqa_cpu import gqa_state_dicts

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DECODE_ATOL, DECODE_RTOL = 2e-5, 1.5e-3          # tests/test_gpu_ops.py:146
BLOCK_ATOL, BLOCK_RTOL = 2e-3, 2e-3              # tests/test_gpu_ops.py:140 (the prefill / block kernels)
LOGIT_MEAN_TOL, GAP_TOL = 1e-3, 8e-3             # tests/test_gpu_e2e.py:26-27
# Retrieval scores: test_retrieval_score's rule (<= 1 fp16 ulp, <= 5 % of the elements differing) with its 2e-3 absolute term
# tightened: at this test's shape the measured worst deviation was 4.8e-7, three orders of magnitude inside 2e-3.  What the
# absolute term has to cover is the fp32 summation order of a 128-term dot product near a zero crossing of the score:
# 128 terms x 2^-24 x sum |terms| (~40 for N(0,1) queries against chunk means of 8 N(0,1) keys) ~ 3e-4; 5e-4 covers it.
SCORE_ATOL = 5e-4


def _ops():
    from triforce_amd import ops
    return ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.float16)


def ulp_report(name, got, want, max_ulp_frac, atol=0.0, ulps=1):
    """tests/test_gpu_ops.py ulp_report: at most `max_ulp_frac` of the elements differ, none by more than `ulps` fp16 ulp."""
    got, want = got.float().cpu(), want.float().cpu()
    diff = (got - want).abs()
    ulp = torch.maximum(want.abs(), torch.tensor(6.1e-5)) * 2 ** -10
    bad = diff > (ulp * (ulps + 0.01) + atol)
    frac = (diff > 0).float().mean().item()
    Hh.record("ulp_report", float((diff / (ulp * (ulps + 0.01) + atol)).max()), what=name, max_abs=float(diff.max()),
              mean_abs=float(diff.mean()), ulps=ulps, atol=float(atol), frac_differing=frac, frac_allowed=max_ulp_frac,
              frac_used=frac / max_ulp_frac, max_ref=float(want.abs().max()))
    assert not bad.any(), f"{name}: {int(bad.sum())} elements off by >{ulps} ulp, max diff {diff.max().item():.3e}"
    assert frac <= max_ulp_frac, f"{name}: {frac:.4%} elements differ (allowed {max_ulp_frac:.2%})"


def _logit_check(what, got, want, spacings=2.0):
    d = (got - want).abs()
    mag = max(1.0, float(want.abs().max()))
    bound = max(1e-3, spacings * 2.0 ** (math.floor(math.log2(mag)) - 10))
    Hh.record("logit_check", float(d.max()) / bound, what=what, max_abs=float(d.max()), mean_abs=float(d.mean()), bound=bound,
              mean_bound=LOGIT_MEAN_TOL, mean_used=float(d.mean()) / LOGIT_MEAN_TOL, max_ref=mag, spacings=spacings)
    assert d.max() <= bound and d.mean() < LOGIT_MEAN_TOL, \
        f"{what}: max |dlogit| {d.max():.2e} (bound {bound:.2e}), mean {d.mean():.2e}"


def _expand(x, g, dim):
    return x if g == 1 else x.repeat_interleave(g, dim=dim)


# ---- 1. decode attention ---------------------------------------------------------------------------------------------------
GQA_DECODE_SHAPES = [(4, 1, 128, 7),      # 28 stacked rows: two q-tiles
                     (4, 1, 128, 8),      # exactly 32
                     (8, 1, 128, 7),      # gs = 4: two sub-groups per KV head
                     (2, 1, 128, 8),      # exactly 16: one q-tile, full
                     (8, 2, 64, 1), (8, 2, 64, 3),
                     (2, 1, 128, 17),     # gs = 1
                     (4, 2, 128, 32)]     # gs = 1, 32 rows


def _decode_inputs(H, Hkv, D, sq, sk, cap=None):
    cap = cap or sk
    seed = 1000 + 37 * H + 11 * Hkv + sq + sk
    q, k, v = rnd(sq, H, D, seed=seed), rnd(cap, Hkv, D, seed=seed + 1), rnd(cap, Hkv, D, seed=seed + 2)
    return q, k, v, k.permute(1, 0, 2).contiguous().to(DEV), v.permute(1, 0, 2).contiguous().to(DEV)


@pytest.mark.parametrize("sk_kind", ["sq", 33, 1031, 4103])
@pytest.mark.parametrize("H,Hkv,D,sq", GQA_DECODE_SHAPES)
def test_decode_attention_matches_oracle_on_expanded_kv(H, Hkv, D, sq, sk_kind):
    """Every split count the key count allows, both output layouts, the one- and the two-launch merge (bit-identical), the
    ticket row left zero (a second call on it), rows the call does not own untouched — and the same bits as the
    multi-head kernel on the repeated K / V: stacking rows changes which MFMA column a row sits in, not its arithmetic."""
    ops = _ops()
    sk = sq if sk_kind == "sq" else sk_kind
    assert sk >= sq
    g = H // Hkv
    scale = R.softmax_scale_for(D)
    q, k, v, kd, vd = _decode_inputs(H, Hkv, D, sq, sk)
    want = R.attn_kvcache(q, _expand(k, g, 1), _expand(v, g, 1), scale).reshape(sq, H * D).float()
    qd = q.to(DEV)
    ke, ve = _expand(kd, g, 0).contiguous(), _expand(vd, g, 0).contiguous()
    assert ops.gqa_stack(g, sq)[0] * sq <= 32
    tiles = (sk + 15) // 16
    for nsplit in [n for n in (1, 3, 8, 9) if n <= tiles] + [None]:
        two = ops.attn_decode_gqa(qd, kd, vd, sk, scale, nsplit=nsplit, fused_merge=False)
        Hh.close(two.float().cpu(), want, what=f"gqa decode {H}/{Hkv} D{D} sq{sq} sk{sk} nsplit{nsplit}", atol=DECODE_ATOL,
                 rtol=DECODE_RTOL)
        for _ in range(2):                                    # the second call runs on the tickets the first one left
            one = ops.attn_decode_gqa(qd, kd, vd, sk, scale, nsplit=nsplit, fused_merge=True)
            assert torch.equal(one, two)
        row = ops._ticket_row(qd.device, torch.cuda.current_stream().cuda_stream or 0)
        torch.cuda.synchronize()
        assert int(row.abs().sum()) == 0
        if nsplit is not None:
            mha = ops.attn_decode(qd, ke, ve, sk, scale, nsplit=nsplit)
            assert torch.equal(two, mha), "not the multi-head kernel's bits on the repeated K / V"
        # k-octet-major output with spare rows, row-major output with spare rows: sentinel rows stay
        act = ops.Act.empty(sq, H * D, DEV, R=sq + 3)
        act.t.fill_(-7.0)
        ops.attn_decode_gqa(qd, kd, vd, sk, scale, nsplit=nsplit, out=act)
        assert torch.equal(act.rows(), two) and bool((act.t[:, sq:] == -7.0).all())
        wide = torch.full((sq + 3, H * D), -7.0, dtype=torch.float16, device=DEV)
        ops.attn_decode_gqa(qd, kd, vd, sk, scale, nsplit=nsplit, fused_merge=False, out=wide[:sq])
        assert torch.equal(wide[:sq], two) and bool((wide[sq:] == -7.0).all())


@pytest.mark.parametrize("H,Hkv,D,sq", [(4, 1, 128, 7), (8, 1, 128, 7), (8, 2, 64, 3), (2, 1, 128, 17)])
def test_decode_attention_device_key_count_and_token_major_cache(H, Hkv, D, sq):
    """sk_dev below the launch bound (the captured forward's form) over a token-major cache view with spare capacity."""
    ops = _ops()
    sk, cap, g = 777, 1024, H // Hkv
    scale = R.softmax_scale_for(D)
    q, k, v, _, _ = _decode_inputs(H, Hkv, D, sq, sk, cap=cap)
    kd, vd = k.to(DEV).permute(1, 0, 2), v.to(DEV).permute(1, 0, 2)            # (Hkv, T, D) views of [T][Hkv][D] storage
    want = R.attn_kvcache(q, _expand(k[:sk], g, 1), _expand(v[:sk], g, 1), scale).reshape(sq, H * D).float()
    skd = torch.tensor([sk], dtype=torch.int32, device=DEV)
    for fused in (False, True):
        got = ops.attn_decode_gqa(q.to(DEV), kd, vd, cap, scale, sk_dev=skd, nsplit=4, fused_merge=fused)
        Hh.close(got.float().cpu(), want, what=f"gqa decode sk_dev {H}/{Hkv} sq{sq}", atol=DECODE_ATOL, rtol=DECODE_RTOL)
    got = ops.attn_decode(q.to(DEV), kd, vd, sk, scale)                       # the model's call: dispatch by head counts
    Hh.close(got.float().cpu(), want, what=f"gqa decode dispatch {H}/{Hkv} sq{sq}", atol=DECODE_ATOL, rtol=DECODE_RTOL)


# ---- 2. prefill attention ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 77])
@pytest.mark.parametrize("sq", [33, 129, 300])
@pytest.mark.parametrize("H,Hkv,D", [(4, 2, 128), (8, 1, 64)])
def test_prefill_attention_matches_oracle_and_the_multi_head_kernel(H, Hkv, D, sq, extra):
    """tf_attn_prefill_gqa against the oracle at the bound the project gives tf_attn_prefill's body (P rounded once to fp16:
    atol 2e-3 / rtol 2e-3; measured here: at most 0.29 of it, max |d| 1.95e-3 = one fp16 ulp at |ref| 3.4), and bit for bit
    against tf_attn_prefill on the repeated K / V.  Measured against the split-KV decode kernel's bound (2e-5 / 1.5e-3, P as
    hi + lo) the same outputs use up to 8.5x of it — the multi-head kernel's own figure, since the bits are equal; that
    bound is asserted where it belongs, on tf_attn_decode_gqa_act."""
    ops = _ops()
    sk, g = sq + extra, H // Hkv
    scale = R.softmax_scale_for(D)
    q, k, v, kd, vd = _decode_inputs(H, Hkv, D, sq, sk)
    want = R.attn_kvcache(q, _expand(k, g, 1), _expand(v, g, 1), scale).reshape(sq, H * D).float()
    got = ops.attn_prefill(q.to(DEV), kd, vd, sk, scale)                      # > 32 rows under GQA: tf_attn_prefill_gqa
    Hh.close(got.float().cpu(), want, what=f"gqa prefill {H}/{Hkv} D{D} sq{sq} sk{sk}", atol=BLOCK_ATOL, rtol=BLOCK_RTOL)
    # same launch, same body, only the K / V base differs: tf_attn_prefill on the repeated K / V gives the same bits
    L = ops.hip.lib()
    ke, ve = _expand(kd, g, 0).contiguous(), _expand(vd, g, 0).contiguous()
    nsplit = L.tf_attn_prefill_pick_nsplit(H, sq, sk)
    ws = torch.empty(L.tf_attn_prefill_ws_floats(H, sq, D, nsplit), dtype=torch.float32, device=DEV)
    mha = torch.empty(sq, H * D, dtype=torch.float16, device=DEV)
    st, sh = ke.stride(1), ke.stride(0)
    ops.hip.check(L.tf_attn_prefill(ops._ptr(q.to(DEV)), ops._ptr(ke), ops._ptr(ve), ops._ptr(mha), st, sh, sq, sk, H, D,
                                    float(scale), nsplit, ops._ptr(ws), ws.numel(), ops._stream()), "tf_attn_prefill")
    assert torch.equal(got, mha)


# ---- 3. q|k|v + RoPE + append -------------------------------------------------------------------------------------------------
def _rope_tables(D):
    return R.rope_tables_yarn(D, 4096, 16.0, 256) if D == 128 else R.rope_tables_plain(D, 4096)


@pytest.mark.parametrize("rotate_k", [True, False])
@pytest.mark.parametrize("M", [1, 7, 17])
@pytest.mark.parametrize("H,Hkv,D,K", [(4, 2, 64, 256), (8, 1, 128, 1024)])
def test_rope_append_gqa_bit_exact(H, Hkv, D, K, M, rotate_k):
    ops = _ops()
    T, slot0 = 64, 17
    qkv = rnd(M, (H + 2 * Hkv) * D, seed=6 + M)
    cos, sin = _rope_tables(D)
    pos = torch.randint(0, 4096, (M,), generator=torch.Generator().manual_seed(M))
    q = qkv[:, :H * D].view(M, H, D)
    k = qkv[:, H * D:(H + Hkv) * D].view(M, Hkv, D)
    v = qkv[:, (H + Hkv) * D:].view(M, Hkv, D)
    want_q = R.apply_rope(q, cos, sin, pos)
    want_k = R.apply_rope(k, cos, sin, pos) if rotate_k else k
    for head_major in (True, False):
        if head_major:
            kl = torch.full((Hkv, T, D), -7.0, dtype=torch.float16, device=DEV)
            vl = torch.full((Hkv, T, D), -7.0, dtype=torch.float16, device=DEV)
        else:
            kl = torch.full((T, Hkv, D), -7.0, dtype=torch.float16, device=DEV).permute(1, 0, 2)
            vl = torch.full((T, Hkv, D), -7.0, dtype=torch.float16, device=DEV).permute(1, 0, 2)
        got_q = ops.rope_append(qkv.to(DEV), cos.to(DEV), sin.to(DEV), pos.to(DEV), kl, vl, slot0, H, D, rotate_k=rotate_k,
                                Hkv=Hkv)
        assert torch.equal(got_q.cpu(), want_q)
        assert torch.equal(kl[:, slot0:slot0 + M].permute(1, 0, 2).cpu(), want_k)
        assert torch.equal(vl[:, slot0:slot0 + M].permute(1, 0, 2).cpu(), v)
        for t in (kl, vl):                                   # rows outside the written slots are unchanged
            assert bool((t[:, :slot0] == -7.0).all()) and bool((t[:, slot0 + M:] == -7.0).all())
        sdev = torch.tensor([3], dtype=torch.int32, device=DEV)
        ops.rope_append(qkv.to(DEV), cos.to(DEV), sin.to(DEV), pos.to(DEV), kl, vl, 0, H, D, rotate_k=rotate_k, slot0_dev=sdev,
                        Hkv=Hkv)
        assert torch.equal(kl[:, 3:3 + M].permute(1, 0, 2).cpu(), want_k)


@pytest.mark.parametrize("rotate_k", [True, False])
@pytest.mark.parametrize("M", [1, 7, 17])
@pytest.mark.parametrize("H,Hkv,D,K", [(4, 2, 64, 256), (8, 1, 128, 1024)])
def test_qkv_rope_gqa_fused(H, Hkv, D, K, M, rotate_k):
    """tests/test_gpu_ops.py test_qkv_rope_fused with two head counts: (1) the epilogue alone is bit-exact against the GEMM
    kernel + tf_rope_append_gqa; (2) with the norm prologue, both activation layouts, slot0 and slot0_dev, against the oracle
    pipeline at that test's ulp bounds; cache rows outside the written slots keep their sentinel."""
    ops = _ops()
    eps, slot0, T = 1e-5, 5, 64
    N = (H + 2 * Hkv) * D
    w = rnd(N, K, seed=200 + M, scale=0.05)
    x = rnd(M, K, seed=201)
    ln = (1 + 0.1 * rnd(K, seed=202).float()).half()
    cos, sin = _rope_tables(D)
    pos = torch.randint(0, 4096, (M,), generator=torch.Generator().manual_seed(M))
    pl = ops.PackedLinear(w.to(DEV), rope=(H, Hkv, D))
    assert pl.wp_rope is not None and pl.gqa and pl.wp_rope_n8 is None
    cd, sd, pd = cos.to(DEV), sin.to(DEV), pos.to(DEV)

    def caches():
        return (torch.full((Hkv, T, D), -7.0, dtype=torch.float16, device=DEV),
                torch.full((Hkv, T, D), -7.0, dtype=torch.float16, device=DEV))
    h = ops.rmsnorm(x.to(DEV), ln.to(DEV), eps)
    k1, v1 = caches()
    k2, v2 = caches()
    q1 = ops.qkv_rope(h, pl, None, 0.0, cd, sd, pd, k1, v1, slot0, H, D, rotate_k=rotate_k, Hkv=Hkv)
    q2 = ops.rope_append(ops.linear(h, pl), cd, sd, pd, k2, v2, slot0, H, D, rotate_k=rotate_k, Hkv=Hkv)
    assert torch.equal(q1, q2) and torch.equal(k1, k2) and torch.equal(v1, v2)
    qkv = R.linear(R.rms_norm(x, ln, eps), w)
    wq = R.apply_rope(qkv[:, :H * D].view(M, H, D), cos, sin, pos)
    wk = qkv[:, H * D:(H + Hkv) * D].view(M, Hkv, D)
    wk = R.apply_rope(wk, cos, sin, pos) if rotate_k else wk
    wv = qkv[:, (H + Hkv) * D:].view(M, Hkv, D)
    sdev = torch.tensor([slot0], dtype=torch.int32, device=DEV)
    outs = []
    for packed in (False, True):
        for dev_slot in (False, True):
            k3, v3 = caches()
            xin = ops.Act.from_rows(x.to(DEV)) if packed else x.to(DEV)
            q3 = ops.qkv_rope(xin, pl, ln.to(DEV), eps, cd, sd, pd, k3, v3, 0 if dev_slot else slot0, H, D, rotate_k=rotate_k,
                              slot0_dev=sdev if dev_slot else None, Hkv=Hkv)
            what = "gqa qkv_rope"                            # (one parity-table row per tensor: the worst case over the cases)
            ulp_report(what + " q", q3, wq, max_ulp_frac=8e-2, ulps=2, atol=1e-3)
            ulp_report(what + " k", k3[:, slot0:slot0 + M].permute(1, 0, 2), wk, max_ulp_frac=8e-2, ulps=2, atol=1e-3)
            ulp_report(what + " v", v3[:, slot0:slot0 + M].permute(1, 0, 2), wv, max_ulp_frac=5e-2, ulps=1, atol=1e-4)
            for t in (k3, v3):
                assert bool((t[:, :slot0] == -7.0).all()) and bool((t[:, slot0 + M:] == -7.0).all())
            outs.append((q3, k3, v3))
    for q3, k3, v3 in outs[1:]:                              # the layout and the slot's source change no bit
        assert torch.equal(q3, outs[0][0]) and torch.equal(k3, outs[0][1]) and torch.equal(v3, outs[0][2])


# ---- 4. retrieval build ---------------------------------------------------------------------------------------------------------
def test_retrieval_build_staged():
    """SURVEY section 7's staging: scores from q-bar against the oracle's at the score bound, top-k against the device's own
    scores (tie-tolerant), gathered rows bit-exact given the device's indices, chunk 0 in slot 0."""
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache
    from triforce_amd.models.config_yarn import LlamaConfig
    ops = _ops()
    Hkv, g, D, T, chunk, budget, L = 2, 2, 128, 2048, 8, 256, 2

    class _Model:
        config = LlamaConfig(hidden_size=Hkv * g * D, num_attention_heads=Hkv * g, num_key_value_heads=Hkv, num_hidden_layers=L)
        device = torch.device(DEV)

    kv = FlashSimpleCache(_Model, T + 64)
    kv.k.copy_(rnd(*kv.k.shape, seed=41).to(DEV))
    kv.v.copy_(rnd(*kv.v.shape, seed=42).to(DEV))
    kv.seq_len = T
    rc = RetrievalCache(_Model, max_budget=budget, prefill=T, chunk_size=chunk, gamma=6)
    assert (rc.num_heads, rc.q_heads) == (Hkv, Hkv * g)
    for layer in range(L):
        q = rnd(1, Hkv * g, D, seed=50 + layer)
        rc.init_graph_cache(kv, q.to(DEV), layer)
        qbar = q[0].view(Hkv, g, D).float().mean(dim=1).to(torch.float16)
        assert torch.equal(ops.group_mean_query(q[0].to(DEV), Hkv).cpu(), qbar)
        kl = kv.k[layer].permute(1, 0, 2).cpu()
        want = R.retrieval_scores(kl, qbar, T, chunk)
        dev_scores = rc.last_scores[layer].cpu()
        ulp_report("gqa retrieval scores", dev_scores, want, max_ulp_frac=0.05, atol=SCORE_ATOL)
        idx = rc.last_idx[layer].cpu().long()
        assert R.topk_matches_reference(dev_scores, idx, R.retrieval_topk(dev_scores, rc.select_sets))
        assert bool((idx[:, 0] == 0).all())
        for src, dst in ((kv.k, rc.k), (kv.v, rc.v)):
            full = src[layer].permute(1, 0, 2).cpu()
            assert torch.equal(dst[layer, :, :budget].permute(1, 0, 2).cpu(), R.retrieval_gather(full[:T], idx, chunk))
    assert rc.init_graph


# ---- 5 / 6. model and end to end ------------------------------------------------------------------------------------------------
def _case(**over):
    """A tiny-gqa-sized target (zoo "tiny-gqa": hidden 512, 4 query / 2 KV heads, D = 128, 2 layers) with small_gamma6's draft."""
    g = dict(Hh.load_golden("small_gamma6"))
    tcfg = specs.llama_config(512, 768, 2, 4, vocab_size=g["dcfg"]["vocab_size"], max_position_embeddings=4096,
                              rope_scaling=dict(type="yarn", factor=16.0, original_max_position_embeddings=256),
                              name="tiny-yarn-gqa-target")
    g.update(dict(dict(tcfg=tcfg, tseed=711, prefill=512, gen_len=160, budget=256), **over))
    return g


_WEIGHTS = {}


def _weights(g):
    if "w" not in _WEIGHTS:                                  # drawn once, shared, left unchanged
        gcfg, gsd, esd = gqa_state_dicts(g["tcfg"], g["tseed"], 2)
        dsd = specs.random_state_dict(g["dcfg"], g["dseed"], head_std=g["head_std"])
        _WEIGHTS["w"] = (gcfg, gsd, esd, dsd)
    return _WEIGHTS["w"]


def _product(g, graphs):
    gcfg, gsd, _, dsd = _weights(g)
    return Hh.build_product(dict(g, tcfg=gcfg), DEV, gsd, dsd, graphs=graphs)


def _oracle(g, capacity):
    _, _, esd, _ = _weights(g)
    return M.OracleTarget(g["tcfg"], esd), M.FullCache(g["tcfg"], capacity)


def test_model_logits_eager_and_captured_match_the_expanded_oracle():
    from triforce_amd.utils.sampling import norm_logits
    g = _case()
    gamma = g["gamma"]
    ge = _product(g, graphs=True)
    assert sorted(ge.target_graphs) == sorted({1, gamma + 1, gamma + 2})
    ot, okv = _oracle(g, 512)
    prompt = specs.random_prompt(g["tcfg"]["vocab_size"], 300, g["pseed"])
    lo = ot.forward(prompt, okv, None)
    lp = ge.inference(prompt.to(DEV))                          # chunked prefill: the logits of the reference's last chunk
    keep = lp.shape[1]
    _logit_check("gqa prefill logits", lp.cpu(), lo[:, -keep:])
    kvc = ge.engine.kv_cache
    S = kvc.seq_len
    assert S == 300 and okv.seq_len == 300
    for q_len in (1, gamma + 1, gamma + 2):
        ids = torch.randint(3, g["tcfg"]["vocab_size"], (1, q_len), generator=torch.Generator().manual_seed(q_len))
        want = ot.forward(ids, okv, None)
        okv.seq_len = S
        if q_len == 1:
            eager = ge.engine.model(input_ids=ids.to(DEV), kv_cache=kvc, graph_cache=None).logits.clone()
            kvc.seq_len = S
            captured = ge.decode_step(ids.to(DEV)).clone()
        else:                                   # as test_captured_target_verify_equals_eager: appended rows and probabilities too
            eager = ge.inference(ids.to(DEV), eager=True).clone()
            assert kvc.seq_len == S + q_len
            rows_k = kvc.k[:, :, S:S + q_len].clone()
            kvc.seq_len = S
            kvc.k[:, :, S:S + q_len].zero_()
            captured = ge.inference(ids.to(DEV)).clone()
            dk = (kvc.k[:, :, S:S + q_len].float() - rows_k.float()).abs()
            assert float(dk[0].max()) == 0.0 and float(dk.max()) < 2e-2       # layer 0 rows do not depend on attention
            kvc.seq_len = S
            p_graph = ge.verify_probs(ids.to(DEV), g["temperature"], g["top_p"]).clone()
            p_eager = norm_logits(eager[0], temperature=g["temperature"], top_k=-1, top_p=g["top_p"])
            assert Hh.bound("gqa captured vs eager target verify: probability rows", (p_graph - p_eager).abs().max(), 1e-3)
        assert kvc.seq_len == S + q_len
        kvc.seq_len = S
        _logit_check(f"gqa eager q={q_len}", eager.cpu(), want)
        _logit_check(f"gqa captured q={q_len}", captured.cpu(), want)
        _logit_check(f"gqa captured vs eager q={q_len}", captured.cpu(), eager.cpu())


def _gaps(g, prompt, stream):
    """Teacher-forced gaps through the expanded-MHA oracle (tests/helpers.py teacher_forced_gaps on that state dict)."""
    ot, okv = _oracle(g, prompt.shape[1] + len(stream) + 8)
    logits = ot.forward(prompt, okv, None)[0, -1]
    gaps = [float(logits.max() - logits[stream[0]])]
    for i in range(len(stream) - 1):
        logits = ot.forward(torch.tensor([[stream[i]]]), okv, None)[0, -1]
        gaps.append(float(logits.max() - logits[stream[i + 1]]))
    return gaps


def _check_stream(what, g, prompt, stream):
    gaps = _gaps(g, prompt, stream)
    worst = max(gaps)
    Hh.record("bound", worst / GAP_TOL, what=f"gqa {what}: worst teacher-forced gap", value=worst, limit=GAP_TOL)
    assert worst < GAP_TOL, f"{what}: token {gaps.index(worst)} trails the oracle argmax by {worst:.4f} logit"
    exact = sum(1 for x in gaps if x == 0.0)
    assert exact >= len(gaps) - 3, f"{what}: only {exact}/{len(gaps)} tokens are the oracle's exact argmax"


@pytest.mark.parametrize("graphs", [False, True])
def test_greedy_triforce_and_extend_match_the_expanded_oracle(graphs):
    from triforce_amd.utils.decoding import Autoregressive, TriForceRunner
    g = _case()
    ge = _product(g, graphs=graphs)
    prompt = Hh.prompt_of(g)
    tok = Hh.FakeTokenizer()
    tok.eos_token_id = -1
    _, ar = Autoregressive(tok, ge, prompt.to(DEV), max_len=40, top_k=-1, top_p=g["top_p"], temperature=g["temperature"],
                           return_tokens=True)
    run = TriForceRunner(tok, ge, g["gamma"], top_k=-1, top_p=g["top_p"], temperature=g["temperature"])
    run.prefill(prompt.to(DEV))
    while run.n < 40:
        run.step()
    stream = list(run.emitted)
    assert len(stream) >= 41 and (run.accepted_count > 0 or run.resample_count > 0)
    _check_stream(f"triforce graphs={graphs}", g, prompt, stream)
    _check_stream(f"autoregressive graphs={graphs}", g, prompt, ar)
    n = min(len(ar), len(stream))
    assert Hh.common_prefix(ar[:n], stream[:n]) >= 16
    # a chat turn: [pending] + 64 ids -> a 64-row body through the GQA prefill kernel, the last row alone
    turn = torch.randint(3, g["tcfg"]["vocab_size"], (1, 64), generator=torch.Generator().manual_seed(77))
    run.extend(turn.to(DEV))
    history = torch.cat([prompt, torch.tensor([stream]), turn], dim=1)
    assert torch.equal(run.history.cpu(), history) and run.n == 0
    while run.n < 16:
        run.step()
    _check_stream(f"extend graphs={graphs}", g, history, list(run.emitted))


# ---- 7. ABI ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_head_counts_and_head_dims():
    ops = _ops()
    L = ops.hip.lib()
    buf = torch.zeros(1 << 16, dtype=torch.float16, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    pos = torch.zeros(8, dtype=torch.int64, device=DEV)
    p, w, ps, s = ops._ptr(buf), ops._ptr(ws), ops._ptr(pos), ops._stream()
    for H, Hkv, D in ((8, 3, 128), (4, 2, 96), (2, 4, 128)):
        assert L.tf_attn_decode_gqa_act(p, p, p, p, H * D, 8, D, 4096, 1, 16, None, H, Hkv, D, 0.1, 1, w, ws.numel(), None,
                                        s) == -22
        assert L.tf_attn_prefill_gqa(p, p, p, p, D, 4096, 40, 40, H, Hkv, D, 0.1, 8, w, ws.numel(), s) == -22
        assert L.tf_skinny_qkv_rope_gqa_act(p, p, 64, 8, None, 0.0, None, p, p, ps, p, p, p, D, 4096, 0, None, 1, H, Hkv, D, 64, 1,
                                            s) == -22
        assert L.tf_rope_append_gqa(p, (H + 2 * Hkv) * D, p, p, ps, p, p, p, D, 4096, 0, None, 1, H, Hkv, D, 1, s) == -22
    torch.cuda.synchronize()
