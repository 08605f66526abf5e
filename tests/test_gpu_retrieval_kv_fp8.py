"""FP8 storage of the retrieval cache on a real MI355X (TRIFORCE_RETRIEVAL_KV=fp8).

The row format is that of the FP8 full cache (include/triforce_hip.h "FP8 KV CACHE"): dequantization is exact in fp16, so every
kernel has a plain oracle.  The attention over codes followed by fp16 rows against the fp16 kernel on [deq(codes) | rows] and
against the all-codes FP8 kernel (torch.equal); the gather and the tail refresh against the host restatement of the quantizer, or
against the source bytes when the source holds codes.  The engine: only the spec forward changes, it reads what the cache says
it stores, and greedy TriForce stays the target's own continuation — at the tiny sizes and at full 7B size."""
import math

import pytest
import torch

from tests import helpers as Hh
from tests.test_gpu_reanchor import _golden, _lossless, _question, _set_path, _steps

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ENV = "TRIFORCE_RETRIEVAL_KV"
GAP_TOL = 8e-3        # as tests/test_gpu_e2e.py: an emitted token may trail the target's argmax by ~2 fp16 spacings
GREEDY = dict(top_k=-1, top_p=1e-9, temperature=1.0)
D = 128
SENTINEL = 0xA5


def _ops():
    from triforce_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _planes(shape, seed, lo=-26, hi=17):
    """fp16 K and V of ``shape`` (..., T, D) whose rows span the exponents of the contract, with all-zero rows."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for _ in range(2):
        x = torch.randn(*shape, device=DEV, generator=g)
        mag = torch.randint(lo, hi, (*shape[:-1], 1), device=DEV, generator=g).float()
        x = (x * torch.pow(2.0, mag)).clamp(-65504, 65504)
        x[..., ::97, :] = 0
        out.append(x.half())
    return out


def _f8(*shape, fill=0):
    """(k codes, v codes, k exponents, v exponents) of (..., T, D) / (..., T), every byte ``fill``."""
    kc = torch.full((*shape, D), fill, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)
    ke = torch.full(shape, fill, dtype=torch.uint8, device=DEV)
    return kc, kc.clone(), ke, ke.clone()


# =====================================================================================================================
# 1. attention: codes then fp16 rows in one launch
# =====================================================================================================================
_ATTN = {}


def _attn_cache():
    """32 heads x 12 288 coded keys (scores of a sane magnitude, row scales over several exponents), their deq, and 32 fp16
    tail rows per head; built once and left unchanged."""
    if not _ATTN:
        ops = _ops()
        H, T = 32, 12288
        g = torch.Generator(device=DEV).manual_seed(11)
        k = (torch.randn(H, T, D, device=DEV, generator=g) *
             torch.pow(2.0, torch.randint(-5, 1, (H, T, 1), device=DEV, generator=g).float())).half()
        v = (torch.randn(H, T, D, device=DEV, generator=g) *
             torch.pow(2.0, torch.randint(-12, 5, (H, T, 1), device=DEV, generator=g).float())).half()
        kc, vc, ke, ve = _f8(H, T)
        ops.kv_quant_rows(k, v, kc, vc, ke, ve, 0, deq=True)          # k, v now hold deq
        tk = (torch.randn(H, 32, D, device=DEV, generator=g) * 0.4).half()
        tv = (torch.randn(H, 32, D, device=DEV, generator=g) * 3.0).half()
        _ATTN["c"] = (kc, vc, ke, ve, k, v, tk, tv)
    return _ATTN["c"]


def _forms(skc, n):
    """(nsplit, fused merge, packed): the default split in both merges and layouts, and forced splits — for the short
    streams one tile per split (a split of tail rows alone; a split that is the tile straddling the boundary) and two
    splits (the first ends on the straddling tile when sk_codes is mid-tile); for the real budgets 3 and 13 (more than the
    one-launch merge folds)."""
    tiles = (skc + n + 15) // 16
    forms = [(None, True, False), (None, False, True)]
    if skc < 4096:
        forms += [(s, f, p) for s, f, p in ((tiles, True, True), (2, False, False)) if 1 < s <= tiles]
    else:
        forms += [(3, True, True), (13, False, False), (13, True, True)]
    return forms


@pytest.mark.parametrize("H", [1, 5, 32])
@pytest.mark.parametrize("skc", [8, 16, 24, 40, 4096, 12288])
def test_attention_is_bit_identical_to_fp16_on_deq_then_tail(skc, H, monkeypatch):
    ops = _ops()
    kc, vc, ke, ve, kd, vd, tk, tv = (t[:H] for t in _attn_cache())
    scale = 1.0 / math.sqrt(D)
    g = torch.Generator(device=DEV).manual_seed(100 * skc + H)
    n_cases = 0
    for n in (1, 7, 16, 17, 18, 32):                                # n_tail = sq
        q = torch.randn(n, H, D, device=DEV, generator=g).half()
        kf = torch.cat([kd[:, :skc], tk[:, :n]], dim=1)
        vf = torch.cat([vd[:, :skc], tv[:, :n]], dim=1)
        for nsplit, fused, packed in _forms(skc, n):
            monkeypatch.setattr(ops, "ATTN_FUSED_MERGE", fused)
            a = ops.attn_decode(q, kf, vf, skc + n, scale, nsplit=nsplit, packed=packed)
            b = ops.attn_decode_fp8_tail(q, kc, vc, ke, ve, tk, tv, skc, scale, n_tail=n, nsplit=nsplit, packed=packed)
            ta, tb = (a.t, b.t) if packed else (a, b)
            assert torch.isfinite(tb.float()).all()
            assert torch.equal(ta, tb), f"sk_codes {skc} n_tail {n} H {H} nsplit {nsplit} fused {fused} packed {packed}"
            n_cases += 1
    Hh.note(f"retrieval fp8 attention sk_codes={skc} H={H}: {n_cases} shapes/forms bit-identical to tf_attn_decode_act")


def test_attention_rendezvous_merge_and_strided_tail(monkeypatch):
    """The in-launch merge of more than 8 splits (off by default, tf_attn_tune), and tail rows that are a strided view (the
    layer slice of the cache's [L][H][gamma + 1][D] array is contiguous; a longer row array is not)."""
    from triforce_amd import hip
    ops = _ops()
    kc, vc, ke, ve, kd, vd, tk, tv = (t[:5] for t in _attn_cache())
    scale, skc, n = 1.0 / math.sqrt(D), 4096, 17
    q = torch.randn(n, 5, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)).half()
    kf, vf = torch.cat([kd[:, :skc], tk[:, 9:9 + n]], dim=1), torch.cat([vd[:, :skc], tv[:, 9:9 + n]], dim=1)
    tks, tvs = tk[:, 9:9 + n], tv[:, 9:9 + n]
    assert not tks.is_contiguous()
    old = hip.lib().tf_attn_tune(0, 1)
    try:
        for nsplit in (None, 32):
            a = ops.attn_decode(q, kf, vf, skc + n, scale, nsplit=nsplit, packed=True)
            b = ops.attn_decode_fp8_tail(q, kc, vc, ke, ve, tks, tvs, skc, scale, nsplit=nsplit, packed=True)
            assert torch.equal(a.t, b.t), nsplit
    finally:
        hip.lib().tf_attn_tune(0, old)


@pytest.mark.parametrize("skc,n,H", [(24, 17, 5), (40, 32, 1), (4096, 7, 32), (12288, 17, 32)])
def test_attention_equals_the_all_codes_kernel_when_the_tail_is_representable(skc, n, H):
    """Tail rows set to deq(quantize(rows)): the output also equals tf_attn_decode_fp8_act over storage that holds those rows
    as codes — the new form is section 17's kernel with another source for its last rows."""
    ops = _ops()
    kc, vc, ke, ve, _, _, tk, tv = (t[:H] for t in _attn_cache())
    kc2, vc2, ke2, ve2 = _f8(H, skc + n)
    for dst, src in ((kc2, kc), (vc2, vc), (ke2, ke), (ve2, ve)):
        dst[:, :skc] = src[:, :skc]
    tkd, tvd = tk[:, :n].clone(), tv[:, :n].clone()
    ops.kv_quant_rows(tkd, tvd, kc2, vc2, ke2, ve2, skc, deq=True)   # tkd / tvd now hold deq of the codes at [skc, skc + n)
    assert not torch.equal(tkd, tk[:, :n])
    scale = 1.0 / math.sqrt(D)
    q = torch.randn(n, H, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)).half()
    for nsplit, packed in ((None, False), (None, True), (2, True)):
        a = ops.attn_decode_fp8(q, kc2, vc2, ke2, ve2, skc + n, scale, nsplit=nsplit, packed=packed)
        b = ops.attn_decode_fp8_tail(q, kc, vc, ke, ve, tkd, tvd, skc, scale, nsplit=nsplit, packed=packed)
        assert torch.equal(a.t, b.t) if packed else torch.equal(a, b), (nsplit, packed)


def test_attention_refuses_bad_shapes():
    from triforce_amd import hip
    ops = _ops()
    kc, vc, ke, ve = _f8(2, 64)
    rows = torch.zeros(2, 40, D, dtype=torch.float16, device=DEV)
    q = torch.zeros(7, 2, D, dtype=torch.float16, device=DEV)
    with pytest.raises(hip.TriforceHipError):
        ops.attn_decode_fp8_tail(q, kc, vc, ke, ve, rows, rows, 64, 0.1)          # 40 tail rows
    with pytest.raises(IndexError):
        ops.attn_decode_fp8_tail(q, kc, vc, ke, ve, rows[:, :7], rows[:, :7], 65, 0.1)   # more coded keys than the layer holds
    with pytest.raises(IndexError):
        ops.attn_decode_fp8_tail(q, kc, vc, ke, ve, rows[:, :7], rows[:, :7], 64, 0.1, n_tail=8)


# =====================================================================================================================
# 2. gather
# =====================================================================================================================
def _planted_idx(H, C, sets, seed):
    """Chunk 0 in slot 0, then distinct chunks in no order (what the top-k hands over)."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for _ in range(H):
        p = torch.randperm(C - 1, generator=g)[:sets - 1] + 1
        rows.append(torch.cat([torch.zeros(1, dtype=torch.long), p]))
    idx = torch.stack(rows)
    assert bool((idx[:, 1:-1] > idx[:, 2:]).any()) and bool((idx[:, 1:-1] < idx[:, 2:]).any())
    return idx.to(torch.int32).to(DEV)


@pytest.mark.parametrize("H", [2, 32])
def test_gather_from_fp16_rows_and_from_codes(H):
    ops = _ops()
    chunk, C, sets = 8, 61, 13
    T = C * chunk + 3
    k, v = _planes((H, T, D), seed=50 + H)
    # strided source: rows [5, 5 + T) of a longer layer
    kb, vb = torch.zeros(H, T + 9, D, dtype=torch.float16, device=DEV), torch.zeros(H, T + 9, D, dtype=torch.float16, device=DEV)
    kb[:, 5:5 + T], vb[:, 5:5 + T] = k, v
    idx = _planted_idx(H, C, sets, seed=52)
    R = sets * chunk
    kc, vc, ke, ve = _f8(H, R + 7, fill=SENTINEL)
    ops.retrieval_gather_fp8(kb[:, 5:5 + T], vb[:, 5:5 + T], idx, kc, vc, ke, ve, chunk)
    torch.cuda.synchronize()
    want = ops.retrieval_gather_fp8_ref(k, v, idx, chunk)
    for got, ref in zip((kc, vc, ke, ve), want):
        assert torch.equal(_bits(got[:, :R]), _bits(ref)), "gather from fp16 differs from the host restatement"
        assert bool((_bits(got[:, R:]) == SENTINEL).all()), "wrote past the gathered rows"
    assert int(ke[:, :R].min()) == 127 - 15 and int(ke[:, :R].max()) > 127

    # from codes: the bytes of the source rows the index names
    sk_, sv_, sek, sev = _f8(H, T + 9)
    ops.kv_quant_rows(k, v, sk_, sv_, sek, sev, 5)
    kc2, vc2, ke2, ve2 = _f8(H, R + 7, fill=SENTINEL)
    ops.retrieval_gather_fp8(sk_[:, 5:], sv_[:, 5:], idx, kc2, vc2, ke2, ve2, chunk, src_exp=(sek[:, 5:], sev[:, 5:]))
    torch.cuda.synchronize()
    rows = (idx.long().unsqueeze(-1) * chunk + torch.arange(chunk, device=DEV)).reshape(H, -1) + 5
    for got, src in ((kc2, sk_), (vc2, sv_)):
        assert torch.equal(_bits(got[:, :R]), _bits(src).gather(1, rows.unsqueeze(-1).expand(-1, -1, D)))
        assert bool((_bits(got[:, R:]) == SENTINEL).all())
    for got, src in ((ke2, sek), (ve2, sev)):
        assert torch.equal(got[:, :R], src.gather(1, rows)) and bool((got[:, R:] == SENTINEL).all())
    # ... which are the codes the fp16 route produced from the same rows
    assert torch.equal(_bits(kc2[:, :R]), _bits(kc[:, :R])) and torch.equal(ve2[:, :R], ve[:, :R])
    with pytest.raises(IndexError):
        ops.retrieval_gather_fp8(k, v, idx, kc[:, :R - 1], vc[:, :R - 1], ke, ve, chunk)


# =====================================================================================================================
# 3. tail refresh
# =====================================================================================================================
@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("n", [0, 1, 9, 300])
def test_tail_refresh_into_codes_from_both_sources(n, L):
    ops = _ops()
    H, Ts, Td, s0, d0 = 3, 400, 340, 37, 29
    k, v = _planes((L, H, Ts, D), seed=60 + L)
    # fp16 -> codes, through layer slices of taller tensors (strides of a real cache's kc[layers])
    big = _f8(L + 1, H, Td, fill=SENTINEL)
    dst = tuple(t[1:] for t in big)
    ops.kv_quant_rows_pair(k, v, *dst, s0, d0, n)
    torch.cuda.synchronize()
    if n:
        rk, rke, _ = ops.kv_quantize_ref(k[:, :, s0:s0 + n])
        rv, rve, _ = ops.kv_quantize_ref(v[:, :, s0:s0 + n])
        for got, ref in zip(dst, (rk, rv, rke, rve)):
            assert torch.equal(_bits(got[:, :, d0:d0 + n]), _bits(ref)), "refresh from fp16 differs from the host restatement"
    for got in big:
        keep = _bits(got).clone()
        keep[1:, :, d0:d0 + n] = SENTINEL
        assert bool((keep == SENTINEL).all()), "wrote outside rows [dst_t0, dst_t0 + n)"

    # codes -> codes
    src = _f8(L, H, Ts)
    for l in range(L):
        ops.kv_quant_rows(k[l], v[l], src[0][l], src[1][l], src[2][l], src[3][l], 0)
    big2 = _f8(L + 1, H, Td, fill=SENTINEL)
    dst2 = tuple(t[1:] for t in big2)
    ops.kv_quant_rows_pair(src[0], src[1], *dst2, s0, d0, n, src_exp=(src[2], src[3]))
    torch.cuda.synchronize()
    for got, s in zip(dst2, src):
        assert torch.equal(_bits(got[:, :, d0:d0 + n]), _bits(s[:, :, s0:s0 + n]))
    for got in big2:
        keep = _bits(got).clone()
        keep[1:, :, d0:d0 + n] = SENTINEL
        assert bool((keep == SENTINEL).all())
    if n:
        with pytest.raises(IndexError):
            ops.kv_quant_rows_pair(k, v, *dst, Ts - n + 1, d0, n)
        with pytest.raises(IndexError):
            ops.kv_quant_rows_pair(k, v, *dst, s0, Td - n + 1, n)


class _M:
    """The geometry a cache constructor reads from a model."""

    def __init__(self, L, H):
        class config:
            num_hidden_layers, num_attention_heads, num_key_value_heads, hidden_size = L, H, H, H * D
        self.config, self.device = config, torch.device(DEV)


@pytest.mark.parametrize("rc_fp8", [False, True], ids=["fp16rc", "fp8rc"])
@pytest.mark.parametrize("kv_fp8", [False, True], ids=["fp16kv", "fp8kv"])
def test_tail_plan_replays_after_seq_len_advanced(kv_fp8, rc_fp8):
    """RetrievalCache.update_graph_cache over a resident full cache, all four (full tier, retrieval tier) pairs: one launch
    plan, replayed as the tail grows (codes -> fp16 rows has no plan: values only); and the single-layer refresh of a rebuild,
    which takes the unplanned call.  An fp16 retrieval cache holds the full cache's fp16 rows, or the deq of its codes, bit for
    bit; an FP8 one the full cache's codes, or the quantizer's host restatement of its fp16 rows."""
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache
    ops = _ops()
    L, H, P, B = 3, 2, 64, 32
    m = _M(L, H)
    kv = FlashSimpleCache(m, P + B, kv_dtype="fp8" if kv_fp8 else "fp16")
    rc = RetrievalCache(m, max_budget=B, prefill=P, chunk_size=8, gamma=6, kv_dtype="fp8" if rc_fp8 else "fp16")
    k, v = _planes((L, H, P + B, D), seed=70)
    if kv_fp8:
        for l in range(L):
            ops.kv_quant_rows(k[l], v[l], *kv.layer_codes(l), 0)
    else:
        kv.k.copy_(k)
        kv.v.copy_(v)
    if not rc_fp8 and kv_fp8:                                        # rows [0, P + 31) of kv.dequantize(l, P + 31), per layer
        deq = [kv.dequantize(l, P + 31) for l in range(L)]
        want = tuple(torch.stack([d[i] for d in deq]) for i in range(2))
    elif not rc_fp8:
        want = (kv.k, kv.v)
    elif kv_fp8:
        want = (kv.kc, kv.vc, kv.ke, kv.ve)
    else:
        want = (*ops.kv_quantize_ref(k)[:2], *ops.kv_quantize_ref(v)[:2])
        want = (want[0], want[2], want[1], want[3])
    held = (rc.kc, rc.vc, rc.ke, rc.ve) if rc_fp8 else (rc.k[:, :, :B], rc.v[:, :, :B])
    plans = []
    for g in (5, 12, 31):
        kv.seq_len = P + g
        rc.update_graph_cache(kv)
        torch.cuda.synchronize()
        plans.append(rc._tail_plan[1] if rc_fp8 or not kv_fp8 else None)
        for got, w in zip(held, want):
            assert torch.equal(_bits(got[:, :, B - g:]), _bits(w[:, :, P:P + g])), g
    assert plans[0] is plans[1] is plans[2] and (plans[0] is None) == (kv_fp8 and not rc_fp8)
    assert int(_bits(held[0][:, :, 0]).max()) == 0                   # row 0: never in a tail of <= 31 rows
    rc.reset()
    kv.seq_len = P + 7
    rc._copy_tail(kv, slice(1, 2))
    torch.cuda.synchronize()
    assert torch.equal(_bits(held[0][1, :, B - 7:]), _bits(want[0][1, :, P:P + 7]))
    assert int(_bits(held[0][0]).max()) == 0 and int(_bits(held[0][2]).max()) == 0
    kv.seq_len = P + B + 1
    with pytest.raises(IndexError, match="retrieval budget"):
        rc.update_graph_cache(kv)


def test_tail_refresh_from_the_offloading_cache_mirror():
    """OffloadingFlashSimpleCache.tail_source: fp16 rows of the device mirror, first row 0."""
    from triforce_amd.models.cache import OffloadingFlashSimpleCache, RetrievalCache
    ops = _ops()
    L, H, P, B = 2, 2, 64, 32
    m = _M(L, H)
    kv = OffloadingFlashSimpleCache(m, P + B)
    kv.set_tail(P, B)
    k, v = _planes((L, H, B, D), seed=71)
    kv.tail_k.copy_(k)
    kv.tail_v.copy_(v)
    rc = RetrievalCache(m, max_budget=B, prefill=P, chunk_size=8, gamma=6, kv_dtype="fp8")
    kv.seq_len = P + 9
    rc.update_graph_cache(kv)
    torch.cuda.synchronize()
    rk, rke, _ = ops.kv_quantize_ref(k[:, :, :9])
    assert torch.equal(_bits(rc.kc[:, :, B - 9:]), _bits(rk)) and torch.equal(rc.ke[:, :, B - 9:], rke)
    assert torch.equal(rc.ve[:, :, B - 9:], ops.kv_quantize_ref(v[:, :, :9])[1])


# =====================================================================================================================
# 4. the engine
# =====================================================================================================================
def _engine(g, monkeypatch, on, graphs=False, tsd=None, dsd=None):
    if on:
        monkeypatch.setenv(ENV, "fp8")
    else:
        monkeypatch.delenv(ENV, raising=False)
    ge = Hh.build_product(g, DEV, tsd, dsd, graphs=graphs)
    assert ge.engine.graph_cache.fp8 == on
    return ge


def _small():
    """small_gamma6 with head_dim 128 (256 hidden = 2 heads x 128), its own prefill / budget (1 000 / 128)."""
    import copy
    g = copy.deepcopy(Hh.load_golden("small_gamma6"))
    g["tcfg"]["num_attention_heads"] = g["tcfg"]["num_key_value_heads"] = 2
    return g


@pytest.mark.parametrize("kv_fp8", [False, True], ids=["fp16kv", "fp8kv"])
def test_knob_changes_only_the_spec_forward(kv_fp8, monkeypatch):
    """Knob on vs off from the same weights: prefill logits, the target verify's logits and appended full-cache rows and the
    AR step are bit-identical, and both builds select the same chunks.  The cache then holds what the contract says: codes
    of the selected source rows (copied from an FP8 full cache, quantized from an fp16 one) and of the generated tail."""
    ops = _ops()
    g = _small()
    if kv_fp8:
        monkeypatch.setenv("TRIFORCE_KV_CACHE", "fp8")
    oeng, tsd, dsd = Hh.build_oracle(g)
    ge0 = _engine(g, monkeypatch, False, tsd=tsd, dsd=dsd)
    ge1 = _engine(g, monkeypatch, True, tsd=tsd, dsd=dsd)
    prompt = Hh.prompt_of(g).to(DEV)
    outs = []
    for ge in (ge0, ge1):
        kv = ge.engine.kv_cache
        assert kv.fp8 == kv_fp8
        ge.inference(prompt[:, :-1])
        lp = ge.inference(prompt[:, -1:])
        S = kv.seq_len
        ids = torch.randint(3, g["tcfg"]["vocab_size"], (1, g["gamma"] + 1), generator=torch.Generator().manual_seed(4)).to(DEV)
        lv = ge.inference(ids, eager=True)
        planes = (kv.kc, kv.vc, kv.ke, kv.ve) if kv_fp8 else (kv.k, kv.v)
        rows = [_bits(t[:, :, :S + ids.shape[1]]).clone() for t in planes]
        la = ge.inference(ids[:, :1])
        outs.append((lp, lv, rows, la, S))
    (lp0, lv0, rows0, la0, S0), (lp1, lv1, rows1, la1, S1) = outs
    assert S0 == S1
    assert torch.equal(lp0, lp1) and torch.equal(lv0, lv1) and torch.equal(la0, la1)
    assert all(torch.equal(a, b) for a, b in zip(rows0, rows1))
    rc0, rc1, kv = ge0.engine.graph_cache, ge1.engine.graph_cache, ge1.engine.kv_cache
    B, P, cs = rc1.max_budget, rc1.prefill, rc1.chunk_size
    R = B - 2 * cs                                         # (the AR step rebuilt the cache and refreshed a tail of < 2 chunks)
    for l in range(rc1.layers):
        assert torch.equal(rc0.last_idx[l], rc1.last_idx[l]) and torch.equal(rc0.last_scores[l], rc1.last_scores[l])
        idx = rc1.last_idx[l][:, :R // cs].contiguous()
        if kv_fp8:                                         # codes copied: byte-equal to indexing the source
            rws = (idx.long().unsqueeze(-1) * cs + torch.arange(cs, device=DEV)).reshape(rc1.num_heads, -1)
            for got, src in ((rc1.kc[l], kv.kc[l]), (rc1.vc[l], kv.vc[l])):
                assert torch.equal(_bits(got[:, :R]), _bits(src).gather(1, rws.unsqueeze(-1).expand(-1, -1, D)))
            assert torch.equal(rc1.ke[l, :, :R], kv.ke[l].gather(1, rws)) and torch.equal(rc1.ve[l, :, :R], kv.ve[l].gather(1, rws))
            # ... so the middle tier reads exactly the deq the fp16-storage retrieval cache was handed
            dk, dv = rc1.dequantize(l)
            assert torch.equal(dk[:, :B], rc0.k[l, :, :B]) and torch.equal(dv[:, :B], rc0.v[l, :, :B])
        else:
            want = ops.retrieval_gather_fp8_ref(kv.k[l], kv.v[l], idx, cs)
            for got, ref in zip(rc1.layer_codes(l), want):
                assert torch.equal(_bits(got[:, :R]), _bits(ref))
    # the tail refresh after the verify + AR rows above
    n = kv.seq_len - P
    assert n == g["gamma"] + 2
    ge1.update_graph_cache()
    torch.cuda.synchronize()
    if kv_fp8:
        assert torch.equal(_bits(rc1.kc[:, :, B - n:]), _bits(kv.kc[:, :, P:P + n])) and torch.equal(rc1.ve[:, :, B - n:], kv.ve[:, :, P:P + n])
    else:
        assert torch.equal(_bits(rc1.kc[:, :, B - n:]), _bits(ops.kv_quantize_ref(kv.k[:, :, P:P + n])[0]))
        assert torch.equal(rc1.ve[:, :, B - n:], ops.kv_quantize_ref(kv.v[:, :, P:P + n])[1])
    for name in ("k", "v"):
        with pytest.raises(AttributeError, match=ENV):
            getattr(rc1, name)


def test_spec_logits_match_a_torch_forward_over_deq_codes_then_fp16_tail(monkeypatch):
    """The spec forward against the oracle's forward whose retrieval K / V are deq(codes) of the product's cache followed by
    the fp16 rows the forward appends: within the spec-logit bound of the fp16 tier (tests/test_gpu_e2e._logit_check)."""
    from tests.test_gpu_e2e import _logit_check
    g = _small()
    oeng, tsd, dsd = Hh.build_oracle(g)
    ge0 = _engine(g, monkeypatch, False, tsd=tsd, dsd=dsd)
    ge1 = _engine(g, monkeypatch, True, tsd=tsd, dsd=dsd)
    prompt = Hh.prompt_of(g)
    for ge in (ge0, ge1):
        ge.inference(prompt[:, :-1].to(DEV))
        ge.inference(prompt[:, -1:].to(DEV))
    oeng.inference(prompt[:, :-1])
    oeng.inference(prompt[:, -1:])
    og, pg = oeng.graph_cache, ge1.engine.graph_cache
    B, gamma = pg.max_budget, g["gamma"]
    for l in range(pg.layers):                              # the oracle reads what the product's cache stores
        dk, dv = pg.dequantize(l)
        og.key_cache[l, :B] = dk[:, :B].permute(1, 0, 2).cpu()
        og.value_cache[l, :B] = dv[:, :B].permute(1, 0, 2).cpu()
    vt = torch.tensor([[11, 12, 13] + [100] * (gamma - 2)])
    So = oeng.kv_cache.seq_len
    pos = torch.arange(So, So + gamma + 1).unsqueeze(0)

    def spec(ge):
        e = ge.engine
        return e.model(input_ids=vt.to(DEV), kv_cache=e.kv_cache, graph_cache=e.graph_cache, position_ids=pos.to(DEV),
                       spec=True).logits.cpu()
    sp8, sp16 = spec(ge1), spec(ge0)
    assert torch.equal(spec(ge1), sp8)
    assert not torch.equal(sp8, sp16), "the FP8 storage was not exercised"
    want = oeng.model.forward(vt, oeng.kv_cache, og, position_ids=pos, spec=True)
    _logit_check("retrieval-kv fp8 spec logits vs torch on deq(codes) | fp16 tail", sp8, want)
    # the rows the forward appended are the fp16 rows of the fp16-storage run, bit for bit (same weights, same inputs)
    s = ge0.engine.graph_cache.spec_slot
    assert torch.equal(pg.spec_k[0], ge0.engine.graph_cache.k[0, :, s:]) and torch.equal(pg.spec_v[0], ge0.engine.graph_cache.v[0, :, s:])


def test_captured_retrieval_verify_rows_are_the_eager_spec_distribution(monkeypatch):
    from triforce_amd.utils.sampling import norm_logits
    g = _small()
    ge = _engine(g, monkeypatch, True, graphs=True)
    prompt = Hh.prompt_of(g).to(DEV)
    ge.inference(prompt[:, :-1])
    ge.inference(prompt[:, -1:])
    S = ge.engine.kv_cache.seq_len
    gamma = g["gamma"]
    ids = torch.randint(3, g["tcfg"]["vocab_size"], (1, gamma + 1), generator=torch.Generator().manual_seed(6)).to(DEV)
    pos = torch.arange(S, S + gamma + 1, device=DEV).unsqueeze(0)
    rows = ge.graph_verify(ids, pos).clone()
    logits = ge.engine.model_verify(ids, pos, probs=False)
    want = norm_logits(logits[0], temperature=g["temperature"], top_k=-1, top_p=g["top_p"])
    assert torch.equal(rows.reshape(want.shape), want)


# ---- greedy losslessness: every token within GAP_TOL of the target's own AR argmax, all but <= 2 exactly it (_lossless) ----
# Seed: tests/test_gpu_reanchor.py's (small_gamma6 weights, prompt seed 203, prefill 128, budget 64, head_dim 128); the
# fp16-storage run meets the condition for it — the knob-off case below is that check, on the same settings.
def _run_plain(g, monkeypatch, on, graphs, kv_fp8, w_fp8, n=56):
    from triforce_amd.utils.decoding import TriForceRunner
    _set_path(monkeypatch, "on_device" if graphs else "eager", kv_fp8)
    if w_fp8:
        monkeypatch.setenv("TRIFORCE_RETRIEVAL_WEIGHTS", "fp8")
    else:
        monkeypatch.delenv("TRIFORCE_RETRIEVAL_WEIGHTS", raising=False)
    ge = _engine(g, monkeypatch, on, graphs=graphs)
    assert ge.engine.kv_cache.fp8 == kv_fp8 and ge.engine.model.weights.fp8_active() == w_fp8
    doc = Hh.prompt_of(g).to(DEV)
    run = TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], **GREEDY)
    assert (run.inner is not None) == graphs
    run.prefill(doc)
    stream = _steps(run, n)[:n + 5]
    return ge, run, doc, stream


@pytest.mark.parametrize("kv_fp8", [False, True], ids=["fp16kv", "fp8kv"])
def test_the_seed_meets_the_argmax_condition_with_fp16_storage(kv_fp8, monkeypatch):
    g = _golden(True)
    ge, run, doc, stream = _run_plain(g, monkeypatch, False, True, kv_fp8, False)
    _lossless(f"retrieval-kv fp16 storage, kv_fp8={kv_fp8}", ge.engine.model, doc, stream, g, kv_fp8)


@pytest.mark.parametrize("w_fp8", [False, True], ids=["fp16w", "fp8w"])
@pytest.mark.parametrize("kv_fp8", [False, True], ids=["fp16kv", "fp8kv"])
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_greedy_triforce_is_lossless_small(graphs, kv_fp8, w_fp8, monkeypatch):
    g = _golden(True)
    ge, run, doc, stream = _run_plain(g, monkeypatch, True, graphs, kv_fp8, w_fp8)
    assert len(stream) >= 57 and (run.accepted_count > 0 or run.resample_count > 0)
    _lossless(f"retrieval-kv fp8 graphs={graphs} kv_fp8={kv_fp8} w_fp8={w_fp8}", ge.engine.model, doc, stream, g, kv_fp8)


def test_rebuild_every_is_lossless_and_rebuilds_codes(monkeypatch):
    from triforce_amd.utils.decoding import TriForce
    ops = _ops()
    g = _golden(True)
    _set_path(monkeypatch, "on_device")
    ge = _engine(g, monkeypatch, True, graphs=True)
    doc = Hh.prompt_of(g).to(DEV)
    res = TriForce(Hh.FakeTokenizer(), ge, doc, gamma=g["gamma"], max_len=40, return_details=True, rebuild_every=2, **GREEDY)
    _lossless("retrieval-kv fp8 rebuild_every=2", ge.engine.model, doc, res["tokens"], g, False)
    rc, kv = ge.engine.graph_cache, ge.engine.kv_cache
    gen, cs = kv.seq_len - rc.prefill, rc.chunk_size
    keep = min(rc.select_sets, (rc.max_budget - gen) // cs)            # sets not overwritten by the generated tail
    assert keep >= 1
    for layer in (0, rc.layers - 1):
        idx = rc.last_idx[layer][:, :keep].contiguous()
        want = ops.retrieval_gather_fp8_ref(kv.k[layer], kv.v[layer], idx, cs)
        for got, ref in zip(rc.layer_codes(layer), want):
            assert torch.equal(_bits(got[:, :keep * cs]), _bits(ref))


def test_reanchor_crosses_the_budget_losslessly(monkeypatch):
    from triforce_amd.utils.decoding import TriForceRunner
    g = _golden(True)
    _set_path(monkeypatch, "on_device")
    ge = _engine(g, monkeypatch, True, graphs=True)
    kv, rc = ge.engine.kv_cache, ge.engine.graph_cache
    doc = Hh.prompt_of(g).to(DEV)
    run = TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], reanchor_at=48, **GREEDY)
    run.prefill(doc)
    while run.n < 120:
        run.step()
        assert rc.prefill % 8 == 0 and kv.seq_len - rc.prefill + g["gamma"] + 2 <= 64
    assert run.reanchors >= 2 and rc.prefill > rc.prefill0
    _lossless("retrieval-kv fp8 reanchor_at=48, 120 tokens", ge.engine.model, doc, list(run.emitted), g, False)


def test_session_ask_keep_is_lossless(monkeypatch):
    from triforce_amd.utils.decoding import TriForceSession
    g = _golden(True)
    _set_path(monkeypatch, "on_device")
    ge = _engine(g, monkeypatch, True, graphs=True)
    doc, q = Hh.prompt_of(g).to(DEV), _question(g, 12, 32)
    s = TriForceSession(Hh.FakeTokenizer(), ge, g["gamma"], **GREEDY)
    s.prefill(doc)
    s.generate(10)
    st = s.ask(q, 24, keep=g["prefill"])
    assert ge.engine.graph_cache.prefill == g["prefill"]
    _lossless("retrieval-kv fp8 ask(keep=P)", ge.engine.model, torch.cat([doc, q], dim=1), st["tokens"], g, False)


def test_full_scale_7b_greedy_triforce_is_the_exact_ar_argmax(monkeypatch):
    """configs[1] shape: 7B width, 124 928-token prefix, budget 4 096, gamma 6, hipGraphs, random weights.  A few decode steps;
    every emitted token is the argmax of the target's own AR steps over the same cache.  The retrieval cache takes <= 0.52 x
    the fp16 K + V (0.505 x by arithmetic)."""
    import argparse
    import bench
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.sampling import UniformSource
    monkeypatch.setenv(ENV, "fp8")
    args = argparse.Namespace(target="llama-7B-128K", prefill=124928, budget=4096, chunk_size=8, gamma=6, temp=1.0,
                              top_p=1e-9, gen_cap=256, seed=0, no_graphs=False)
    dev = torch.device(DEV)
    target, draft = bench.load_models(args, dev, "random", "random:1", "random:2")
    ge = bench.build_engine(args, dev, target, draft)
    rc = ge.engine.graph_cache
    assert rc.fp8
    fp16_bytes = 2 * rc.layers * rc.num_heads * rc.real_budget * rc.head_dim * 2
    assert rc.nbytes() <= 0.52 * fp16_bytes, (rc.nbytes(), fp16_bytes)
    tcfg, _ = bench.target_config(args.target)
    ids = torch.randint(3, tcfg.vocab_size, (1, args.prefill), generator=torch.Generator().manual_seed(0)).to(dev)
    run = TriForceRunner(bench._Tok(), ge, args.gamma, top_k=-1, top_p=args.top_p, temperature=args.temp,
                         rng=UniformSource(dev, seed=0))
    bench.do_prefill(run, ge, ids, "synthetic")
    eng = ge.engine
    P = eng.kv_cache.seq_len
    while run.n < 8:
        run.step()
    stream = list(run.emitted)
    assert len(stream) >= 9 and eng.kv_cache.seq_len == P + run.n
    eng.kv_cache.seq_len = P
    gaps = []
    for i in range(len(stream) - 1):                       # teacher-forced target (full-cache forward)
        tok = torch.tensor([[stream[i]]], device=dev)
        logits = eng.model(input_ids=tok, kv_cache=eng.kv_cache, graph_cache=None).logits[0, -1]
        gaps.append(float(logits.max() - logits[stream[i + 1]]))
    Hh.note(f"retrieval-kv fp8 full 7B: cache {rc.nbytes() / 2**30:.3f} GiB vs fp16 {fp16_bytes / 2**30:.3f} GiB, "
            f"{len(gaps)} tokens, max gap {max(gaps):.5f}, accepted {run.accepted_count}")
    assert all(x == 0.0 for x in gaps), f"token {next(i for i, x in enumerate(gaps) if x) + 1} is not the AR argmax: {gaps}"
    del ge, run, eng, rc, target, draft
    torch.cuda.empty_cache()
