"""FP8 storage of the target's full KV cache on a real MI355X (TRIFORCE_KV_CACHE=fp8).

The contract (include/triforce_hip.h "FP8 KV CACHE") makes dequantization exact in fp16, so every FP8 kernel has a plain
oracle: the quantizer is checked bit for bit against the host restatement ops.kv_quantize_ref, and the FP8 attention, the
FP8 -> fp16 row copy and the retrieval build against the existing fp16 kernels run on the dequantized cache (torch.equal).
The engine: a forward through an FP8 cache against an fp64 restatement over the K / V it stored, eager == captured, and
greedy TriForce lossless with respect to the FP8-KV target, at the tiny sizes and at full 7B size."""
import math

import pytest
import torch

from tests import helpers as Hh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ENV = "TRIFORCE_KV_CACHE"
GAP_TOL = 8e-3        # as tests/test_gpu_e2e.py: an emitted token may trail the target's argmax by ~2 fp16 spacings
D = 128


def _ops():
    from triforce_amd import ops
    return ops


def _planes(H, T, seed):
    """(H, T, D) fp16 K and V on the device whose rows span every exponent of the contract (row magnitudes 2^-26 .. 2^17,
    a few all-zero rows, saturating rows included)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for _ in range(2):
        x = torch.randn(H, T, D, device=DEV, generator=g)
        mag = torch.randint(-26, 17, (H, T, 1), device=DEV, generator=g).float()
        x = (x * torch.pow(2.0, mag)).clamp(-65504, 65504)
        x[:, ::97] = 0
        out.append(x.half())
    return out


def _f8_layer(H, T):
    f8 = torch.float8_e4m3fn
    return (torch.zeros(H, T, D, dtype=f8, device=DEV), torch.zeros(H, T, D, dtype=f8, device=DEV),
            torch.zeros(H, T, dtype=torch.uint8, device=DEV), torch.zeros(H, T, dtype=torch.uint8, device=DEV))


def _bits(t):
    return t.view(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the quantizer
# ---------------------------------------------------------------------------------------------------------------------
def test_quantizer_matches_the_host_restatement_on_every_fp16_value_and_exponent():
    """All 63 488 finite fp16 values, each in rows built to land on every exponent from -15 to 7 (the row's max picks e;
    the other 127 values of the row are the fp16 values under test, scaled into range or saturating)."""
    ops = _ops()
    allv = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    allv = allv[torch.isfinite(allv)].to(DEV)
    rows = []
    for e in list(range(-15, 8)) + [None]:
        # every finite value that fits under the row maximum 448 * 2^e (that row then takes exponent e); None: all values
        # unscaled behind a 65504 lead (saturation at e = 7)
        lead = torch.tensor(65504.0 if e is None else 448.0 * 2.0 ** e, device=DEV).half()
        vals = allv if e is None else allv[allv.abs() <= lead]
        n = (vals.numel() + 126) // 127
        pad = torch.zeros(n * 127, dtype=torch.float16, device=DEV)
        pad[:vals.numel()] = vals
        r = torch.cat([lead.expand(n, 1), pad.view(n, 127)], dim=1)
        rows.append(r)
    x = torch.cat(rows)                                            # (R, 128)
    R = x.shape[0]
    H = 1
    k = x.view(H, R, D).contiguous()
    v = (-x).view(H, R, D).contiguous()
    kc, vc, ke, ve = _f8_layer(H, R + 5)
    ops.kv_quant_rows(k, v, kc, vc, ke, ve, 5)
    torch.cuda.synchronize()
    for src, codes, ex in ((k, kc, ke), (v, vc, ve)):
        rc, re_, rd = ops.kv_quantize_ref(src[0])
        assert torch.equal(_bits(codes[0, 5:]), _bits(rc)), "codes differ from the host restatement"
        assert torch.equal(ex[0, 5:], re_), "exponents differ from the host restatement"
    assert int(ke[0, 5:].min()) == 127 - 15 and int(ke[0, 5:].max()) == 127 + 7
    Hh.note(f"fp8 kv quantizer: {R} rows x 128 (every finite fp16 value at every exponent) bit-identical to the host")


@pytest.mark.parametrize("device_slot", [False, True])
def test_quantizer_random_rows_slots_and_deq_write_back(device_slot):
    ops = _ops()
    H, T, n, slot = 32, 4200, 29, 4103
    k0, v0 = _planes(H, n, seed=3)
    # strided input rows: (H, n, D) views of a (n, H, D) buffer (the staging of a real forward is (H, 32, D))
    kb, vb = k0.permute(1, 0, 2).contiguous(), v0.permute(1, 0, 2).contiguous()
    k, v = kb.permute(1, 0, 2), vb.permute(1, 0, 2)
    kc, vc, ke, ve = _f8_layer(H, T)
    sd = torch.tensor([slot], dtype=torch.int32, device=DEV) if device_slot else None
    ops.kv_quant_rows(k, v, kc, vc, ke, ve, 0 if device_slot else slot, slot0_dev=sd, deq=True)
    torch.cuda.synchronize()
    for src, out, codes, ex in ((k0, k, kc, ke), (v0, v, vc, ve)):
        rc, re_, rd = ops.kv_quantize_ref(src)
        assert torch.equal(_bits(codes[:, slot:slot + n]), _bits(rc))
        assert torch.equal(ex[:, slot:slot + n], re_)
        assert torch.equal(out, rd), "deq write-back differs from the host dequantization"
        assert int(_bits(codes[:, :slot]).max()) == 0 and int(_bits(codes[:, slot + n:]).max()) == 0, "wrote outside the rows"


# ---------------------------------------------------------------------------------------------------------------------
# 2. the FP8 decode attention == the fp16 kernel on the dequantized cache
# ---------------------------------------------------------------------------------------------------------------------
_CACHES = {}


def _cache(H):
    """(codes..., deq K, deq V) of a 124 935-key layer, quantized by the device kernel (checked against the host)."""
    if H not in _CACHES:
        _CACHES.clear()
        torch.cuda.empty_cache()
        ops = _ops()
        T = 124935
        g = torch.Generator(device=DEV).manual_seed(H)
        # scores of a sane magnitude, row scales spread over several exponents
        k = (torch.randn(H, T, D, device=DEV, generator=g) *
             torch.pow(2.0, torch.randint(-5, 1, (H, T, 1), device=DEV, generator=g).float())).half()
        v = (torch.randn(H, T, D, device=DEV, generator=g) *
             torch.pow(2.0, torch.randint(-12, 5, (H, T, 1), device=DEV, generator=g).float())).half()
        kc, vc, ke, ve = _f8_layer(H, T)
        ops.kv_quant_rows(k, v, kc, vc, ke, ve, 0)
        rc, re_, kd = ops.kv_quantize_ref(k)
        assert torch.equal(_bits(kc), _bits(rc)) and torch.equal(ke, re_)
        del rc, re_, k
        vd = ops.kv_quantize_ref(v)[2]
        del v
        _CACHES[H] = (kc, vc, ke, ve, kd, vd)
    return _CACHES[H]


@pytest.mark.parametrize("H", [32, 40])
def test_fp8_attention_is_bit_identical_to_fp16_on_the_dequantized_cache(H, monkeypatch):
    ops = _ops()
    kc, vc, ke, ve, kd, vd = _cache(H)
    scale = 1.0 / math.sqrt(D)
    g = torch.Generator(device=DEV).manual_seed(7)
    n_cases = 0
    for sq in (1, 7, 16, 17, 18, 32):
        q = torch.randn(sq, H, D, device=DEV, generator=g).half()
        for sk in (1, 15, 4103, 124935):
            if sk < sq:                                   # (a query row with no visible key: not a decode shape)
                continue
            forms = [(None, True, False)]
            if sk >= 4103:
                forms += [(None, False, True), (3, True, True), (13, False, False)]
            for nsplit, fused, packed in forms:
                monkeypatch.setattr(ops, "ATTN_FUSED_MERGE", fused)
                a = ops.attn_decode(q, kd, vd, sk, scale, nsplit=nsplit, packed=packed)
                b = ops.attn_decode_fp8(q, kc, vc, ke, ve, sk, scale, nsplit=nsplit, packed=packed)
                ta, tb = (a.t, b.t) if packed else (a, b)
                assert torch.isfinite(tb.float()).all()
                assert torch.equal(ta, tb), f"sq {sq} sk {sk} H {H} nsplit {nsplit} fused {fused} packed {packed}"
                n_cases += 1
    # sk_dev below the host key count (the captured forward sizes the launch by the capacity)
    for sq in (7, 18):
        q = torch.randn(sq, H, D, device=DEV, generator=g).half()
        sk_dev = torch.tensor([60001], dtype=torch.int32, device=DEV)
        a = ops.attn_decode(q, kd, vd, 124935, scale, sk_dev=sk_dev, packed=True)
        b = ops.attn_decode_fp8(q, kc, vc, ke, ve, 124935, scale, sk_dev=sk_dev, packed=True)
        c = ops.attn_decode(q, kd, vd, 60001, scale, nsplit=ops._pick_nsplit(H, 124935), packed=True)
        assert torch.equal(a.t, b.t) and torch.equal(b.t, c.t)
        n_cases += 1
    Hh.note(f"fp8 attention H={H}: {n_cases} shapes/forms bit-identical to tf_attn_decode_act on deq(K), deq(V)")


def test_fp8_attention_refuses_bad_shapes():
    from triforce_amd import hip
    ops = _ops()
    kc, vc, ke, ve = _f8_layer(2, 64)
    q = torch.zeros(33, 2, D, dtype=torch.float16, device=DEV)
    with pytest.raises(hip.TriforceHipError):
        ops.attn_decode_fp8(q, kc, vc, ke, ve, 64, 0.1)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the FP8 -> fp16 row copy and the retrieval build
# ---------------------------------------------------------------------------------------------------------------------
def test_dequant_rows_pair_and_retrieval_build_match_the_fp16_path(monkeypatch):
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    from oracle import specs
    ops = _ops()
    L, H, T = 3, 32, 1100
    kc = torch.zeros(L, H, T, D, dtype=torch.float8_e4m3fn, device=DEV)
    vc, ke, ve = torch.zeros_like(kc), torch.zeros(L, H, T, dtype=torch.uint8, device=DEV), None
    ve = torch.zeros_like(ke)
    kd, vd = torch.zeros(L, H, T, D, dtype=torch.float16, device=DEV), torch.zeros(L, H, T, D, dtype=torch.float16, device=DEV)
    for l in range(L):
        k, v = _planes(H, T, seed=20 + l)
        ops.kv_quant_rows(k, v, kc[l], vc[l], ke[l], ve[l], 0)
        kd[l], vd[l] = ops.kv_quantize_ref(k)[2], ops.kv_quantize_ref(v)[2]
    a_k, a_v = torch.zeros(L, H, 300, D, dtype=torch.float16, device=DEV), torch.zeros(L, H, 300, D, dtype=torch.float16, device=DEV)
    b_k, b_v = a_k.clone(), a_v.clone()
    ops.kv_dequant_rows_pair(kc, vc, ke, ve, a_k, a_v, 1000, 37, 100)
    ops.kv_copy_rows_pair(kd, vd, b_k, b_v, 1000, 37, 100)
    assert torch.equal(a_k, b_k) and torch.equal(a_v, b_v)

    # retrieval build from an FP8 cache == from an fp16 cache holding the dequantized values
    cfg = specs.llama2_7b_128k_config()
    cfg["num_hidden_layers"] = 2
    model = LlamaForCausalLM.from_state_dict(LlamaConfig.from_dict(cfg), specs.random_state_dict(cfg, 3), DEV)
    f8 = FlashSimpleCache(model, 1024 + 64, kv_dtype="fp8")
    f16 = FlashSimpleCache(model, 1024 + 64, kv_dtype="fp16")
    for l in range(2):
        k, v = _planes(32, 1030, seed=40 + l)
        k = (k.float() * 2.0 ** -12).half()                       # scores of a sane magnitude
        ops.kv_quant_rows(k, v, *f8.layer_codes(l), 0)
        f16.k[l, :, :1030], f16.v[l, :, :1030] = ops.kv_quantize_ref(k)[2], ops.kv_quantize_ref(v)[2]
    f8.seq_len = f16.seq_len = 1030
    for l in range(2):
        dk, dv = f8.dequantize(l)
        assert torch.equal(dk, f16.k[l, :, :1030]) and torch.equal(dv, f16.v[l, :, :1030])
    ga = RetrievalCache(model, max_budget=256, prefill=1024, gamma=6, chunk_size=8)
    gb = RetrievalCache(model, max_budget=256, prefill=1024, gamma=6, chunk_size=8)
    q = torch.randn(1, 32, D, device=DEV).half()
    for l in range(2):
        ga.init_graph_cache(f8, q, l)
        gb.init_graph_cache(f16, q, l)
        assert torch.equal(ga.last_scores[l], gb.last_scores[l]) and torch.equal(ga.last_idx[l], gb.last_idx[l])
    ga.update_graph_cache(f8)
    gb.update_graph_cache(f16)
    assert torch.equal(ga.k, gb.k) and torch.equal(ga.v, gb.v)


# ---------------------------------------------------------------------------------------------------------------------
# 4. a target forward through an FP8 cache
# ---------------------------------------------------------------------------------------------------------------------
def _truth_full_forward(cfg, sd, ids, pos, kd, vd):
    """One-layer full-cache forward accumulated in fp64, rounded at the reference's fp16 points, whose attention reads the
    K / V rows kd / vd (T, H, D) (the dequantized rows the device stored, the fresh ones included)."""
    import torch.nn.functional as F
    from oracle import ref_ops as R
    H, hid, eps = cfg["num_attention_heads"], cfg["hidden_size"], cfg["rms_norm_eps"]
    q_len = ids.shape[1]
    cos, sin = R.rope_tables_for(cfg)
    scale = R.softmax_scale_for(D)

    def lin(x, w):
        return (x.double() @ w.double().t()).half()

    def norm(x, w):
        xf = x.double()
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        return w * xf.half()

    Lp = "model.layers.0."
    x = F.embedding(ids[0], sd["model.embed_tokens.weight"])
    h = norm(x, sd[Lp + "input_layernorm.weight"])
    q = R.apply_rope(lin(h, sd[Lp + "self_attn.q_proj.weight"]).view(q_len, H, D), cos, sin, pos[0])
    sk = kd.shape[0]
    s = torch.einsum("qhd,khd->hqk", q.double(), kd.double()) * float(scale)
    qi, kj = torch.arange(q_len).view(q_len, 1), torch.arange(sk).view(1, sk)
    s = s.masked_fill(kj > (sk - q_len + qi), float("-inf"))
    a = torch.einsum("hqk,khd->qhd", torch.softmax(s, dim=-1), vd.double()).half()
    x = x + lin(a.reshape(q_len, H * D), sd[Lp + "self_attn.o_proj.weight"])
    h = norm(x, sd[Lp + "post_attention_layernorm.weight"])
    gate, up = lin(h, sd[Lp + "mlp.gate_proj.weight"]), lin(h, sd[Lp + "mlp.up_proj.weight"])
    act = (gate.double() * torch.sigmoid(gate.double())).half() * up
    x = x + lin(act, sd[Lp + "mlp.down_proj.weight"])
    return lin(norm(x, sd["model.norm.weight"]), sd["lm_head.weight"]).float()


def test_target_forward_with_an_fp8_cache_matches_fp64_over_the_stored_rows():
    from oracle import specs
    from triforce_amd.models.cache import FlashSimpleCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    cfg = specs.llama2_7b_128k_config()
    cfg["num_hidden_layers"] = 1
    sd = specs.random_state_dict(cfg, 31)
    model = LlamaForCausalLM.from_state_dict(LlamaConfig.from_dict(cfg), sd, DEV)
    cache = FlashSimpleCache(model, 4096 + 64, kv_dtype="fp8")
    gen = torch.Generator().manual_seed(5)
    P, n = 4096, 7
    ids = torch.randint(3, 32000, (1, P + n), generator=gen)
    pre = model(input_ids=ids[:, :P].to(DEV), kv_cache=cache).logits[0, -1].cpu()
    assert cache.seq_len == P
    kd, vd = cache.dequantize(0)
    # the prefill chunk's stored rows are what a truth forward computes, quantized by the contract
    truth_pre = _truth_full_forward(cfg, sd, ids[:, P - 1:P], torch.tensor([[P - 1]]), kd.permute(1, 0, 2).cpu(),
                                    vd.permute(1, 0, 2).cpu())[-1]
    # eager decode rows
    pos = torch.arange(P, P + n).unsqueeze(0)
    eager = model(input_ids=ids[:, P:].to(DEV), kv_cache=cache, position_ids=pos.to(DEV)).logits[0].cpu()
    kd, vd = cache.dequantize(0)
    truth = _truth_full_forward(cfg, sd, ids[:, P:], pos, kd.permute(1, 0, 2).cpu(), vd.permute(1, 0, 2).cpu())
    # captured form (dev_len) over the same cache: rows re-appended at the same slot
    slot = torch.tensor([P], dtype=torch.int32, device=DEV)
    skd = torch.tensor([P + n], dtype=torch.int32, device=DEV)
    tok = ids[:, P:].to(DEV)
    pdev = pos.to(DEV)
    cache.seq_len = P
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model(input_ids=tok, kv_cache=cache, position_ids=pdev, dev_len=(slot, skd))      # warm-up
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model(input_ids=tok, kv_cache=cache, position_ids=pdev, dev_len=(slot, skd)).logits
    graph.replay()
    torch.cuda.synchronize()
    captured = out[0].cpu()
    assert torch.equal(captured, eager), "captured and eager FP8-cache forwards differ"
    # (the prefill chunk's block attention rounds P once to fp16, see pair_softmax_pv / lds_softmax_* in csrc/attn.hip: a wider bar for its row)
    for what, got, want, ulps, mean in (("prefill last row", pre, truth_pre, 4, 2e-3), ("decode rows", eager, truth, 2, 1e-3)):
        d = (got - want).abs()
        mag = float(want.abs().max())
        spacing = 2.0 ** (math.floor(math.log2(max(mag, 1.0))) - 10)
        Hh.note(f"fp8 kv forward, {what}: max |dlogit| vs fp64 {float(d.max()):.3e} (spacing {spacing:.2e}), "
                f"mean {float(d.mean()):.3e}")
        assert float(d.max()) <= ulps * spacing and float(d.mean()) < mean, what


# ---------------------------------------------------------------------------------------------------------------------
# 5. / 6. greedy TriForce is lossless with respect to the FP8-KV target
# ---------------------------------------------------------------------------------------------------------------------
def _ar_gaps(model, prompt, stream, budget, prefill_chunk=None):
    """Teacher-forced argmax gaps of the product's own FP8-KV target: the prompt, then one AR step per emitted token."""
    from triforce_amd.models.cache import FlashSimpleCache
    cache = FlashSimpleCache(model, budget, kv_dtype="fp8")
    P = prompt.shape[1]
    c = prefill_chunk or P
    for r0 in range(0, P, c):
        logits = model(input_ids=prompt[:, r0:r0 + c], kv_cache=cache).logits[0, -1]
    gaps = [float(logits.max() - logits[stream[0]])]
    for i in range(len(stream) - 1):
        logits = model(input_ids=torch.tensor([[stream[i]]], device=DEV), kv_cache=cache).logits[0, -1]
        gaps.append(float(logits.max() - logits[stream[i + 1]]))
    del cache
    return gaps


@pytest.mark.parametrize("graphs", [False, True])
def test_greedy_triforce_with_an_fp8_kv_cache_is_lossless_small(graphs, monkeypatch):
    from triforce_amd.utils.decoding import TriForce
    import copy
    monkeypatch.setenv(ENV, "fp8")
    g = copy.deepcopy(Hh.load_golden("small_gamma6"))
    # the small_gamma6 shapes with head_dim 128 (the FP8 cache's only head size): 256 hidden = 2 heads x 128
    g["tcfg"]["num_attention_heads"] = g["tcfg"]["num_key_value_heads"] = 2
    ge = Hh.build_product(g, DEV, graphs=graphs)
    assert ge.engine.kv_cache.fp8
    prompt = Hh.prompt_of(g).to(DEV)
    res = TriForce(Hh.FakeTokenizer(), ge, prompt, gamma=g["gamma"], max_len=g["gen_len"], top_k=-1, top_p=g["top_p"],
                   temperature=g["temperature"], return_details=True)
    gaps = _ar_gaps(ge.engine.model, prompt, res["tokens"], g["prefill"] + g["gen_len"] + 16)
    assert max(gaps) < GAP_TOL, f"token {gaps.index(max(gaps))} trails the FP8-KV target's argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x == 0.0) >= len(gaps) - 3
    Hh.note(f"fp8 kv small_gamma6 graphs={graphs}: acceptance {res['acceptance_rate']:.3f}, {len(gaps)} tokens")


def test_full_scale_7b_greedy_triforce_with_an_fp8_kv_cache_is_lossless(monkeypatch):
    """configs[1] shape: 7B, 124 928-token prefix through a REAL chunked prefill, budget 4096, gamma 6, hipGraphs, random
    weights.  Every emitted token is the teacher-forced argmax (up to GAP_TOL) of AR steps over the same FP8 cache, and
    the cache with its scratch takes <= 0.56 x the fp16 cache's bytes."""
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
    kv = ge.engine.kv_cache
    assert kv.fp8
    fp16_bytes = 2 * kv.layers * kv.num_heads * kv.max_budget * kv.head_dim * 2
    assert kv.nbytes() <= 0.56 * fp16_bytes, (kv.nbytes(), fp16_bytes)
    tcfg, _ = bench.target_config(args.target)
    ids = torch.randint(3, tcfg.vocab_size, (1, args.prefill), generator=torch.Generator().manual_seed(0)).to(dev)
    run = TriForceRunner(bench._Tok(), ge, args.gamma, top_k=-1, top_p=args.top_p, temperature=args.temp,
                         rng=UniformSource(dev, seed=0))
    bench.do_prefill(run, ge, ids, "real")
    P = kv.seq_len
    assert P == args.prefill
    while run.n < 20:
        run.step()
    stream = list(run.emitted)
    assert len(stream) >= 21 and kv.seq_len == P + run.n
    kv.seq_len = P                                         # AR steps over the same FP8 prefix
    gaps = []
    for i in range(len(stream) - 1):
        tok = torch.tensor([[stream[i]]], device=dev)
        logits = ge.engine.model(input_ids=tok, kv_cache=kv, graph_cache=None).logits[0, -1]
        gaps.append(float(logits.max() - logits[stream[i + 1]]))
    assert max(gaps) < GAP_TOL, f"token {gaps.index(max(gaps)) + 1} trails the FP8-KV AR argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x == 0.0) >= len(gaps) - 2
    Hh.note(f"fp8 kv full 7B: cache {kv.nbytes() / 2**30:.2f} GiB vs fp16 {fp16_bytes / 2**30:.2f} GiB, "
            f"{len(gaps)} tokens lossless")
    del ge, run, kv, target, draft
    torch.cuda.empty_cache()
