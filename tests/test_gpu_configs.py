"""Device-vs-oracle parity at the widths of the BASELINE configs the small golden fixtures cannot reach:

  configs[2]  LWM-Text-Chat-128K: 7B widths with PLAIN RoPE, theta = 1e7, positions >= 100 000
              (reference models/modeling_llama.py:181-186 — the non-YaRN branch of _init_rope)
  configs[4]  Llama-2-13B-128K at TP = 8: ONE RANK's shard — hidden 5120, 5 local heads x 128, 1728 MLP columns,
              gamma 16 (17 / 18 rows: two MFMA row tiles), retrieval cache of 12 305 slots — through the tensor-parallel
              engine's layer (un-fused at 17 rows, fused at 7), sliced as models/TP_layers.py:126-147 slices it
  attention   the split-KV kernel with its DEFAULT split rule at H = 5 (nsplit ~ 51: the two-launch merge) and H = 40
  fp64 truth  device, CPU oracle and an fp64-accumulating restatement of one 7B-width layer: the device must be no
              further from the exactly-accumulated result than the CPU oracle is — the evidence behind the logit bar
              of tests/test_gpu_e2e.py (_logit_check), with every measured deviation written to gpurun_out/parity_notes.txt

All through the C ABI (ops -> libtriforce_hip.so); the oracle is the checker only.
"""
import math
import os
import socket

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_model as M
from oracle import ref_ops as R
from oracle import specs
from tests import helpers as Hh
from tests.test_gpu_e2e import GAP_TOL, _logit_check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _fill_retrieval(ogc, seed):
    gen = torch.Generator().manual_seed(seed)
    ogc.key_cache.copy_(torch.randn(ogc.key_cache.shape, generator=gen).half())
    ogc.value_cache.copy_(torch.randn(ogc.value_cache.shape, generator=gen).half())
    return gen


def _deviation(what, got, want):
    d = (got - want).abs()
    Hh.note(f"{what}: max |dlogit| {float(d.max()):.3e}, mean {float(d.mean()):.3e}, max |logit| {float(want.abs().max()):.2f}")
    return d


# ---------------------------------------------------------------------------------------------------------------
# configs[2]: LWM — plain RoPE, theta 1e7
# ---------------------------------------------------------------------------------------------------------------
def test_lwm_plain_rope_theta1e7_layer_logits_match_oracle():
    """One decoder layer at the LWM-Text-Chat-128K widths (7B: hidden 4096, 32 x 128 heads, intermediate 11008, vocabulary
    32000) with its PLAIN rotary tables (theta 1e7, no scaling) at positions >= 100 000, over a 4 103-slot retrieval
    cache AND over a full cache: fused q|k|v + RoPE + append epilogue, split-KV attention, fp32-out lm_head."""
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    cfg = specs.lwm_text_chat_128k_config()
    assert cfg["rope_scaling"] is None and cfg["rope_theta"] == 1e7
    cfg["num_hidden_layers"] = 1
    sd = specs.random_state_dict(cfg, 47)
    gamma, budget, prefill = 6, 4096, 8192
    ot = M.OracleTarget(cfg, sd)
    ogc = M.RetrievalCacheO(cfg, budget, prefill, 8, gamma)
    gen = _fill_retrieval(ogc, 6)
    model = LlamaForCausalLM.from_state_dict(LlamaConfig.from_dict(cfg), sd, DEV)
    # the rotary tables themselves: plain RoPE at theta 1e7 (the product builds them on the host like the reference)
    cos, sin = R.rope_tables_plain(128, cfg["max_position_embeddings"], 1e7)
    assert torch.equal(model.cos.cpu(), cos) and torch.equal(model.sin.cpu(), sin)
    pg = RetrievalCache(model, max_budget=budget, prefill=prefill, gamma=gamma, chunk_size=8)
    pg.k.copy_(ogc.key_cache.permute(0, 2, 1, 3))
    pg.v.copy_(ogc.value_cache.permute(0, 2, 1, 3))
    ids = torch.randint(3, 32000, (1, gamma + 1), generator=gen)
    pos = torch.arange(120000, 120000 + gamma + 1).unsqueeze(0)
    okv, pkv = M.FullCache(cfg, 64), FlashSimpleCache(model, 64)
    want = ot.forward(ids, okv, ogc, position_ids=pos, spec=True)
    got = model(input_ids=ids.to(DEV), kv_cache=pkv, graph_cache=pg, position_ids=pos.to(DEV), spec=True).logits.cpu()
    _deviation("LWM (plain RoPE theta 1e7) 7B-width layer, retrieval-cache forward at position 120 000", got, want)
    _logit_check("LWM-width layer, retrieval-cache forward", got, want)
    s = pg.spec_slot                                       # rows appended by the fused RoPE epilogue: rotated K, bit for bit
    dk = (pg.k[0, :, s:].permute(1, 0, 2).cpu().float() - ogc.key_cache[0, s:].float()).abs()
    assert Hh.bound("appended K rows, max", dk.max(), 8e-3) and Hh.bound("appended K rows, mean", dk.mean(), 2e-6)
    trail = want.max(-1).values - want.gather(-1, got.argmax(-1, keepdim=True))[..., 0]
    assert float(trail.max()) < GAP_TOL
    # full-cache branch (target verify): 8 rows appended behind 2 000 cached keys whose positions end at 110 000
    S = 2000
    okv, pkv = M.FullCache(cfg, S + 16), FlashSimpleCache(model, S + 16)
    okv.key_cache[0, :S] = torch.randn(S, 32, 128, generator=gen).half()
    okv.value_cache[0, :S] = torch.randn(S, 32, 128, generator=gen).half()
    okv.seq_len = S
    pkv.k[0, :, :S] = okv.key_cache[0, :S].permute(1, 0, 2).to(DEV)
    pkv.v[0, :, :S] = okv.value_cache[0, :S].permute(1, 0, 2).to(DEV)
    pkv.seq_len = S
    ids8 = torch.randint(3, 32000, (1, gamma + 2), generator=gen)
    pos8 = torch.arange(110000, 110000 + gamma + 2).unsqueeze(0)
    want = ot.forward(ids8, okv, None, position_ids=pos8)
    got = model(input_ids=ids8.to(DEV), kv_cache=pkv, graph_cache=None, position_ids=pos8.to(DEV)).logits.cpu()
    _deviation("LWM 7B-width layer, full-cache forward at position 110 000", got, want)
    _logit_check("LWM-width layer, full-cache forward", got, want)


# ---------------------------------------------------------------------------------------------------------------
# configs[1] at FULL cache size: one layer's target verify, model forward vs oracle
# ---------------------------------------------------------------------------------------------------------------
def test_full_size_cfg2_single_layer_target_verify_matches_oracle():
    """BASELINE configs[1] shapes for ONE layer through the MODEL forward (not op by op): 8 verify rows appended behind
    124 928 cached keys (32 heads x 128, YaRN positions 124 928...), fused q|k|v + RoPE + append, split-KV attention over
    124 936 keys, o_proj, MLP, lm_head — against the oracle's forward over the same cache.  (The 32-layer engine at this
    size is checked on the device for losslessness in tests/test_gpu_e2e.py; the oracle cannot run 32 layers x 125K keys
    on a CPU in test time, one layer it can.)"""
    from triforce_amd.models.cache import FlashSimpleCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    cfg = specs.llama2_7b_128k_config()
    cfg["num_hidden_layers"] = 1
    sd = specs.random_state_dict(cfg, 61)
    S, rows = 124928, 8
    ot = M.OracleTarget(cfg, sd)
    model = LlamaForCausalLM.from_state_dict(LlamaConfig.from_dict(cfg), sd, DEV)
    okv, pkv = M.FullCache(cfg, S + 16), FlashSimpleCache(model, S + 16)
    g = torch.Generator(device=DEV).manual_seed(9)
    pkv.k[0, :, :S].normal_(generator=g)                      # (H, S, D) on the device; the oracle gets the same bits
    pkv.v[0, :, :S].normal_(generator=g)
    okv.key_cache[0, :S] = pkv.k[0, :, :S].permute(1, 0, 2).cpu()
    okv.value_cache[0, :S] = pkv.v[0, :, :S].permute(1, 0, 2).cpu()
    okv.seq_len = pkv.seq_len = S
    ids = torch.randint(3, 32000, (1, rows), generator=torch.Generator().manual_seed(10))
    want = ot.forward(ids, okv, None)
    got = model(input_ids=ids.to(DEV), kv_cache=pkv, graph_cache=None).logits.cpu()
    _deviation(f"configs[1] full-size single layer: {rows} rows over {S + rows} keys x 32 heads", got, want)
    _logit_check("full-size cfg2 layer, target verify", got, want)
    dk = (pkv.k[0, :, S:S + rows].permute(1, 0, 2).cpu().float() - okv.key_cache[0, S:S + rows].float()).abs()
    assert Hh.bound("appended K rows at positions >= 124 928, max", dk.max(), 8e-3) and Hh.bound("appended K rows at positions >= 124 928, mean", dk.mean(), 2e-6), "appended K rows (RoPE at positions >= 124 928) differ"
    trail = want.max(-1).values - want.gather(-1, got.argmax(-1, keepdim=True))[..., 0]
    assert float(trail.max()) < GAP_TOL


# ---------------------------------------------------------------------------------------------------------------
# configs[4]: 13B, one rank of TP = 8
# ---------------------------------------------------------------------------------------------------------------
def _one_process_group():
    import torch.distributed as dist
    if not dist.is_initialized():
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", rank=0, world_size=1, init_method=f"tcp://127.0.0.1:{port}")


def _shard_engine(cfg, sd, rank, world, gamma, budget, prefill, gen_len=64):
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.TP_llama import DistributedLlama
    llm = DistributedLlama("unused", config=LlamaConfig.from_dict(cfg), device=DEV, local_rank=rank, world_size=world,
                           prefill=prefill, gen_len=gen_len, retrieval_budget=budget, retrieval_chunk_size=8,
                           kv_offload=True, on_chip_layers=cfg["num_hidden_layers"], gamma=gamma)
    llm.init_parameters(sd)
    return llm


@pytest.mark.parametrize("gamma,fused", [(16, False), (16, True), (6, True), (6, False)])
def test_13b_tp8_shard_layer_logits_match_oracle(gamma, fused, monkeypatch):
    """Rank 3 of an 8-way Llama-2-13B-128K layer (5 heads x 128, 1728 MLP columns, hidden 5120; retrieval cache of
    budget 12 288 + gamma + 1 slots) through the tensor-parallel engine with a one-process group — every all-reduce is
    the identity, so the rank computes the narrower network oracle.specs.shard_of() slices out of the same full state
    dict by the reference's rule (TP_layers.py:126-147).  gamma 16: 17-row retrieval verify and 18-row target verify
    (two MFMA row tiles; the un-fused layer, and — round 4 — the fused 8-launch layer with k-octet-major activations);
    gamma 6: the fused layer (with the real exchange kernel in a one-rank group playing the all-reduce) and the un-fused
    one.  NB the target verify here runs behind a 9 000-key full cache (prefill 16 384), not 130 048: the 130K-key H = 5
    attention is covered at the op level (test_attn_decode_default_split_rule_at_13b_head_counts)."""
    from triforce_amd.utils.oneshot_ar import OneShotAllReduce
    monkeypatch.setenv("TRIFORCE_ALLREDUCE", "rccl")       # no peers to map in a one-process group
    monkeypatch.setenv("TRIFORCE_TP_FUSE", "1" if fused else "0")
    _one_process_group()
    rank, world, budget, prefill = 3, 8, 12288, 16384
    cfg = specs.llama2_13b_128k_config()
    cfg["num_hidden_layers"] = 1
    sd = specs.random_state_dict(cfg, 53)
    scfg, ssd = specs.shard_of(cfg, sd, rank, world)
    assert (scfg["num_attention_heads"], scfg["intermediate_size"], scfg["head_dim"]) == (5, 1728, 128)
    llm = _shard_engine(cfg, sd, rank, world, gamma, budget, prefill)
    assert (llm.weights.H_local, llm.weights.I_local) == (5, 1728)
    if fused:
        llm._ar = OneShotAllReduce.local_group(1, DEV, llm.ONESHOT_MAX_ROWS * llm.hidden_size)[0]
    assert llm._fused_decode(gamma + 1) == fused
    ot = M.OracleTarget(scfg, ssd)
    ogc = M.RetrievalCacheO(scfg, budget, prefill, 8, gamma)
    assert ogc.real_budget == budget + gamma + 1
    gen = _fill_retrieval(ogc, 8)
    rc = llm.retrieval_cache
    rc.k.copy_(ogc.key_cache.permute(0, 2, 1, 3))
    rc.v.copy_(ogc.value_cache.permute(0, 2, 1, 3))
    ids = torch.randint(3, 32000, (1, gamma + 1), generator=gen)
    pos = torch.arange(130048, 130048 + gamma + 1).unsqueeze(0)
    want = ot.forward(ids, M.FullCache(scfg, 8), ogc, position_ids=pos, spec=True)
    got = llm.retrieval_inference(ids.to(DEV), pos.to(DEV)).cpu()
    tag = f"13B TP8 shard (rank {rank}: 5 heads, I 1728), gamma {gamma}, {'fused' if fused else 'un-fused'} layer"
    _deviation(f"{tag}, retrieval verify over {ogc.real_budget} slots", got, want)
    _logit_check(f"{tag}, retrieval verify", got, want)
    trail = want.max(-1).values - want.gather(-1, got.argmax(-1, keepdim=True))[..., 0]
    assert float(trail.max()) < GAP_TOL
    # target verify: gamma + 2 rows behind S cached keys (positions continue at S, like the engine's own forward)
    S = 9000
    okv = M.FullCache(scfg, S + 32)
    okv.key_cache[0, :S] = torch.randn(S, 5, 128, generator=gen).half()
    okv.value_cache[0, :S] = torch.randn(S, 5, 128, generator=gen).half()
    okv.seq_len = S
    kvc = llm.kv_cache
    kvc.k[0, :, :S] = okv.key_cache[0, :S].permute(1, 0, 2).to(DEV)
    kvc.v[0, :, :S] = okv.value_cache[0, :S].permute(1, 0, 2).to(DEV)
    kvc.seq_len = S
    ids_t = torch.randint(3, 32000, (1, gamma + 2), generator=gen)
    want = ot.forward(ids_t, okv, None)
    got = llm.inference(ids_t.to(DEV)).cpu()
    _deviation(f"{tag}, target verify ({gamma + 2} rows over {S} keys)", got, want)
    _logit_check(f"{tag}, target verify", got, want)
    assert llm.kv_cache.seq_len == S + gamma + 2
    if fused:
        assert llm._ar.error() == 0


# ---------------------------------------------------------------------------------------------------------------
# attention at the head counts of the 13B engine, default split rule
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sq,sk,H", [(17, 12305, 5), (18, 130066, 5), (1, 130049, 5), (7, 4103, 40), (8, 32775, 40),
                                     (18, 20018, 40)])
def test_attn_decode_default_split_rule_at_13b_head_counts(sq, sk, H):
    """tf_attn_decode[_fused] with the DEFAULT nsplit at H = 5 (one rank of the 13B at TP = 8: ~51 splits per head ->
    more than FUSED_MERGE_MAX_SPLITS, the two-launch merge) and H = 40 (the un-sharded 13B), one and two q-tiles."""
    from triforce_amd import hip, ops
    D = 128
    scale = R.softmax_scale_for(D)
    g = torch.Generator().manual_seed(100 + sq + H)
    q = torch.randn(sq, H, D, generator=g).half()
    k = torch.randn(sk, H, D, generator=g).half()
    v = torch.randn(sk, H, D, generator=g).half()
    nsplit = hip.lib().tf_attn_decode_pick_nsplit(H, sk)
    if H == 5 and sk > 100000:
        assert nsplit > 8, "expected the many-split (two-launch merge) regime at 5 heads"
    want = R.attn_kvcache(q, k, v, scale).reshape(sq, H * D)
    got = ops.attn_decode(q.to(DEV), k.permute(1, 0, 2).contiguous().to(DEV), v.permute(1, 0, 2).contiguous().to(DEV), sk,
                          scale)
    d = (got.float().cpu() - want.float()).abs()
    Hh.note(f"attention {sq} rows x {sk} keys x {H} heads, default nsplit {nsplit}: max |d| {float(d.max()):.2e}, "
            f"mean {float(d.mean()):.2e}")
    Hh.close(got.float().cpu(), want.float(), atol=2e-5, rtol=1.5e-3)      # tests/test_gpu_ops.py DECODE_*


# ---------------------------------------------------------------------------------------------------------------
# fp64 truth: is the device further from the exactly-accumulated result than the CPU oracle is?
# ---------------------------------------------------------------------------------------------------------------
def _truth_retrieval_forward(cfg, sd, ids, pos, gk, gv, spec_slot):
    """The oracle's retrieval-cache forward (oracle.ref_model.OracleTarget.forward, spec branch) with every reduction
    accumulated in fp64 and rounded ONCE at the reference's rounding points (each op's fp16 output): the result the
    reference's arithmetic defines up to accumulation order.  One layer; gk / gv (R, H, D) fp16, rows >= spec_slot are
    overwritten with this block's K / V like RetrievalCache.update (cache.py:184-189)."""
    H, hid, eps = cfg["num_attention_heads"], cfg["hidden_size"], cfg["rms_norm_eps"]
    D = cfg.get("head_dim", hid // H)                      # a TP shard keeps hidden but has fewer heads (specs.shard_of)
    q_len = ids.shape[1]
    cos, sin = R.rope_tables_for(cfg)
    scale = R.softmax_scale_for(D)

    def lin(x, w):
        return (x.double() @ w.double().t()).half()

    def norm(x, w):                                        # fp32 normalise -> fp16 -> x weight, modeling_llama.py:138-143
        xf = x.double()
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        return w * xf.half()

    L = "model.layers.0."
    x = F.embedding(ids[0], sd["model.embed_tokens.weight"])
    h = norm(x, sd[L + "input_layernorm.weight"])
    q = lin(h, sd[L + "self_attn.q_proj.weight"]).view(q_len, H, D)
    k = lin(h, sd[L + "self_attn.k_proj.weight"]).view(q_len, H, D)
    v = lin(h, sd[L + "self_attn.v_proj.weight"]).view(q_len, H, D)
    q, k = R.apply_rope(q, cos, sin, pos[0]), R.apply_rope(k, cos, sin, pos[0])       # fp16 element-wise: exact roundings
    gk, gv = gk.clone(), gv.clone()
    gk[spec_slot:spec_slot + q_len], gv[spec_slot:spec_slot + q_len] = k, v
    sk = gk.shape[0]
    s = torch.einsum("qhd,khd->hqk", q.double(), gk.double()) * float(scale)
    qi, kj = torch.arange(q_len).view(q_len, 1), torch.arange(sk).view(1, sk)
    s = s.masked_fill(kj > (sk - q_len + qi), float("-inf"))
    a = torch.einsum("hqk,khd->qhd", torch.softmax(s, dim=-1), gv.double()).half()
    x = x + lin(a.reshape(q_len, H * D), sd[L + "self_attn.o_proj.weight"])
    h = norm(x, sd[L + "post_attention_layernorm.weight"])
    gate, up = lin(h, sd[L + "mlp.gate_proj.weight"]), lin(h, sd[L + "mlp.up_proj.weight"])
    act = (gate.double() * torch.sigmoid(gate.double())).half() * up                  # silu rounded to fp16, then x up
    x = x + lin(act, sd[L + "mlp.down_proj.weight"])
    return lin(norm(x, sd["model.norm.weight"]), sd["lm_head.weight"]).float().unsqueeze(0)


def test_device_is_as_close_to_fp64_truth_as_the_cpu_oracle():
    """north_star asks for logits "within 1e-3 fp16" of the reference's CPU path; tests/test_gpu_e2e.py allows 2 fp16
    spacings at the largest logit, arguing that the CPU path's own fp32 accumulation order is that far from exact.
    Here that argument is measured at 7B widths: device, CPU oracle and an fp64-accumulating restatement (same fp16
    rounding points) of one layer over a 4 103-slot retrieval cache.  The device must be no further from the fp64 result
    than the CPU oracle is (max within one fp16 spacing more, mean within 15 %).
    Measured (profiles/r03*_parity_notes.txt): with P rounded once to fp16 before the PV MFMA (round 2) the device's mean
    distance to the fp64 result was 7.9e-4 against the oracle's 5.7e-4 — 37 % of the attention outputs were one ulp
    off; with P fed as hi + lo (csrc/attn.hip, attn_tile) it is 5.5e-4 / max one fp16 spacing: level with the oracle.
    Both differ from the exactly accumulated logits at ~2/3 of the positions — a one-ulp flip in a hidden state moves
    every logit of the row by a fraction of a spacing — which is what the resolution-aware bar of _logit_check rests on."""
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    cfg = specs.llama2_7b_128k_config()
    cfg["num_hidden_layers"] = 1
    sd = specs.random_state_dict(cfg, 31)
    gamma, budget, prefill = 6, 4096, 8192
    ot = M.OracleTarget(cfg, sd)
    ogc = M.RetrievalCacheO(cfg, budget, prefill, 8, gamma)
    gen = _fill_retrieval(ogc, 5)
    gk0, gv0 = ogc.key_cache[0].clone(), ogc.value_cache[0].clone()
    model = LlamaForCausalLM.from_state_dict(LlamaConfig.from_dict(cfg), sd, DEV)
    pg = RetrievalCache(model, max_budget=budget, prefill=prefill, gamma=gamma, chunk_size=8)
    pg.k.copy_(ogc.key_cache.permute(0, 2, 1, 3))
    pg.v.copy_(ogc.value_cache.permute(0, 2, 1, 3))
    ids = torch.randint(3, 32000, (1, gamma + 1), generator=gen)
    pos = torch.arange(100000, 100000 + gamma + 1).unsqueeze(0)
    oracle = ot.forward(ids, M.FullCache(cfg, 64), ogc, position_ids=pos, spec=True)
    device = model(input_ids=ids.to(DEV), kv_cache=FlashSimpleCache(model, 64), graph_cache=pg, position_ids=pos.to(DEV),
                   spec=True).logits.cpu()
    truth = _truth_retrieval_forward(cfg, sd, ids, pos, gk0, gv0, ogc.real_budget - gamma - 1)
    d_dev, d_orc, d_do = (device - truth).abs(), (oracle - truth).abs(), (device - oracle).abs()
    mag = float(truth.abs().max())
    spacing = 2.0 ** (math.floor(math.log2(max(mag, 1.0))) - 10)
    Hh.note(f"fp64 truth, 7B-width layer ({truth.numel()} logits, max |logit| {mag:.2f}, fp16 spacing {spacing:.2e}): "
            f"device-truth max {float(d_dev.max()):.3e} mean {float(d_dev.mean()):.3e} | "
            f"oracle-truth max {float(d_orc.max()):.3e} mean {float(d_orc.mean()):.3e} | "
            f"device-oracle max {float(d_do.max()):.3e} mean {float(d_do.mean()):.3e} | "
            f"logits differing from truth: device {float((d_dev > 0).float().mean()):.3f}, "
            f"oracle {float((d_orc > 0).float().mean()):.3f}")
    assert float(d_dev.max()) <= float(d_orc.max()) + spacing, "device is further from the fp64 result than the CPU oracle"
    assert float(d_dev.mean()) <= 1.15 * float(d_orc.mean()) + 1e-6
    assert float(d_dev.max()) <= 2 * spacing and float(d_dev.mean()) < 1e-3


@pytest.mark.parametrize("gamma", [16, 6])
def test_fused_tp_layer_is_as_close_to_fp64_truth_as_the_cpu_oracle(gamma, monkeypatch):
    """The fp64-truth comparison of the test above for the two cases the round-3 verdict found un-covered: the FUSED
    tensor-parallel layer (rank 3 of the 13B at TP = 8 with the real exchange kernel in the chain — the case that sat at
    1.9 of the 2 allowed fp16 spacings against the oracle) at 7 rows, and at 17 rows: two MFMA row tiles, the two-q-tile
    attention kernel, k-octet-major activations, K split across workgroups in the q|k|v / gate|up GEMMs.  Device, CPU oracle
    and the fp64-accumulating restatement of the same shard; the device must be no further from the fp64 result than
    the oracle is (max within one fp16 spacing more, mean within 15 %)."""
    from triforce_amd.utils.oneshot_ar import OneShotAllReduce
    monkeypatch.setenv("TRIFORCE_ALLREDUCE", "rccl")
    monkeypatch.setenv("TRIFORCE_TP_FUSE", "1")
    _one_process_group()
    rank, world, budget, prefill = 3, 8, 12288, 16384
    cfg = specs.llama2_13b_128k_config()
    cfg["num_hidden_layers"] = 1
    sd = specs.random_state_dict(cfg, 53)
    scfg, ssd = specs.shard_of(cfg, sd, rank, world)
    llm = _shard_engine(cfg, sd, rank, world, gamma, budget, prefill)
    llm._ar = OneShotAllReduce.local_group(1, DEV, llm.ONESHOT_MAX_ROWS * llm.hidden_size)[0]
    assert llm._fused_decode(gamma + 1)
    ot = M.OracleTarget(scfg, ssd)
    ogc = M.RetrievalCacheO(scfg, budget, prefill, 8, gamma)
    gen = _fill_retrieval(ogc, 8)
    gk0, gv0 = ogc.key_cache[0].clone(), ogc.value_cache[0].clone()
    rc = llm.retrieval_cache
    rc.k.copy_(ogc.key_cache.permute(0, 2, 1, 3))
    rc.v.copy_(ogc.value_cache.permute(0, 2, 1, 3))
    ids = torch.randint(3, 32000, (1, gamma + 1), generator=gen)
    pos = torch.arange(130048, 130048 + gamma + 1).unsqueeze(0)
    oracle = ot.forward(ids, M.FullCache(scfg, 8), ogc, position_ids=pos, spec=True)
    device = llm.retrieval_inference(ids.to(DEV), pos.to(DEV)).cpu()
    truth = _truth_retrieval_forward(scfg, ssd, ids, pos, gk0, gv0, ogc.real_budget - gamma - 1)
    d_dev, d_orc, d_do = (device - truth).abs(), (oracle - truth).abs(), (device - oracle).abs()
    mag = float(truth.abs().max())
    spacing = 2.0 ** (math.floor(math.log2(max(mag, 1.0))) - 10)
    Hh.note(f"fp64 truth, fused 13B TP8-shard layer, {gamma + 1} rows ({truth.numel()} logits, max |logit| {mag:.2f}, fp16 "
            f"spacing {spacing:.2e}): device-truth max {float(d_dev.max()):.3e} mean {float(d_dev.mean()):.3e} | "
            f"oracle-truth max {float(d_orc.max()):.3e} mean {float(d_orc.mean()):.3e} | "
            f"device-oracle max {float(d_do.max()):.3e} mean {float(d_do.mean()):.3e}")
    # which logit carries the device's largest deviation, and what it is made of (the round-4 verdict asked for it: at 7 rows the
    # device's max sat further from the truth than the oracle's, inside the one-spacing slack): a logit of magnitude >= 4 rounds to
    # a grid of `spacing`; the fp32 value in front of that rounding is reported via the two neighbours the truth lies between
    w = int(d_dev.reshape(-1).argmax())
    row, tok = divmod(w, truth.shape[-1])
    tv, dv, ov = float(truth.reshape(-1)[w]), float(device.reshape(-1)[w]), float(oracle.reshape(-1)[w])
    Hh.note(f"fp64 truth, fused 13B TP8-shard layer, {gamma + 1} rows: the device's worst logit is row {row} token {tok}: truth {tv:.5f}, "
            f"device {dv:.5f} ({abs(dv - tv) / spacing:.2f} spacings at max |logit|; {abs(dv - tv) / (2.0 ** (math.floor(math.log2(max(abs(tv), 1e-3))) - 10)):.2f} "
            f"spacings of its OWN binade), oracle {ov:.5f}; logits this far out: device {int((d_dev > 0.75 * float(d_dev.max())).sum())}, "
            f"oracle {int((d_orc > 0.75 * float(d_dev.max())).sum())} of {truth.numel()} — the max of {truth.numel()} rounding errors of a 5120-term fp16-input "
            "sum whose hidden state already carries one fp16 rounding per layer op; the MEAN is the statistic that separates the two paths")
    assert llm._ar.error() == 0
    assert float(d_dev.max()) <= float(d_orc.max()) + spacing, "device is further from the fp64 result than the CPU oracle"
    assert float(d_dev.mean()) <= 1.15 * float(d_orc.mean()) + 1e-6
    assert float(d_dev.max()) <= 2 * spacing and float(d_dev.mean()) < 1e-3
