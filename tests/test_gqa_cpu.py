"""Grouped-query attention targets on CPU: config rules, weight shapes, the rotary row order with two
head counts, the group-mean retrieval query, every refusal, and the host logic end to end — the product with every HIP op
swapped for an oracle restatement (cpu_ops + the GQA stand-ins below) against the UNMODIFIED oracle run on the expanded
multi-head state dict (k_proj / v_proj head blocks repeated g times), which is what a GQA model is defined to be."""
import pytest
import torch

from oracle import ref_model as M
from oracle import ref_ops as R
from oracle import specs
from tests import cpu_backend
from tests import helpers as Hh


# ---- GQA stand-ins: expand K / V over the head axis, then the oracle op ------------------------------------------------
def _expand(layer, H):
    g = H // layer.shape[0]
    return layer if g == 1 else layer.repeat_interleave(g, dim=0)


def gqa_attn_decode(q, k_layer, v_layer, sk, scale, sk_dev=None, nsplit=None, packed=False):
    H = q.shape[1]
    return cpu_backend.attn_decode(q, _expand(k_layer, H), _expand(v_layer, H), sk, scale, packed=packed)


def gqa_attn_prefill(q, k_layer, v_layer, sk, scale):
    return gqa_attn_decode(q, k_layer, v_layer, sk, scale)


def gqa_rope_append(qkv, cos, sin, positions, k_layer, v_layer, slot0, H, D, rotate_k=True, slot0_dev=None, Hkv=None):
    Hkv = H if Hkv is None else Hkv
    rows = qkv.shape[0]
    q = qkv[:, :H * D].reshape(rows, H, D)
    k = qkv[:, H * D:(H + Hkv) * D].reshape(rows, Hkv, D)
    v = qkv[:, (H + Hkv) * D:].reshape(rows, Hkv, D)
    qr = R.apply_rope(q, cos, sin, positions)
    kr = R.apply_rope(k, cos, sin, positions) if rotate_k else k
    k_layer[:, slot0:slot0 + rows] = kr.permute(1, 0, 2)
    v_layer[:, slot0:slot0 + rows] = v.permute(1, 0, 2)
    return qr.contiguous()


@pytest.fixture
def gqa_ops(cpu_ops, monkeypatch):
    monkeypatch.setattr(cpu_ops, "attn_decode", gqa_attn_decode)
    monkeypatch.setattr(cpu_ops, "attn_prefill", gqa_attn_prefill)
    monkeypatch.setattr(cpu_ops, "rope_append", gqa_rope_append)
    return cpu_ops


# ---- a tiny-gqa-sized case (zoo "tiny-gqa": hidden 512, 4 / 2 heads, D = 128) with small_gamma6's draft ------------------
def _case():
    g = dict(Hh.load_golden("small_gamma6"))
    tcfg = specs.llama_config(512, 768, 2, 4, vocab_size=g["dcfg"]["vocab_size"], max_position_embeddings=4096,
                              rope_scaling=dict(type="yarn", factor=16.0, original_max_position_embeddings=256),
                              name="tiny-yarn-gqa-target")
    g.update(tcfg=tcfg, tseed=711, prefill=512, gen_len=24, budget=128)
    return g


def gqa_state_dicts(tcfg_mha, seed, Hkv, head_std=0.05):
    """(GQA config, GQA state dict, expanded MHA state dict): the seeded MHA draw with k_proj / v_proj cut to the first Hkv
    heads, and the same weights with each of those head blocks repeated g times."""
    H, hid = tcfg_mha["num_attention_heads"], tcfg_mha["hidden_size"]
    D, g = hid // H, H // Hkv
    sd = specs.random_state_dict(tcfg_mha, seed, head_std=head_std)
    gsd, esd = dict(sd), dict(sd)
    for name, w in sd.items():
        if "k_proj" in name or "v_proj" in name:
            small = w[:Hkv * D].contiguous()
            gsd[name] = small
            esd[name] = small.view(Hkv, D, hid).repeat_interleave(g, dim=0).reshape(H * D, hid).contiguous()
    return dict(tcfg_mha, num_key_value_heads=Hkv), gsd, esd


def _product(g, gcfg, gsd, dsd):
    return Hh.build_product(dict(g, tcfg=gcfg), "cpu", gsd, dsd)


def _oracle_ar(g, esd, prompt, n):
    eng = M.OracleEngine(M.OracleTarget(g["tcfg"], esd), M.FullCache(g["tcfg"], prompt.shape[1] + n + 16), None, None, None,
                         g["temperature"], g["top_p"])
    return M.autoregressive(eng, prompt, n, g["temperature"], g["top_p"])


# ---- config --------------------------------------------------------------------------------------------------------------
def test_config_rules():
    from triforce_amd.models.config_yarn import LlamaConfig
    c = LlamaConfig(hidden_size=1024, num_attention_heads=8, num_key_value_heads=2)
    assert (c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.kv_groups) == (8, 2, 128, 4)
    with pytest.raises(ValueError, match="GQA"):
        LlamaConfig(hidden_size=1024, num_attention_heads=8, num_key_value_heads=3)
    with pytest.raises(ValueError, match="GQA"):
        LlamaConfig(hidden_size=4096, num_attention_heads=8, num_key_value_heads=2)        # head_dim 512
    m = LlamaConfig(hidden_size=4096, num_attention_heads=8)                               # MHA: any head_dim, as before
    assert m.num_key_value_heads == 8 and m.head_dim == 512 and m.kv_groups == 1
    assert LlamaConfig(hidden_size=512, num_attention_heads=8, num_key_value_heads=1).head_dim == 64


def test_zoo_entries():
    from triforce_amd.models import zoo
    t = zoo.config("tiny-gqa")
    assert (t.hidden_size, t.num_attention_heads, t.num_key_value_heads, t.head_dim) == (512, 4, 2, 128)
    tiny = zoo.config("tiny")
    assert (t.num_hidden_layers, t.intermediate_size, t.rope_scaling) == (tiny.num_hidden_layers, tiny.intermediate_size,
                                                                          tiny.rope_scaling)
    b = zoo.config("llama-70B-32K")
    assert (b.hidden_size, b.intermediate_size, b.num_hidden_layers, b.num_attention_heads, b.num_key_value_heads,
            b.head_dim, b.max_position_embeddings, b.rope_scaling["factor"]) == (8192, 28672, 80, 64, 8, 128, 32768, 8.0)


# ---- weights ---------------------------------------------------------------------------------------------------------------
def test_load_state_dict_fuses_gqa_rows_in_qkv_order():
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.llama_core import LlamaWeights
    g = _case()
    gcfg, gsd, _ = gqa_state_dicts(g["tcfg"], g["tseed"], 2)
    W = LlamaWeights(LlamaConfig.from_dict(gcfg), "cpu").load_state_dict(gsd)
    assert (W.H, W.Hkv, W.H_local, W.Hkv_local, W.D) == (4, 2, 4, 2, 128)
    for i in range(W.L):
        w = W.wqkv[i].w
        assert tuple(w.shape) == ((4 + 2 * 2) * 128, 512) and W.wqkv[i].rope == (4, 2, 128) and W.wqkv[i].gqa
        p = f"model.layers.{i}.self_attn."
        assert torch.equal(w[:512], gsd[p + "q_proj.weight"])
        assert torch.equal(w[512:768], gsd[p + "k_proj.weight"])
        assert torch.equal(w[768:], gsd[p + "v_proj.weight"])
    with pytest.raises(ValueError, match="GQA"):
        LlamaWeights(LlamaConfig.from_dict(gcfg), "cpu", rank=0, world_size=2)


def test_init_random_shapes_and_mha_draw_unchanged():
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.llama_core import LlamaWeights
    g = _case()
    gcfg = dict(g["tcfg"], num_key_value_heads=2)
    W = LlamaWeights(LlamaConfig.from_dict(gcfg), "cpu").init_random(3)
    assert all(tuple(w.w.shape) == (1024, 512) for w in W.wqkv)
    Wm = LlamaWeights(LlamaConfig.from_dict(g["tcfg"]), "cpu").init_random(3)
    assert all(tuple(w.w.shape) == (1536, 512) and w.rope == (4, 128) and not w.gqa for w in Wm.wqkv)
    # the multi-head draw is the (3 H D, hidden) normal draw of the ("qkv", layer, rank) generator, as before
    import zlib
    gen = torch.Generator(device="cpu")
    gen.manual_seed((3 * 1000003 + zlib.crc32(repr(("qkv", 0, 0)).encode())) % (2 ** 31))
    want = (torch.randn(1536, 512, generator=gen, dtype=torch.float32) * 0.02).to(torch.float16)
    assert torch.equal(Wm.wqkv[0].w, want)


# ---- rotary row order --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hkv,D", [(4, 2, 64), (8, 1, 128), (4, 4, 128), (64, 8, 128), (3, 3, 32)])
def test_rope_row_order_two_head_counts(H, Hkv, D):
    from triforce_amd import ops
    order = ops.rope_row_order(H, Hkv, D)
    N = (H + 2 * Hkv) * D
    assert order.shape == (N,) and torch.equal(order.sort().values, torch.arange(N))          # a permutation
    qk = order[:(H + Hkv) * D].view(-1, 16)                                                    # 16-row panels of q and k
    for p, panel in enumerate(qk.tolist()):
        head, d0 = p // (D // 16), 8 * (p % (D // 16))
        assert panel == [head * D + d0 + e for e in range(8)] + [head * D + D // 2 + d0 + e for e in range(8)], (p, panel)
    assert torch.equal(order[(H + Hkv) * D:], torch.arange((H + Hkv) * D, N))                  # v rows in natural order
    if Hkv == H:                                                                                # the one-head-count function
        d = torch.arange(D // 2).view(D // 16, 8)
        per_head = torch.cat([d, d + D // 2], dim=1).reshape(-1)
        old_qk = (torch.arange(2 * H).view(-1, 1) * D + per_head.view(1, -1)).reshape(-1)
        assert torch.equal(order, torch.cat([old_qk, torch.arange(2 * H * D, 3 * H * D)]))


def test_packed_linear_gqa_takes_no_narrow_or_fp8_copy():
    from triforce_amd import ops
    w = torch.randn((4 + 2 * 2) * 64, 1024).to(torch.float16)
    pl = ops.PackedLinear(w, rope=(4, 2, 64), pack=True)
    assert pl.gqa and pl.rope == (4, 2, 64) and pl.wp_rope_n8 is None
    assert torch.equal(pl.wp_rope, ops.pack_weight(w[ops.rope_row_order(4, 2, 64)]))
    with pytest.raises(ValueError, match="GQA"):
        ops.Fp8Linear(pl)
    same = ops.PackedLinear(torch.zeros(3 * 4 * 64, 64, dtype=torch.float16), rope=(4, 4, 64), pack=True)
    assert not same.gqa and same.rope == (4, 64)                        # equal head counts: the multi-head weight


def test_gqa_stack_rule():
    from triforce_amd import ops
    assert ops.gqa_stack(4, 7) == (4, 1) and ops.gqa_stack(4, 8) == (4, 1)          # 28 / 32 rows: KV read once
    assert ops.gqa_stack(8, 7) == (4, 2) and ops.gqa_stack(8, 4) == (8, 1) and ops.gqa_stack(8, 1) == (8, 1)
    assert ops.gqa_stack(2, 17) == (1, 2) and ops.gqa_stack(2, 32) == (1, 2) and ops.gqa_stack(2, 16) == (2, 1)
    assert ops.gqa_stack(6, 8) == (3, 2) and ops.gqa_stack(1, 32) == (1, 1)


# ---- q-bar ---------------------------------------------------------------------------------------------------------------------
def test_group_mean_query():
    from triforce_amd import ops
    gen = torch.Generator().manual_seed(5)
    q = torch.randn(8, 128, generator=gen).to(torch.float16)
    same = ops.group_mean_query(q, 8)
    assert same is q or torch.equal(same, q)                              # g = 1: q bit for bit
    got = ops.group_mean_query(q, 2)
    want = torch.stack([q[4 * j:4 * j + 4].float().mean(dim=0) for j in range(2)]).to(torch.float16)
    assert got.dtype == torch.float16 and got.shape == (2, 128) and torch.equal(got, want)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_greedy_streams_equal_the_expanded_mha_oracle(gqa_ops):
    from triforce_amd.utils.decoding import Autoregressive, TriForce
    g = _case()
    gcfg, gsd, esd = gqa_state_dicts(g["tcfg"], g["tseed"], 2)
    dsd = specs.random_state_dict(g["dcfg"], g["dseed"], head_std=g["head_std"])
    ge = _product(g, gcfg, gsd, dsd)
    tok = Hh.FakeTokenizer()
    tok.eos_token_id = -1
    rc = ge.engine.graph_cache
    assert (rc.num_heads, rc.q_heads, ge.engine.kv_cache.num_heads) == (2, 4, 2)
    for pseed in (g["pseed"], g["pseed"] + 1):           # the second prompt: the update_graph_cache_retrieval path
        prompt = specs.random_prompt(g["tcfg"]["vocab_size"], g["prefill"], pseed)
        want = _oracle_ar(g, esd, prompt, g["gen_len"])
        _, ar = Autoregressive(tok, ge, prompt, max_len=g["gen_len"], top_k=-1, top_p=g["top_p"],
                               temperature=g["temperature"], return_tokens=True)
        assert ar == want
        res = TriForce(tok, ge, prompt, gamma=g["gamma"], max_len=g["gen_len"], top_k=-1, top_p=g["top_p"],
                       temperature=g["temperature"], return_details=True)
        n = min(len(res["tokens"]), len(want))
        assert n >= g["gen_len"] and res["tokens"][:n] == want[:n]
        # the selection ran per KV head on the group mean: (Hkv, sets) indices, chunk 0 in slot 0, rows gathered from the cache
        assert rc.init_graph and tuple(rc.last_idx[0].shape) == (2, rc.select_sets) and bool((rc.last_idx[0][:, 0] == 0).all())
        assert tuple(rc.last_scores[0].shape) == (2, rc.chunks)


def test_retrieval_selection_uses_the_group_mean(gqa_ops):
    """init_graph_cache on a GQA cache scores q-bar: same scores and rows as the oracle's retrieval ops on (K, q-bar)."""
    from triforce_amd import ops
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache
    from triforce_amd.models.config_yarn import LlamaConfig

    class _Model:
        config = LlamaConfig(hidden_size=512, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=1)
        device = torch.device("cpu")

    gen = torch.Generator().manual_seed(9)
    kv = FlashSimpleCache(_Model, 160)
    kv.k.copy_(torch.randn(kv.k.shape, generator=gen).to(torch.float16))
    kv.v.copy_(torch.randn(kv.v.shape, generator=gen).to(torch.float16))
    kv.seq_len = 128
    rc = RetrievalCache(_Model, max_budget=32, prefill=128, chunk_size=8, gamma=6)
    q = torch.randn(1, 4, 128, generator=gen).to(torch.float16)
    rc.init_graph_cache(kv, q, 0)
    qbar = ops.group_mean_query(q[0], 2)
    scores = R.retrieval_scores(kv.k[0].permute(1, 0, 2), qbar, 128, 8)
    assert torch.equal(rc.last_scores[0], scores)
    idx = R.retrieval_topk(scores, 4)
    assert torch.equal(rc.last_idx[0].long(), idx.long())
    for h in range(2):
        for j in range(4):
            c = int(idx[h, j])
            assert torch.equal(rc.k[0, h, 8 * j:8 * j + 8], kv.k[0, h, 8 * c:8 * c + 8])
            assert torch.equal(rc.v[0, h, 8 * j:8 * j + 8], kv.v[0, h, 8 * c:8 * c + 8])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _gqa_cfg(**kw):
    from triforce_amd.models.config_yarn import LlamaConfig
    return LlamaConfig(**dict(dict(hidden_size=512, intermediate_size=768, num_hidden_layers=1, num_attention_heads=4,
                                   num_key_value_heads=2, vocab_size=64), **kw))


def test_draft_model_refuses_gqa():
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as Draft
    with pytest.raises(ValueError, match="GQA.*68M draft"):
        Draft(_gqa_cfg(), "cpu")


def test_tp_and_sequoia_engines_refuse_gqa():
    from triforce_amd.models.TP_llama import DistributedLlama
    from triforce_amd.models.TP_llama_tree import DistributedLlama as TreeLlama
    for cls in (DistributedLlama, TreeLlama):
        with pytest.raises(ValueError, match="GQA.*tensor-parallel"):
            cls("unused", config=_gqa_cfg(), device="cpu", local_rank=0, world_size=1, kv_offload=True, on_chip_layers=1)


def test_offloading_and_distributed_caches_refuse_gqa():
    from triforce_amd.models import cache as C
    from triforce_amd.models.TP_layers import DistributedOffloadingConfig

    class _Model:
        config = _gqa_cfg()
        device = torch.device("cpu")

    with pytest.raises(ValueError, match="GQA.*offloading"):
        C.OffloadingFlashSimpleCache(_Model, 64)
    dcfg = DistributedOffloadingConfig(_gqa_cfg(), 0, 1)
    with pytest.raises(ValueError, match="GQA"):
        C.DistributedSimpleCache(dcfg, 64, device="cpu", on_chip_layers=1)
    with pytest.raises(ValueError, match="GQA"):
        C.DistributedRetrievalCache(dcfg, 64, device="cpu", prefill=64)


def test_fp8_tiers_refuse_gqa(monkeypatch):
    from triforce_amd.models import cache as C
    from triforce_amd.models.modeling_llama import LlamaForCausalLM

    class _Model:
        config = _gqa_cfg()
        device = torch.device("cpu")

    with pytest.raises(ValueError, match="GQA.*TRIFORCE_KV_CACHE"):
        C.FlashSimpleCache(_Model, 64, kv_dtype="fp8")
    with pytest.raises(ValueError, match="GQA.*TRIFORCE_RETRIEVAL_KV"):
        C.RetrievalCache(_Model, max_budget=32, prefill=64, kv_dtype="fp8")
    for env in ("TRIFORCE_KV_CACHE", "TRIFORCE_RETRIEVAL_KV", "TRIFORCE_RETRIEVAL_WEIGHTS"):
        monkeypatch.setenv(env, "fp8")
        with pytest.raises(ValueError, match=f"GQA.*{env}"):
            LlamaForCausalLM(_gqa_cfg(), "cpu")
        monkeypatch.delenv(env)
    LlamaForCausalLM(_gqa_cfg(), "cpu")                      # fp16 tiers: accepted
    W = LlamaForCausalLM(_gqa_cfg(), "cpu").init_random(1).weights
    with pytest.raises(ValueError, match="GQA.*TRIFORCE_RETRIEVAL_WEIGHTS"):
        W.build_fp8_()


def test_aligned_weights_refuse_gqa():
    from triforce_amd.models.aligned import AlignedSpec
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    with pytest.raises(ValueError, match="GQA.*aligned"):
        LlamaForCausalLM(_gqa_cfg(), "cpu").init_aligned(AlignedSpec())


def test_prefill_per_block_switch_refuses_gqa(monkeypatch):
    from triforce_amd import ops
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    monkeypatch.setattr(ops, "ATTN_PREFILL_ONE_LAUNCH", False)
    with pytest.raises(ValueError, match="GQA.*TRIFORCE_PREFILL_ONE_LAUNCH"):
        LlamaForCausalLM(_gqa_cfg(), "cpu")
    LlamaForCausalLM(_gqa_cfg(num_key_value_heads=4), "cpu")     # a multi-head model keeps the switch
