"""QK norm on the CPU: the config rules, the loader in both directions, the unchanged norm-free draw,
the host restatement of the contract against the oracle's definition, the float64 truth against the rows recorded from
transformers' Qwen3ForCausalLM, every refusal, and the host logic end to end — the product with every HIP op swapped for an
oracle restatement against tests/qk_norm_ref.QkNormOracleTarget — with a vacuity guard: without the norms the stream differs."""
import hashlib
import json
import os

import pytest
import torch

from oracle import ref_model as M
from oracle import ref_ops as R
from oracle import specs
from tests import helpers as Hh
from tests import qk_norm_ref as Q
from tests.test_gqa_cpu import gqa_ops  # noqa: F401  (fixture: cpu_ops + the grouped-query stand-ins)

ZOO = ("tiny-qknorm", "tiny-gqa-qknorm")
GAP_TOL = 8e-3                      # as tests/test_gpu_gqa.py


def _cfg(**kw):
    from triforce_amd.models.config_yarn import LlamaConfig
    return LlamaConfig(**dict(dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2,
                                   vocab_size=64, qk_norm=True), **kw))


# ---- the CPU stand-in of the new op: the oracle's own rms_norm and rotation ---------------------------------------------------
def qk_norm_rope_append_cpu(qkv, qn, kn, eps, cos, sin, positions, k_layer, v_layer, slot0, H, D, rotate_k=True, slot0_dev=None,
                            Hkv=None):
    Hkv = H if Hkv is None else Hkv
    rows = qkv.shape[0]
    q = R.rms_norm(qkv[:, :H * D].reshape(rows, H, D), qn, eps)
    k = R.rms_norm(qkv[:, H * D:(H + Hkv) * D].reshape(rows, Hkv, D), kn, eps)
    v = qkv[:, (H + Hkv) * D:].reshape(rows, Hkv, D)
    kr = R.apply_rope(k, cos, sin, positions) if rotate_k else k
    k_layer[:, slot0:slot0 + rows] = kr.permute(1, 0, 2)
    v_layer[:, slot0:slot0 + rows] = v.permute(1, 0, 2)
    return R.apply_rope(q, cos, sin, positions).contiguous()


@pytest.fixture
def qkn_ops(gqa_ops, monkeypatch):  # noqa: F811
    monkeypatch.setattr(gqa_ops, "qk_norm_rope_append", qk_norm_rope_append_cpu)
    return gqa_ops


# ---- config -------------------------------------------------------------------------------------------------------------------
def test_config_rules(tmp_path):
    from triforce_amd.models.config_yarn import LlamaConfig, _DEFAULTS
    assert _cfg().qk_norm is True and LlamaConfig().qk_norm is False
    # every existing default is unchanged, and the key set of to_dict() of a norm-free config is the one it was
    assert _DEFAULTS == dict(
        vocab_size=32000, hidden_size=4096, intermediate_size=11008, num_hidden_layers=32, num_attention_heads=32,
        num_key_value_heads=None, hidden_act="silu", max_position_embeddings=2048, rms_norm_eps=1e-6, rope_theta=10000.0,
        rope_scaling=None, attention_bias=False, pad_token_id=None, bos_token_id=1, eos_token_id=2, _name_or_path="",
        model_type="llama", mlp_bias=False, use_sliding_window=False)
    assert set(LlamaConfig().to_dict()) == set(_DEFAULTS) and "qk_norm" not in _DEFAULTS
    assert _cfg().to_dict()["qk_norm"] is True
    assert LlamaConfig.from_dict(_cfg().to_dict()).qk_norm is True
    with pytest.raises(ValueError, match="qk_norm.*attention_bias"):
        _cfg(attention_bias=True)

    def load(**keys):
        d = dict(dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2, vocab_size=64), **keys)
        p = tmp_path / f"c{len(os.listdir(tmp_path))}"
        p.mkdir()
        (p / "config.json").write_text(json.dumps(d))
        return LlamaConfig.from_pretrained(str(p))
    q = load(model_type="qwen3", architectures=["Qwen3ForCausalLM"], head_dim=128)
    assert q.qk_norm is True and q.model_type == "qwen3" and q.head_dim == 128 and q.attention_bias is False
    assert load(model_type="qwen3", qk_norm=False).qk_norm is False                     # an explicit key wins
    assert load(model_type="llama").qk_norm is False and load(model_type="qwen2").qk_norm is False
    assert load(qk_norm=True).qk_norm is True
    assert load(model_type="qwen3").head_dim == 128                                     # head_dim absent
    with pytest.raises(ValueError, match=r"head_dim \(64\).*256 // 2 = 128"):           # Qwen3-0.6B / 1.7B / 4B / 32B style
        load(model_type="qwen3", head_dim=64)
    with pytest.raises(ValueError, match="head_dim"):
        load(model_type="llama", head_dim=256)
    with pytest.raises(ValueError, match="qk_norm.*attention_bias"):
        load(model_type="qwen3", attention_bias=True)
    # rope_scaling spelled with rope_type (Qwen3 cards, transformers 5.x) is read as type
    y = load(model_type="qwen3", rope_scaling=dict(rope_type="yarn", factor=4.0, original_max_position_embeddings=32768))
    assert y.rope_scaling["type"] == "yarn" and y.rope_scaling["factor"] == 4.0
    assert LlamaConfig(rope_scaling=dict(type="yarn", factor=4.0, original_max_position_embeddings=64)).rope_scaling == \
        dict(type="yarn", factor=4.0, original_max_position_embeddings=64)
    with pytest.raises(ValueError, match="Unknown RoPE scaling type"):
        load(rope_scaling=dict(rope_type="linear", factor=4.0))
    with pytest.raises(ValueError, match="type"):
        load(rope_scaling=dict(factor=4.0))
    # transformers 5.x: theta and scaling under rope_parameters, no top-level rope_theta — read, never ignored
    p = load(model_type="qwen3", rope_parameters=dict(rope_type="default", rope_theta=1e6))
    assert p.rope_theta == 1e6 and p.rope_scaling is None and not hasattr(p, "rope_parameters")
    p = load(model_type="qwen3", rope_parameters=dict(rope_type="yarn", rope_theta=1e6, factor=4.0,
                                                       original_max_position_embeddings=32768))
    assert p.rope_theta == 1e6 and p.rope_scaling["type"] == "yarn" and p.rope_scaling["factor"] == 4.0
    assert load(rope_theta=5e5, rope_parameters=dict(rope_type="default", rope_theta=5e5)).rope_theta == 5e5
    with pytest.raises(ValueError, match="disagree"):
        load(rope_theta=1e4, rope_parameters=dict(rope_type="default", rope_theta=1e6))
    with pytest.raises(ValueError, match="rope_parameters.*flat"):
        load(rope_parameters=dict(full_attention=dict(rope_type="default", rope_theta=1e6)))
    with pytest.raises(ValueError, match="both"):
        load(rope_scaling=dict(type="yarn", factor=2.0, original_max_position_embeddings=64),
             rope_parameters=dict(rope_type="yarn", rope_theta=1e6, factor=4.0, original_max_position_embeddings=64))
    # a QK-norm head width the kernel does not serve is refused where the config is built, not at the first forward
    with pytest.raises(ValueError, match=r"qk_norm.*head_dim in \(64, 128\).*got 32"):
        _cfg(hidden_size=64)
    assert _cfg(hidden_size=128).head_dim == 64


def test_zoo_entries():
    from triforce_amd.models import zoo
    t, tq = zoo.config("tiny"), zoo.config("tiny-qknorm")
    assert tq.qk_norm and not t.qk_norm and tq.rope_scaling is None and tq.rope_theta == 1e6
    assert (tq.hidden_size, tq.num_attention_heads, tq.num_key_value_heads, tq.intermediate_size, tq.num_hidden_layers) == \
        (t.hidden_size, t.num_attention_heads, t.num_key_value_heads, t.intermediate_size, t.num_hidden_layers)
    g, gq = zoo.config("tiny-gqa"), zoo.config("tiny-gqa-qknorm")
    assert gq.qk_norm and gq.model_type == "qwen3" and not g.qk_norm
    assert (gq.hidden_size, gq.num_attention_heads, gq.num_key_value_heads) == (g.hidden_size, g.num_attention_heads, g.num_key_value_heads)
    q = zoo.config("qwen3-8B")
    assert (q.hidden_size, q.intermediate_size, q.num_hidden_layers, q.num_attention_heads, q.num_key_value_heads, q.head_dim,
            q.vocab_size, q.rope_theta, q.rms_norm_eps, q.max_position_embeddings, q.qk_norm, q.attention_bias, q.rope_scaling) == \
        (4096, 12288, 36, 32, 8, 128, 151936, 1e6, 1e-6, 40960, True, False, None)
    assert zoo.draft_for("tiny-qknorm") == "llama-68M"


def test_yarn_tables_take_theta_only_for_a_qk_norm_config():
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.llama_core import rope_tables_for, rope_tables_yarn
    rs = dict(type="yarn", factor=4.0, original_max_position_embeddings=256)
    base = dict(hidden_size=256, num_attention_heads=2, max_position_embeddings=1024, rope_theta=1e6, rope_scaling=rs)
    want_theta = rope_tables_yarn(128, 1024, 4.0, 256, base=1e6)
    want_10k = rope_tables_yarn(128, 1024, 4.0, 256)
    assert not torch.equal(want_theta[0], want_10k[0])
    got = rope_tables_for(LlamaConfig(qk_norm=True, **base))
    assert torch.equal(got[0], want_theta[0]) and torch.equal(got[1], want_theta[1])
    for kw in (dict(), dict(model_type="qwen2", attention_bias=True)):                  # Llama / Qwen2: base 10000, as before
        got = rope_tables_for(LlamaConfig(**base, **kw))
        assert torch.equal(got[0], want_10k[0]) and torch.equal(got[1], want_10k[1])
    # the fixture's samples (checked against transformers' YaRN when it was written)
    y = Hh.load_golden("qk_norm_small")["yarn"]
    cfg = LlamaConfig(hidden_size=2 * y["head_dim"], num_attention_heads=2, rope_theta=y["rope_theta"], qk_norm=True,
                      max_position_embeddings=int(y["factor"] * y["original_max_position_embeddings"]),
                      rope_scaling=dict(rope_type="yarn", factor=y["factor"],
                                        original_max_position_embeddings=y["original_max_position_embeddings"]))
    cos, sin = rope_tables_for(cfg)
    assert torch.equal(cos[y["positions"]], y["cos"]) and torch.equal(sin[y["positions"]], y["sin"])


# ---- loader -------------------------------------------------------------------------------------------------------------------
def _loaded(name):
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.llama_core import LlamaWeights
    g = Q.zoo_case(name)
    sd, _, _ = Q.zoo_state_dicts(g)
    return g, sd, LlamaWeights(LlamaConfig.from_dict(g["tcfg"]), "cpu").load_state_dict(sd)


@pytest.mark.parametrize("name", ZOO)
def test_load_state_dict_takes_the_norms_and_packs_a_plain_qkv(name):
    g, sd, W = _loaded(name)
    assert W.qk_norm and len(W.qn) == len(W.kn) == W.L
    for i in range(W.L):
        p = f"model.layers.{i}.self_attn."
        assert torch.equal(W.qn[i], sd[p + "q_norm.weight"]) and torch.equal(W.kn[i], sd[p + "k_norm.weight"])
        assert W.qn[i].shape == (W.D,) and W.qn[i].dtype == torch.float16
        pl = W.wqkv[i]
        assert pl.rope is None and pl.wp_rope is None and pl.wp_rope_n8 is None and pl.bias is None       # no rotary-order copy
        assert torch.equal(pl.w, torch.cat([sd[p + n + "_proj.weight"] for n in ("q", "k", "v")]))


def test_loader_refuses_a_mismatch_in_both_directions():
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.llama_core import LlamaWeights
    g = Q.zoo_case("tiny-qknorm")
    sd, _, _ = Q.zoo_state_dicts(g)
    plain_cfg = {k: v for k, v in g["tcfg"].items() if k != "qk_norm"}
    with pytest.raises(ValueError, match="layer 0.*q_norm / k_norm weights.*qk_norm=False"):       # norms, config says none
        LlamaWeights(LlamaConfig.from_dict(plain_cfg), "cpu").load_state_dict(sd)
    with pytest.raises(ValueError, match="layer 0.*no q_norm / k_norm weights.*qk_norm=True"):      # no norms, config says some
        LlamaWeights(LlamaConfig.from_dict(g["tcfg"]), "cpu").load_state_dict(Q.without_norms(sd))
    for gone, left in (("k", "q"), ("q", "k")):
        part = {k: v for k, v in sd.items() if k != f"model.layers.1.self_attn.{gone}_norm.weight"}
        with pytest.raises(ValueError, match=f"layer 1.*{left}_norm only"):
            LlamaWeights(LlamaConfig.from_dict(g["tcfg"]), "cpu").load_state_dict(part)
        lone = dict(Q.without_norms(sd))                                # one stray norm weight in a norm-free checkpoint
        lone[f"model.layers.0.self_attn.{left}_norm.weight"] = sd[f"model.layers.0.self_attn.{left}_norm.weight"]
        with pytest.raises(ValueError, match=f"layer 0.*{left}_norm only"):
            LlamaWeights(LlamaConfig.from_dict(plain_cfg), "cpu").load_state_dict(lone)
    bad = dict(sd)
    bad["model.layers.0.self_attn.q_norm.weight"] = torch.ones(64, dtype=torch.float16)
    with pytest.raises(ValueError, match="layer 0.*q_norm weight has 64 entries"):
        LlamaWeights(LlamaConfig.from_dict(g["tcfg"]), "cpu").load_state_dict(bad)
    # a norm-free checkpoint with a norm-free config loads as it always did
    LlamaWeights(LlamaConfig.from_dict(plain_cfg), "cpu").load_state_dict(Q.without_norms(sd))


def test_from_pretrained_directory_of_the_qwen3_form(tmp_path):
    from safetensors.torch import save_file
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    g = Q.zoo_case("tiny-gqa-qknorm")
    sd, _, _ = Q.zoo_state_dicts(g)
    d = {k: v for k, v in g["tcfg"].items() if k not in ("qk_norm", "_name_or_path")}       # as Qwen3 ships it: no such key
    d.update(head_dim=128, architectures=["Qwen3ForCausalLM"])
    assert d["model_type"] == "qwen3"
    (tmp_path / "config.json").write_text(json.dumps(d))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    m = LlamaForCausalLM.from_pretrained(str(tmp_path), device_map="cpu")
    assert m.config.qk_norm and m.weights.qk_norm
    assert torch.equal(m.weights.kn[1], sd["model.layers.1.self_attn.k_norm.weight"])
    # the silent wrong-model load is gone: the same directory read as a Llama config is refused
    d["model_type"] = "llama"
    (tmp_path / "config.json").write_text(json.dumps(d))
    with pytest.raises(ValueError, match="layer 0.*qk_norm=False"):
        LlamaForCausalLM.from_pretrained(str(tmp_path), device_map="cpu")


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    from triforce_amd.models.aligned import AlignedSpec
    from triforce_amd.models.llama_core import LlamaWeights
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as Draft
    from triforce_amd.models.TP_llama import DistributedLlama
    from triforce_amd.models.TP_llama_tree import DistributedLlama as TreeLlama
    with pytest.raises(ValueError, match="QK norm.*68M draft"):
        Draft(_cfg(), "cpu")
    for cls in (DistributedLlama, TreeLlama):
        with pytest.raises(ValueError, match="QK norm.*tensor-parallel"):
            cls("unused", config=_cfg(), device="cpu", local_rank=0, world_size=1, kv_offload=True, on_chip_layers=1)
    with pytest.raises(ValueError, match="QK norm.*tensor-parallel weight shards"):
        LlamaWeights(_cfg(), "cpu", rank=0, world_size=2)
    with pytest.raises(ValueError, match="QK norm.*aligned"):
        LlamaForCausalLM(_cfg(), "cpu").init_aligned(AlignedSpec())
    W = LlamaForCausalLM(_cfg(), "cpu").init_random(1).weights
    with pytest.raises(ValueError, match="QK norm.*TRIFORCE_RETRIEVAL_WEIGHTS.*Fp8Linear"):
        W.build_fp8_()
    monkeypatch.setenv("TRIFORCE_RETRIEVAL_WEIGHTS", "fp8")
    with pytest.raises(ValueError, match="QK norm.*TRIFORCE_RETRIEVAL_WEIGHTS=fp8"):
        LlamaForCausalLM(_cfg(), "cpu")
    LlamaForCausalLM(_cfg(qk_norm=False), "cpu")                         # a norm-free model keeps the tier
    monkeypatch.delenv("TRIFORCE_RETRIEVAL_WEIGHTS")
    for env in ("TRIFORCE_KV_CACHE", "TRIFORCE_RETRIEVAL_KV"):          # the FP8 KV tiers only consume what the kernel writes
        monkeypatch.setenv(env, "fp8")
        LlamaForCausalLM(_cfg(), "cpu")
        monkeypatch.delenv(env)


# ---- random draws -------------------------------------------------------------------------------------------------------------
def _dig(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


# init_random(5) of the zoo's "tiny" / "tiny-gqa" on the commits before attention bias and QK norm existed (the values
# tests/test_attn_bias_cpu.py pins)
PARENT_DRAW = {
    "tiny": dict(embed="4bca198cdf9de9e2", lm_head="5f5ec3e9911075ba", qkv0="e8480b755fb919e2", o1="b6c5658b5943eb21",
                 gu0="fa517069095e4f94", d1="b66ecc53b74954a5"),
    "tiny-gqa": dict(embed="8e4a78e916921230", lm_head="a8318f698727ff9e", qkv0="11736924f98eb518", o1="bad6b65b13593723",
                     gu0="0c748132439389de", d1="deaec2f43398bc46"),
}


@pytest.mark.parametrize("name", sorted(PARENT_DRAW))
def test_norm_free_draw_is_bit_unchanged_and_norm_draw_adds_only_norms(name):
    from triforce_amd.models import zoo
    from triforce_amd.models.llama_core import QK_NORM_STD, LlamaWeights

    def digests(W):
        return dict(embed=_dig(W.embed), lm_head=_dig(W.lm_head.w), qkv0=_dig(W.wqkv[0].w), o1=_dig(W.wo[1].w),
                    gu0=_dig(W.wgu[0].w), d1=_dig(W.wd[1].w))
    W = LlamaWeights(zoo.config(name), "cpu").init_random(5)
    assert digests(W) == PARENT_DRAW[name] and not W.qk_norm and W.qn == [] and W.kn == []
    Wn = LlamaWeights(zoo.config(name + "-qknorm"), "cpu").init_random(5)
    assert digests(Wn) == PARENT_DRAW[name]                              # the matrices are the norm-free draw
    assert QK_NORM_STD == Q.QK_NORM_STD and Wn.wqkv[0].rope is None
    for i in range(Wn.L):
        for w in (Wn.qn[i], Wn.kn[i]):
            f = w.float()
            assert w.shape == (Wn.D,) and abs(float(f.mean()) - 1) < 0.1 and 0.6 * QK_NORM_STD < float(f.std()) < 1.4 * QK_NORM_STD
        assert not torch.equal(Wn.qn[i], Wn.kn[i])
    before, ptr = Wn.qn[0].clone(), Wn.qn[0].data_ptr()
    Wn.overwrite_random_(6)
    assert not torch.equal(Wn.qn[0], before) and Wn.qn[0].data_ptr() == ptr
    W6 = LlamaWeights(zoo.config(name + "-qknorm"), "cpu").init_random(6)
    assert all(torch.equal(a, b) for a, b in zip(Wn.qn + Wn.kn, W6.qn + W6.kn)) and torch.equal(Wn.wqkv[1].w, W6.wqkv[1].w)


# ---- the contract's host restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hkv,D", [(2, 2, 128), (4, 2, 128), (4, 2, 64)])
@pytest.mark.parametrize("rotate_k", [True, False])
def test_qk_norm_rope_ref_is_the_oracles_definition(H, Hkv, D, rotate_k):
    from triforce_amd import ops
    gen = torch.Generator().manual_seed(H * 1000 + D)
    rows = 37
    qkv = torch.randn(rows, (H + 2 * Hkv) * D, generator=gen).half()
    qn, kn = ((1 + 0.25 * torch.randn(D, generator=gen)).half() for _ in range(2))
    cos, sin = R.rope_tables_plain(D, 512, 1e6)
    pos = torch.randint(0, 512, (rows,), generator=gen)
    pos[0] = 0
    q, k, v = ops.qk_norm_rope_ref(qkv, qn, kn, 1e-6, cos, sin, pos, H, D, rotate_k=rotate_k, Hkv=Hkv)
    kl, vl = torch.zeros(Hkv, rows + 3, D).half(), torch.zeros(Hkv, rows + 3, D).half()
    want_q = qk_norm_rope_append_cpu(qkv, qn, kn, 1e-6, cos, sin, pos, kl, vl, 2, H, D, rotate_k=rotate_k, Hkv=Hkv)
    assert torch.equal(q, want_q)
    assert torch.equal(k, kl[:, 2:2 + rows].permute(1, 0, 2)) and torch.equal(v, vl[:, 2:2 + rows].permute(1, 0, 2))
    assert torch.equal(v.reshape(rows, -1), qkv[:, (H + Hkv) * D:])
    assert not kl[:, :2].any() and not kl[:, 2 + rows:].any()


def test_exact_probe_inputs_sum_exactly_in_any_order():
    """The premise of the GPU exact probes: multiples of 2^-4 with |x| <= 8 have squares that are multiples of 2^-8, at most
    2^6 each; 128 of them sum to at most 2^13 = 2^21 units of 2^-8 < 2^24, so every partial sum of any order is exact.
    (A check of arithmetic, not of project code: unlike the other tests of this file it does not depend on the change it
    came with.  The host restatement's own sum is held to the same statement below.)"""
    from triforce_amd import ops
    gen = torch.Generator().manual_seed(4)
    x = (torch.randint(-128, 129, (4096, 128), generator=gen).float() / 16)
    assert float(x.abs().max()) <= 8
    perm = torch.randperm(128, generator=gen)
    a = x.pow(2).sum(-1)
    b = x[:, perm].pow(2).cumsum(-1)[:, -1]
    c = x.double().pow(2).sum(-1)
    assert torch.equal(a, b) and torch.equal(a.double(), c) and float(a.max()) <= 2 ** 13
    # ... so ops.qk_norm_rope_ref is invariant under a permutation of a head's pairs when weights and tables are constant
    xh, one = x[:64].half(), torch.ones(128, dtype=torch.float16)
    cos, sin = torch.ones(1, 128).half(), torch.zeros(1, 128).half()
    pos = torch.zeros(64, dtype=torch.int64)
    q1 = ops.qk_norm_rope_ref(torch.cat([xh, xh, xh], 1), one, one, 1e-6, cos, sin, pos, 1, 128)[0]
    xp = xh[:, perm]
    q2 = ops.qk_norm_rope_ref(torch.cat([xp, xp, xp], 1), one, one, 1e-6, cos, sin, pos, 1, 128)[0]
    assert torch.equal(q1[:, 0][:, perm], q2[:, 0])


# ---- the float64 truth against transformers' rows --------------------------------------------------------------------------------
def test_forward_fp64_reproduces_the_recorded_transformers_rows():
    fx = Hh.load_golden("qk_norm_small")
    assert [c["name"] for c in fx["cases"]] == ["mha", "gqa"] and fx["fp64_bound"] == 1e-8
    assert os.path.getsize(os.path.join(Hh.GOLDEN, "qk_norm_small.pt")) < 256 * 1024
    for g in fx["cases"]:
        assert g["fp64_dev"] < fx["fp64_bound"] and g["norm_std"] == Q.QK_NORM_STD
        sd, esd = Q.state_dicts_of(g["tcfg"], g["tseed"], g["nseed"], g["head_std"])
        ids = specs.random_prompt(g["tcfg"]["vocab_size"], g["prompt_len"] + g["decode"], g["pseed"])[0]
        got = Q.forward_fp64(g["tcfg"], sd, ids)[g["prompt_len"] - g["last"]:]
        want = g["logits"]                                              # HF's float64 rows, stored as fp32
        assert got.shape == want.shape == (g["last"] + g["decode"], g["tcfg"]["vocab_size"])
        # stored fp32: half an fp32 ulp of the largest logit, plus the float64 bound
        tol = float(want.abs().max()) * 2.0 ** -24 + fx["fp64_bound"]
        assert float((got - want.double()).abs().max()) <= tol, g["name"]
        # a grouped-query model is its expanded multi-head state dict
        ecfg = dict(g["tcfg"], num_key_value_heads=g["tcfg"]["num_attention_heads"])
        assert float((Q.forward_fp64(ecfg, esd, ids)[g["prompt_len"] - g["last"]:] - got).abs().max()) < 1e-12
        # and the fp16 oracle restatement sits at fp16 distance from it, the norm-free model nowhere near
        ot = Q.QkNormOracleTarget(ecfg, esd)
        lo = ot.forward(ids[None, :g["prompt_len"]], M.FullCache(ecfg, 256))[0, -g["last"]:]
        assert float((lo.double() - got[:g["last"]]).abs().max()) < 0.05
        plain = Q.forward_fp64(g["tcfg"], Q.without_norms(sd), ids)[g["prompt_len"] - g["last"]:]
        assert float((plain - got).abs().max()) > 0.1


# ---- end to end over the CPU stand-ins -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ZOO)
def test_greedy_streams_equal_the_qk_norm_oracle_and_the_norms_matter(name, qkn_ops):
    from triforce_amd.utils.decoding import Autoregressive, TriForce
    g = Q.zoo_case(name)
    sd, esd, dsd = Q.zoo_state_dicts(g)
    ge = Hh.build_product(g, "cpu", sd, dsd)
    W = ge.engine.model.weights
    assert W.qk_norm and W.wqkv[0].rope is None
    tok = Hh.FakeTokenizer()
    tok.eos_token_id = -1
    prompt = specs.random_prompt(g["tcfg"]["vocab_size"], g["prefill"], g["pseed"])
    eng = Q.build_oracle(g, esd, dsd)
    want = M.autoregressive(eng, prompt, g["gen_len"], g["temperature"], g["top_p"])
    _, ar = Autoregressive(tok, ge, prompt, max_len=g["gen_len"], top_k=-1, top_p=g["top_p"], temperature=g["temperature"],
                           return_tokens=True)
    assert ar == want
    res = TriForce(tok, ge, prompt, gamma=g["gamma"], max_len=g["gen_len"], top_k=-1, top_p=g["top_p"],
                   temperature=g["temperature"], return_details=True)
    n = min(len(res["tokens"]), len(want))
    assert n >= g["gen_len"] and res["tokens"][:n] == want[:n]
    # vacuity guard: the same matrices with both norm weights set to 1 and the norm removed give another stream, and
    # first-step logits more than ten times GAP_TOL away
    zsd = Q.without_norms(Q.unit_norms(esd))
    zeng = Q.build_oracle(g, zsd, dsd)
    zero = M.autoregressive(zeng, prompt, g["gen_len"], g["temperature"], g["top_p"])
    assert zero != want, "removing the norms left the greedy stream unchanged"
    eng.kv_cache.reset()
    zeng.kv_cache.reset()
    ln, lz = eng.inference(prompt)[0, -1], zeng.inference(prompt)[0, -1]
    apart = float((ln - lz).abs().max())
    assert apart > 10 * GAP_TOL, f"normed and norm-free first-step logits are only {apart:.3e} apart"
