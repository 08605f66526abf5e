"""Attention bias on the CPU: the biased oracle against the reference's fixture, the config rules, the
loader, the rotary-order bias copy, every refusal, the unchanged bias-free draw, and the host logic end to end — the product
with every HIP op swapped for an oracle restatement against tests/attn_bias_ref.BiasedOracleTarget — with a vacuity guard:
the biases are large enough that taking them away changes the stream."""
import hashlib
import json
import os

import pytest
import torch

from oracle import ref_model as M
from oracle import specs
from tests import attn_bias_ref as B
from tests import helpers as Hh
from tests.test_gqa_cpu import gqa_ops  # noqa: F401  (fixture: cpu_ops + the grouped-query stand-ins)

ZOO = ("tiny-bias", "tiny-gqa-bias")


def _cfg(**kw):
    from triforce_amd.models.config_yarn import LlamaConfig
    return LlamaConfig(**dict(dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2,
                                   vocab_size=64, attention_bias=True), **kw))


# ---- the restatement against the reference's own run ---------------------------------------------------------------------
def test_biased_oracle_reproduces_the_reference_fixture():
    from tools.gen_attn_bias_golden import state_dicts
    fx = Hh.load_golden("attn_bias_small")
    assert [c["name"] for c in fx["cases"]] == ["mha_qkvo", "mha_qkv_zero_o"]
    assert os.path.getsize(os.path.join(Hh.GOLDEN, "attn_bias_small.pt")) <= os.path.getsize(os.path.join(Hh.GOLDEN, "forward_small.pt"))
    for g in fx["cases"]:
        tsd, dsd = state_dicts(g)
        if g["zero_o"]:
            assert all(not v.any() for k, v in tsd.items() if k.endswith("o_proj.bias"))
        prompt = specs.random_prompt(g["tcfg"]["vocab_size"], g["prefill"], g["pseed"])
        eng = B.build_oracle(g, tsd, dsd)
        l1 = eng.model.forward(prompt[:, :128], eng.kv_cache)
        l2 = eng.model.forward(prompt[:, 128:200], eng.kv_cache)
        l3 = eng.model.forward(prompt[:, 200:201], eng.kv_cache)
        for got, want in zip((l1, l2, l3), g["logits"]):
            assert torch.equal(got[0, -1], want), g["name"]
        assert M.autoregressive(eng, prompt, g["gen_len"], g["temperature"], g["top_p"]) == g["ar_tokens"]
        assert M.triforce(eng, prompt, g["gamma"], g["gen_len"], g["temperature"], g["top_p"])["tokens"] == g["triforce_tokens"]
        # the Qwen2 form: no o_proj bias at all is the zero o_proj bias, bit for bit
        if g["zero_o"]:
            bare = {k: v for k, v in tsd.items() if not k.endswith("o_proj.bias")}
            eng2 = B.build_oracle(g, bare, dsd)
            assert torch.equal(eng2.model.forward(prompt[:, :128], eng2.kv_cache), l1)


# ---- config -----------------------------------------------------------------------------------------------------------------
def test_config_rules(tmp_path):
    from triforce_amd.models.config_yarn import LlamaConfig
    assert _cfg().attention_bias is True and LlamaConfig().attention_bias is False
    assert (LlamaConfig().model_type, LlamaConfig().mlp_bias, LlamaConfig().use_sliding_window) == ("llama", False, False)
    with pytest.raises(ValueError, match="mlp_bias"):
        _cfg(mlp_bias=True)
    with pytest.raises(ValueError, match="use_sliding_window"):
        _cfg(use_sliding_window=True)

    def load(**keys):
        d = dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2, vocab_size=64, **keys)
        p = tmp_path / f"c{len(os.listdir(tmp_path))}"
        p.mkdir()
        (p / "config.json").write_text(json.dumps(d))
        return LlamaConfig.from_pretrained(str(p))
    q = load(model_type="qwen2", use_sliding_window=False, sliding_window=4096, architectures=["Qwen2ForCausalLM"])
    assert q.attention_bias is True and q.model_type == "qwen2" and not hasattr(q, "architectures")
    assert load(model_type="qwen2", attention_bias=False).attention_bias is False          # an explicit key wins
    assert load(model_type="llama").attention_bias is False
    assert load(attention_bias=True, mlp_bias=False).attention_bias is True
    with pytest.raises(ValueError, match="use_sliding_window"):
        load(model_type="qwen2", use_sliding_window=True)
    with pytest.raises(ValueError, match="mlp_bias"):
        load(attention_bias=True, mlp_bias=True)
    d = q.to_dict()
    assert d["attention_bias"] is True and d["model_type"] == "qwen2"


def test_zoo_entries():
    from triforce_amd.models import zoo
    t, tb = zoo.config("tiny"), zoo.config("tiny-bias")
    assert tb.attention_bias and tb.model_type == "llama"
    assert (tb.hidden_size, tb.num_attention_heads, tb.num_key_value_heads, tb.intermediate_size, tb.rope_scaling) == \
        (t.hidden_size, t.num_attention_heads, t.num_key_value_heads, t.intermediate_size, t.rope_scaling)
    g, gb = zoo.config("tiny-gqa"), zoo.config("tiny-gqa-bias")
    assert gb.attention_bias and gb.model_type == "qwen2"
    assert (gb.hidden_size, gb.num_attention_heads, gb.num_key_value_heads) == (g.hidden_size, g.num_attention_heads, g.num_key_value_heads)
    q = zoo.config("qwen2.5-7B-1M")
    assert (q.hidden_size, q.num_attention_heads, q.num_key_value_heads, q.head_dim, q.intermediate_size, q.num_hidden_layers,
            q.vocab_size, q.rope_theta, q.rms_norm_eps, q.attention_bias, q.rope_scaling) == \
        (3584, 28, 4, 128, 18944, 28, 152064, 1e7, 1e-6, True, None)


# ---- loader -------------------------------------------------------------------------------------------------------------------
def _loaded(name):
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.llama_core import LlamaWeights
    g = B.zoo_case(name)
    sd, _, _ = B.zoo_state_dicts(g)
    return g, sd, LlamaWeights(LlamaConfig.from_dict(g["tcfg"]), "cpu").load_state_dict(sd)


@pytest.mark.parametrize("name", ZOO)
def test_load_state_dict_fuses_the_biases(name):
    from triforce_amd import ops
    g, sd, W = _loaded(name)
    assert W.attn_bias and len(W.bqkv) == len(W.bo) == W.L
    for i in range(W.L):
        p = f"model.layers.{i}.self_attn."
        want = torch.cat([sd[p + n + "_proj.bias"] for n in ("q", "k", "v")])
        pl = W.wqkv[i]
        assert torch.equal(pl.bias, want) and pl.bias is W.bqkv[i] and pl.bias.shape == (pl.N,)
        assert torch.equal(pl.bias_rope, want[ops.rope_row_order(W.H, W.Hkv, W.D)]) and pl.wp_rope_n8 is None
        if name == "tiny-bias":
            assert torch.equal(W.wo[i].bias, sd[p + "o_proj.bias"]) and bool(W.wo[i].bias.any()) and W.wo[i].bias_rope is None
        else:                                                        # the Qwen2 form: no o_proj bias
            assert W.wo[i].bias is None and W.bo[i] is None
        assert W.wgu[i].bias is None and W.wd[i].bias is None
    assert W.lm_head.bias is None


def test_from_pretrained_directory(tmp_path):
    from safetensors.torch import save_file
    from triforce_amd.models.llama_core import save_config
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    g = B.zoo_case("tiny-gqa-bias")
    sd, _, _ = B.zoo_state_dicts(g)
    cfg = {k: v for k, v in g["tcfg"].items() if k != "attention_bias"}                 # as Qwen2 ships it: no such key
    save_config(LlamaConfig.from_dict(dict(cfg, attention_bias=True)), str(tmp_path))
    d = json.loads((tmp_path / "config.json").read_text())
    d.pop("attention_bias")
    assert d["model_type"] == "qwen2"
    (tmp_path / "config.json").write_text(json.dumps(d))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    m = LlamaForCausalLM.from_pretrained(str(tmp_path), device_map="cpu")
    assert m.config.attention_bias and m.weights.attn_bias
    p = "model.layers.1.self_attn."
    assert torch.equal(m.weights.wqkv[1].bias, torch.cat([sd[p + n + "_proj.bias"] for n in ("q", "k", "v")]))
    assert m.weights.wo[1].bias is None


def test_partial_and_mismatched_biases_are_refused():
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.llama_core import LlamaWeights
    g = B.zoo_case("tiny-bias")
    sd, _, _ = B.zoo_state_dicts(g)
    part = {k: v for k, v in sd.items() if k != "model.layers.1.self_attn.k_proj.bias"}
    with pytest.raises(ValueError, match="layer 1.*together"):
        LlamaWeights(LlamaConfig.from_dict(g["tcfg"]), "cpu").load_state_dict(part)
    with pytest.raises(ValueError, match="layer 0.*attention_bias=False"):                # biases, config says none
        LlamaWeights(LlamaConfig.from_dict(dict(g["tcfg"], attention_bias=False)), "cpu").load_state_dict(sd)
    bare = {k: v for k, v in sd.items() if not k.endswith(".bias")}
    with pytest.raises(ValueError, match="layer 0.*attention_bias=True"):                 # no biases, config says some
        LlamaWeights(LlamaConfig.from_dict(g["tcfg"]), "cpu").load_state_dict(bare)
    only_o = {k: v for k, v in sd.items() if not k.endswith(".bias") or "o_proj" in k}
    with pytest.raises(ValueError, match="layer 0.*o_proj"):
        LlamaWeights(LlamaConfig.from_dict(dict(g["tcfg"], attention_bias=False)), "cpu").load_state_dict(only_o)


# ---- PackedLinear ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hkv,D", [(2, 2, 128), (4, 2, 128), (4, 2, 64)])
def test_packed_linear_bias_rotary_copy_and_refresh(H, Hkv, D):
    from triforce_amd import ops
    N = (H + 2 * Hkv) * D
    gen = torch.Generator().manual_seed(N)
    w = torch.randn(N, 64, generator=gen).half()
    b = torch.arange(N, dtype=torch.float32).half()                     # the value names its row
    pl = ops.PackedLinear(w.clone(), rope=(H, Hkv, D), pack=True, bias=b.clone())
    order = ops.rope_row_order(H, Hkv, D)
    assert torch.equal(pl.bias_rope, b[order]) and torch.equal(pl.bias_rope.float().long(), order)
    assert torch.equal(pl.wp_rope, ops.pack_weight(w[order]))           # the weight copy and the bias copy agree row for row
    assert pl.wp_rope_n8 is None
    pl.bias.mul_(-1)
    pl.w.mul_(2)
    assert torch.equal(pl.bias_rope, b[order])                          # stale until refresh_
    pl.refresh_()
    assert torch.equal(pl.bias_rope, -b[order]) and torch.equal(pl.wp_rope, ops.pack_weight((2 * w)[order]))
    plain = ops.PackedLinear(w, pack=True, bias=b)
    assert plain.bias_rope is None and torch.equal(plain.bias, b)
    assert ops.PackedLinear(w, rope=(H, Hkv, D), pack=True).bias is None
    with pytest.raises(ValueError, match="attention bias.*Fp8Linear"):
        ops.Fp8Linear(plain)
    x = torch.randn(5, 64, generator=gen).half()
    assert torch.equal(ops.linear(x, plain, bias=plain.bias), torch.nn.functional.linear(x, w, b))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    from triforce_amd.models.aligned import AlignedSpec
    from triforce_amd.models.llama_core import LlamaWeights
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as Draft
    from triforce_amd.models.TP_llama import DistributedLlama
    from triforce_amd.models.TP_llama_tree import DistributedLlama as TreeLlama
    with pytest.raises(ValueError, match="attention bias.*68M draft"):
        Draft(_cfg(), "cpu")
    for cls in (DistributedLlama, TreeLlama):
        with pytest.raises(ValueError, match="attention bias.*tensor-parallel"):
            cls("unused", config=_cfg(), device="cpu", local_rank=0, world_size=1, kv_offload=True, on_chip_layers=1)
    with pytest.raises(ValueError, match="attention bias.*tensor-parallel weight shards"):
        LlamaWeights(_cfg(), "cpu", rank=0, world_size=2)
    with pytest.raises(ValueError, match="attention bias.*aligned"):
        LlamaForCausalLM(_cfg(), "cpu").init_aligned(AlignedSpec())
    W = LlamaForCausalLM(_cfg(), "cpu").init_random(1).weights
    with pytest.raises(ValueError, match="attention bias.*TRIFORCE_RETRIEVAL_WEIGHTS"):
        W.build_fp8_()
    monkeypatch.setenv("TRIFORCE_RETRIEVAL_WEIGHTS", "fp8")
    with pytest.raises(ValueError, match="attention bias.*TRIFORCE_RETRIEVAL_WEIGHTS=fp8"):
        LlamaForCausalLM(_cfg(), "cpu")
    LlamaForCausalLM(_cfg(attention_bias=False), "cpu")                  # a bias-free model keeps the tier
    monkeypatch.delenv("TRIFORCE_RETRIEVAL_WEIGHTS")
    for env in ("TRIFORCE_KV_CACHE", "TRIFORCE_RETRIEVAL_KV"):          # the FP8 KV tiers only consume what the GEMMs produce
        monkeypatch.setenv(env, "fp8")
        LlamaForCausalLM(_cfg(), "cpu")
        monkeypatch.delenv(env)


# ---- random draws -------------------------------------------------------------------------------------------------------------------
def _dig(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


# init_random(5) of the zoo's "tiny" / "tiny-gqa" on the commit before attention bias existed
PARENT_DRAW = {
    "tiny": dict(embed="4bca198cdf9de9e2", lm_head="5f5ec3e9911075ba", qkv0="e8480b755fb919e2", o1="b6c5658b5943eb21",
                 gu0="fa517069095e4f94", d1="b66ecc53b74954a5"),
    "tiny-gqa": dict(embed="8e4a78e916921230", lm_head="a8318f698727ff9e", qkv0="11736924f98eb518", o1="bad6b65b13593723",
                     gu0="0c748132439389de", d1="deaec2f43398bc46"),
}


@pytest.mark.parametrize("name", sorted(PARENT_DRAW))
def test_bias_free_draw_is_bit_unchanged_and_bias_draw_adds_only_biases(name):
    from triforce_amd.models import zoo
    from triforce_amd.models.llama_core import BIAS_STD, LlamaWeights

    def digests(W):
        return dict(embed=_dig(W.embed), lm_head=_dig(W.lm_head.w), qkv0=_dig(W.wqkv[0].w), o1=_dig(W.wo[1].w),
                    gu0=_dig(W.wgu[0].w), d1=_dig(W.wd[1].w))
    W = LlamaWeights(zoo.config(name), "cpu").init_random(5)
    assert digests(W) == PARENT_DRAW[name] and not W.attn_bias and W.wqkv[0].bias is None and W.wo[0].bias is None
    Wb = LlamaWeights(zoo.config(name + "-bias"), "cpu").init_random(5)
    assert digests(Wb) == PARENT_DRAW[name]                              # the matrices are the bias-free draw
    assert BIAS_STD == B.BIAS_STD
    for i in range(Wb.L):
        b = Wb.wqkv[i].bias
        assert b.shape == (Wb.wqkv[i].N,) and 0.7 * BIAS_STD < float(b.float().std()) < 1.3 * BIAS_STD
        assert (Wb.wo[i].bias is not None) == (name == "tiny")          # tiny-gqa-bias is the Qwen2 form
    before = [Wb.wqkv[0].bias.clone(), Wb.wqkv[0].bias_rope.clone()]
    ptr = Wb.wqkv[0].bias_rope.data_ptr()
    Wb.overwrite_random_(6)
    assert not torch.equal(Wb.wqkv[0].bias, before[0]) and Wb.wqkv[0].bias_rope.data_ptr() == ptr
    W6 = LlamaWeights(zoo.config(name + "-bias"), "cpu").init_random(6)
    assert torch.equal(Wb.wqkv[0].bias, W6.wqkv[0].bias) and torch.equal(Wb.wqkv[0].bias_rope, W6.wqkv[0].bias_rope)
    assert torch.equal(Wb.wqkv[1].w, W6.wqkv[1].w)
    if name == "tiny":
        assert torch.equal(Wb.wo[1].bias, W6.wo[1].bias)


# ---- end to end over the CPU stand-ins ----------------------------------------------------------------------------------------------
def _logit_bound(g, esd, prompt, oracle_logits):
    """The GPU tests' logit bound, as they derive it: twice the biased oracle's own max deviation from the fp64 truth."""
    truth = B.forward_fp64(g["ecfg"], esd, prompt[0])[-1]
    return 2.0 * float((oracle_logits.double() - truth).abs().max())


@pytest.mark.parametrize("name", ZOO)
def test_greedy_streams_equal_the_biased_oracle_and_the_biases_matter(name, gqa_ops):  # noqa: F811
    from triforce_amd.utils.decoding import Autoregressive, TriForce
    g = B.zoo_case(name)
    sd, esd, dsd = B.zoo_state_dicts(g)
    ge = Hh.build_product(g, "cpu", sd, dsd)
    W = ge.engine.model.weights
    assert W.attn_bias and W.wqkv[0].bias is not None
    tok = Hh.FakeTokenizer()
    tok.eos_token_id = -1
    prompt = specs.random_prompt(g["tcfg"]["vocab_size"], g["prefill"], g["pseed"])
    eng = B.build_oracle(g, esd, dsd)
    want = M.autoregressive(eng, prompt, g["gen_len"], g["temperature"], g["top_p"])
    _, ar = Autoregressive(tok, ge, prompt, max_len=g["gen_len"], top_k=-1, top_p=g["top_p"], temperature=g["temperature"],
                           return_tokens=True)
    assert ar == want
    res = TriForce(tok, ge, prompt, gamma=g["gamma"], max_len=g["gen_len"], top_k=-1, top_p=g["top_p"],
                   temperature=g["temperature"], return_details=True)
    n = min(len(res["tokens"]), len(want))
    assert n >= g["gen_len"] and res["tokens"][:n] == want[:n]
    # vacuity guard: the same weights with the biases zeroed give another stream, and first-step logits further from the
    # biased ones than ten times the bound the GPU tests put on the device's logits
    zsd = B.zero_biases(esd)
    zeng = B.build_oracle(g, zsd, dsd)
    zero = M.autoregressive(zeng, prompt, g["gen_len"], g["temperature"], g["top_p"])
    assert zero != want, "zeroing the biases left the greedy stream unchanged: raise BIAS_STD"
    eng.kv_cache.reset()
    zeng.kv_cache.reset()
    lb, lz = eng.inference(prompt)[0, -1], zeng.inference(prompt)[0, -1]
    bound = _logit_bound(g, esd, prompt, lb)
    apart = float((lb - lz).abs().max())
    assert apart > 10 * bound, f"biased and bias-free first-step logits are {apart:.3e} apart, GPU logit bound {bound:.3e}"
