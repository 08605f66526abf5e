"""Attention bias on the oracle side: a seeded rule for the q / k / v / o biases and the oracle target
restated with them.  TEST INFRASTRUCTURE ONLY.  tools/gen_attn_bias_golden.py pins ``BiasedOracleTarget`` against the
UNMODIFIED reference built with ``attention_bias=True`` (logits bit-identical, streams identical) and writes
tests/golden/attn_bias_small.pt; the tests take the biased oracle as their reference from there.

Everything but the four projections is the oracle's own: engine, caches and decode loops of oracle/ref_model.py are reused
as they are.  A grouped-query model is, as in DESIGN section 22, its expanded multi-head state dict: k_proj / v_proj head
blocks — weights AND biases — repeated once per query head of the group (``expand_gqa``).
"""
import zlib

import torch
import torch.nn.functional as F

from oracle import ref_model as M
from oracle import ref_ops as R

BIAS_STD = 0.5                      # as triforce_amd.models.llama_core.BIAS_STD: large enough to move the greedy stream
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj")


def bias_of(seed, layer, name, n, std=BIAS_STD):
    """The seeded bias of one projection: N(0, std) fp16 from a generator of its own, keyed by (seed, layer, name)."""
    g = torch.Generator(device="cpu").manual_seed((seed * 1000003 + zlib.crc32(repr(("bias", layer, name)).encode())) % (2 ** 31))
    return (torch.randn(n, generator=g, dtype=torch.float32) * std).to(torch.float16)


def add_biases(cfg, sd, seed, o_bias=True, std=BIAS_STD, zero_o=False):
    """``sd`` + self_attn.{q,k,v}_proj.bias (and o_proj.bias when ``o_bias``) drawn by ``bias_of``; the bias of a projection
    has as many entries as its weight has rows, so a grouped-query dict gets Hkv * D entries for k and v.  ``zero_o``: an
    o_proj bias of zeros (what the reference's module holds for a checkpoint of the Qwen2 form)."""
    out = dict(sd)
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}.self_attn."
        for name in PROJ:
            n = sd[p + name + ".weight"].shape[0]
            if name == "o_proj":
                if zero_o:
                    out[p + name + ".bias"] = torch.zeros(n, dtype=torch.float16)
                elif o_bias:
                    out[p + name + ".bias"] = bias_of(seed, i, name, n, std)
            else:
                out[p + name + ".bias"] = bias_of(seed, i, name, n, std)
    return out


def zero_biases(sd):
    """The same state dict with every attention bias zeroed (the vacuity guard's comparison)."""
    return {k: (torch.zeros_like(v) if k.endswith("_proj.bias") else v) for k, v in sd.items()}


def expand_gqa(cfg, sd):
    """(multi-head config, expanded state dict) of a grouped-query (config, state dict): k_proj / v_proj head blocks of the
    weights and of the biases repeated g = H / Hkv times — the DESIGN section 22 identity, with biases."""
    H, Hkv, hid = cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["hidden_size"]
    D, g = hid // H, H // Hkv
    out = dict(sd)
    for name, w in sd.items():
        if "k_proj" in name or "v_proj" in name:
            if name.endswith(".weight"):
                out[name] = w.view(Hkv, D, hid).repeat_interleave(g, dim=0).reshape(H * D, hid).contiguous()
            else:
                out[name] = w.view(Hkv, D).repeat_interleave(g, dim=0).reshape(H * D).contiguous()
    return dict(cfg, num_key_value_heads=H), out


class BiasedOracleTarget(M.OracleTarget):
    """oracle.ref_model.OracleTarget with the reference's ``bias=config.attention_bias`` projections
    (models/modeling_llama.py:174-177): q / k / v = F.linear(h, W, b), o = F.linear(a, Wo, bo).  A projection without a bias
    entry in the state dict is bias-free.  The rest of the forward is OracleTarget.forward, line for line."""

    def bias(self, i, name):
        return self.sd.get(f"model.layers.{i}.{name}.bias")

    def proj(self, x, i, name):
        return F.linear(x, self.layer(i, name), self.bias(i, name))

    def forward(self, input_ids, kv_cache, graph_cache=None, position_ids=None, spec=False):
        q_len = input_ids.shape[1]
        if position_ids is None:
            position_ids = torch.arange(kv_cache.seq_len, kv_cache.seq_len + q_len).unsqueeze(0)
        pos = position_ids[0]
        x = F.embedding(input_ids[0], self.sd["model.embed_tokens.weight"])
        for i in range(self.L):
            res = x
            h = R.rms_norm(x, self.layer(i, "input_layernorm"), self.eps)
            q = self.proj(h, i, "self_attn.q_proj").view(q_len, self.H, self.D)
            k = self.proj(h, i, "self_attn.k_proj").view(q_len, self.H, self.D)
            v = self.proj(h, i, "self_attn.v_proj").view(q_len, self.H, self.D)
            q = R.apply_rope(q, self.cos, self.sin, pos)
            k = R.apply_rope(k, self.cos, self.sin, pos)
            if spec:
                kk, vv = graph_cache.update(k, v, i)
            else:
                kk, vv = kv_cache.update(k, v, i)
                if q_len == 1 and isinstance(graph_cache, M.RetrievalCacheO):
                    if not graph_cache.init_graph:
                        graph_cache.init_graph_cache(kv_cache, q, i)
                    else:
                        graph_cache.update_graph_cache_retrieval(kv_cache, q, i)
            a = R.attn_kvcache(q, kk, vv, self.scale, causal=True)
            a = self.proj(a.reshape(q_len, self.H * self.D), i, "self_attn.o_proj")
            x = res + a
            res = x
            h = R.rms_norm(x, self.layer(i, "post_attention_layernorm"), self.eps)
            m = R.silu_mul(R.linear(h, self.layer(i, "mlp.gate_proj")), R.linear(h, self.layer(i, "mlp.up_proj")))
            x = res + R.linear(m, self.layer(i, "mlp.down_proj"))
        x = R.rms_norm(x, self.sd["model.norm.weight"], self.eps)
        return R.linear(x, self.sd["lm_head.weight"]).float().unsqueeze(0)


def forward_fp64(cfg, sd, ids):
    """The truth of the logit checks: the model of (config, state dict) — multi-head or grouped-query, biased or not —
    evaluated in float64 on the stored fp16 weights, biases and RoPE tables, with NO intermediate rounding; ``ids`` (T,) are
    fed as one causal block, which is what any chunking of them computes.  -> (T, V) float64 logits."""
    H, Hkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    D, eps, T = R.head_dim_of(cfg), cfg["rms_norm_eps"], ids.numel()
    cos, sin = (t.double() for t in R.rope_tables_for(cfg))
    scale = float(R.softmax_scale_for(D))
    pos = torch.arange(T)

    def w(name):
        return sd[name].double()

    def lin(x, i, name):
        y = x @ w(f"model.layers.{i}.{name}.weight").t()
        b = sd.get(f"model.layers.{i}.{name}.bias")
        return y if b is None else y + b.double()

    def norm(x, weight):
        return weight.double() * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))

    def rope(x):                                                     # (T, heads, D)
        c, s = cos[pos][:, None, :], sin[pos][:, None, :]
        rot = torch.cat([-x[..., D // 2:], x[..., :D // 2]], dim=-1)
        return x * c + rot * s

    x = w("model.embed_tokens.weight")[ids.reshape(-1)]
    mask = torch.full((T, T), float("-inf"), dtype=torch.float64).triu(1)
    for i in range(cfg["num_hidden_layers"]):
        h = norm(x, sd[f"model.layers.{i}.input_layernorm.weight"])
        q = rope(lin(h, i, "self_attn.q_proj").view(T, H, D))
        k = rope(lin(h, i, "self_attn.k_proj").view(T, Hkv, D)).repeat_interleave(H // Hkv, dim=1)
        v = lin(h, i, "self_attn.v_proj").view(T, Hkv, D).repeat_interleave(H // Hkv, dim=1)
        s = torch.einsum("qhd,khd->hqk", q, k) * scale + mask
        a = torch.einsum("hqk,khd->qhd", torch.softmax(s, dim=-1), v).reshape(T, H * D)
        x = x + lin(a, i, "self_attn.o_proj")
        h = norm(x, sd[f"model.layers.{i}.post_attention_layernorm.weight"])
        g = lin(h, i, "mlp.gate_proj")
        x = x + lin(g / (1.0 + torch.exp(-g)) * lin(h, i, "mlp.up_proj"), i, "mlp.down_proj")
    return norm(x, sd["model.norm.weight"]) @ w("lm_head.weight").t()


def zoo_case(name, **over):
    """A golden-style case dict for the zoo's "tiny-bias" / "tiny-gqa-bias" target shape at small_gamma6's vocabulary and
    draft: tcfg = the PRODUCT's config (grouped-query and attention_bias / model_type as the zoo has them), ecfg = the
    multi-head config the oracle runs."""
    from tests import helpers as Hh
    from triforce_amd.models import zoo
    g = dict(Hh.load_golden("small_gamma6"))
    z = dict(zoo.CONFIGS[name])
    tcfg = specs_config(z, g["dcfg"]["vocab_size"])
    g.update(dict(dict(name=name, tcfg=tcfg, ecfg=dict(tcfg, num_key_value_heads=tcfg["num_attention_heads"]), tseed=2911,
                       bseed=2912, prefill=512, gen_len=24, budget=128), **over))
    return g


def specs_config(z, vocab):
    from oracle import specs
    cfg = specs.llama_config(z["hidden_size"], z["intermediate_size"], z["num_hidden_layers"], z["num_attention_heads"],
                             vocab_size=vocab, max_position_embeddings=4096, rope_scaling=z["rope_scaling"],
                             rms_norm_eps=z["rms_norm_eps"], name=z["_name_or_path"])
    cfg.update(num_key_value_heads=z.get("num_key_value_heads", z["num_attention_heads"]), attention_bias=True,
               model_type=z.get("model_type", "llama"))
    return cfg


def zoo_state_dicts(g):
    """(product state dict, expanded multi-head state dict for the oracle, draft state dict) of a ``zoo_case``: the seeded
    multi-head draw with k_proj / v_proj cut to the first Hkv heads, biases from ``add_biases`` (no o_proj bias for the Qwen2
    form), and the same with the KV head blocks repeated."""
    from oracle import specs
    tcfg = g["tcfg"]
    H, Hkv = tcfg["num_attention_heads"], tcfg["num_key_value_heads"]
    D = tcfg["hidden_size"] // H
    sd = specs.random_state_dict(g["ecfg"], g["tseed"], head_std=g["head_std"])
    for name in list(sd):
        if "k_proj" in name or "v_proj" in name:
            sd[name] = sd[name][:Hkv * D].contiguous()
    sd = add_biases(tcfg, sd, g["bseed"], o_bias=tcfg["model_type"] != "qwen2")
    _, esd = expand_gqa(tcfg, sd)
    return sd, esd, specs.random_state_dict(g["dcfg"], g["dseed"], head_std=g["head_std"])


def build_oracle(g, tsd, dsd):
    """The oracle engine of a golden-style case dict ``g`` (tests/helpers.build_oracle) around a BiasedOracleTarget.  ``tsd``
    must be multi-head (``expand_gqa`` first for a grouped-query model), with ``g["ecfg"]`` (else ``g["tcfg"]``) its config."""
    recent = 256 - 16 - g["gamma"]
    cfg = g.get("ecfg", g["tcfg"])
    ot, od = BiasedOracleTarget(cfg, tsd), M.OracleDraft(g["dcfg"], dsd)
    okv = M.FullCache(cfg, g["prefill"] + g["gen_len"] + 16)
    ogc = M.RetrievalCacheO(cfg, g["budget"], g["prefill"], g["chunk"], g["gamma"])
    odc = M.StreamingCacheO(g["dcfg"], gamma=g["gamma"], start_size=16, recent_size=recent)
    return M.OracleEngine(ot, okv, ogc, od, odc, g["temperature"], g["top_p"])


def teacher_forced_gaps(eng, prompt, stream):
    """tests/helpers.teacher_forced_gaps on a given (biased) oracle engine: for every token of ``stream`` how far its oracle
    logit is below the oracle's best given the same prefix."""
    eng.kv_cache.reset()
    logits = eng.inference(prompt)[0, -1]
    gaps = [float(logits.max() - logits[stream[0]])]
    for i in range(len(stream) - 1):
        logits = eng.model.forward(torch.tensor([[stream[i]]]), eng.kv_cache, None)[0, -1]
        gaps.append(float(logits.max() - logits[stream[i + 1]]))
    return gaps
