"""QK norm on the oracle side: a seeded rule for the q_norm / k_norm weights, the oracle target restated
with the two norms, and the float64 truth.  TEST INFRASTRUCTURE ONLY.  tools/gen_qk_norm_golden.py pins ``forward_fp64``
against ``transformers``' Qwen3ForCausalLM evaluated in float64 (the independent definition of the architecture) and writes
tests/golden/qk_norm_small.pt; the tests take these definitions as their reference from there and never import transformers.

Everything but the two norms is the oracle's own: engine, caches and decode loops of oracle/ref_model.py are reused as they
are.  A grouped-query model is, as in DESIGN section 22, its expanded multi-head state dict (``expand_gqa``): k_proj / v_proj
head blocks repeated once per query head of the group; the k_norm weight is per head WIDTH and stays as it is.
"""
import zlib

import torch
import torch.nn.functional as F

from oracle import ref_model as M
from oracle import ref_ops as R

QK_NORM_STD = 0.25                  # as triforce_amd.models.llama_core.QK_NORM_STD
NORMS = ("q_norm", "k_norm")


def norm_weight_of(seed, layer, name, D, std=QK_NORM_STD):
    """The seeded weight of one norm: 1 + std * N(0, 1), fp16, from a generator of its own keyed by (seed, layer, name)."""
    g = torch.Generator(device="cpu").manual_seed((seed * 1000003 + zlib.crc32(repr(("qk_norm", layer, name)).encode())) % (2 ** 31))
    return (1.0 + std * torch.randn(D, generator=g, dtype=torch.float32)).to(torch.float16)


def add_norms(cfg, sd, seed, std=QK_NORM_STD):
    """``sd`` + self_attn.{q,k}_norm.weight ([head_dim] each) drawn by ``norm_weight_of``."""
    out = dict(sd)
    D = R.head_dim_of(cfg)
    for i in range(cfg["num_hidden_layers"]):
        for name in NORMS:
            out[f"model.layers.{i}.self_attn.{name}.weight"] = norm_weight_of(seed, i, name, D, std)
    return out


def unit_norms(sd):
    """The same state dict with both norm weights set to 1 (one half of the vacuity guard's comparison)."""
    return {k: (torch.ones_like(v) if "_norm.weight" in k and "self_attn" in k else v) for k, v in sd.items()}


def without_norms(sd):
    """The same state dict with the q_norm / k_norm weights taken out: the norm-free model of the same matrices."""
    return {k: v for k, v in sd.items() if not ("self_attn" in k and "_norm.weight" in k)}


def expand_gqa(cfg, sd):
    """(multi-head config, expanded state dict) of a grouped-query (config, state dict): k_proj / v_proj head blocks repeated
    g = H / Hkv times — the DESIGN section 22 identity.  The norm weights are per head width: unchanged."""
    H, Hkv, hid = cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["hidden_size"]
    D, g = hid // H, H // Hkv
    out = dict(sd)
    for name, w in sd.items():
        if ("k_proj" in name or "v_proj" in name) and name.endswith(".weight"):
            out[name] = w.view(Hkv, D, hid).repeat_interleave(g, dim=0).reshape(H * D, hid).contiguous()
    return dict(cfg, num_key_value_heads=H), out


class QkNormOracleTarget(M.OracleTarget):
    """oracle.ref_model.OracleTarget with a per-head RMSNorm of q and k in front of the rotation: the oracle's own rms_norm
    (fp32 normalise -> fp16 -> times weight) over the last axis of the (rows, heads, D) projections.  A layer without norm
    weights in the state dict is norm-free.  The rest of the forward is OracleTarget.forward, line for line."""

    def qk(self, x, i, name):
        w = self.sd.get(f"model.layers.{i}.self_attn.{name}.weight")
        return x if w is None else R.rms_norm(x, w, self.eps)

    def forward(self, input_ids, kv_cache, graph_cache=None, position_ids=None, spec=False):
        q_len = input_ids.shape[1]
        if position_ids is None:
            position_ids = torch.arange(kv_cache.seq_len, kv_cache.seq_len + q_len).unsqueeze(0)
        pos = position_ids[0]
        x = F.embedding(input_ids[0], self.sd["model.embed_tokens.weight"])
        for i in range(self.L):
            res = x
            h = R.rms_norm(x, self.layer(i, "input_layernorm"), self.eps)
            q = R.linear(h, self.layer(i, "self_attn.q_proj")).view(q_len, self.H, self.D)
            k = R.linear(h, self.layer(i, "self_attn.k_proj")).view(q_len, self.H, self.D)
            v = R.linear(h, self.layer(i, "self_attn.v_proj")).view(q_len, self.H, self.D)
            q = R.apply_rope(self.qk(q, i, "q_norm"), self.cos, self.sin, pos)
            k = R.apply_rope(self.qk(k, i, "k_norm"), self.cos, self.sin, pos)
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
            a = R.linear(a.reshape(q_len, self.H * self.D), self.layer(i, "self_attn.o_proj"))
            x = res + a
            res = x
            h = R.rms_norm(x, self.layer(i, "post_attention_layernorm"), self.eps)
            m = R.silu_mul(R.linear(h, self.layer(i, "mlp.gate_proj")), R.linear(h, self.layer(i, "mlp.up_proj")))
            x = res + R.linear(m, self.layer(i, "mlp.down_proj"))
        x = R.rms_norm(x, self.sd["model.norm.weight"], self.eps)
        return R.linear(x, self.sd["lm_head.weight"]).float().unsqueeze(0)


def forward_fp64(cfg, sd, ids):
    """The truth of the logit checks: the model of (config, state dict) — multi-head or grouped-query, with the q / k norms
    where the state dict has them — evaluated in float64 on the stored fp16 weights and RoPE tables, with NO intermediate
    rounding; ``ids`` (T,) are fed as one causal block.  -> (T, V) float64 logits."""
    H, Hkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    D, eps, T = R.head_dim_of(cfg), cfg["rms_norm_eps"], ids.numel()
    cos, sin = (t.double() for t in R.rope_tables_for(cfg))
    scale = float(R.softmax_scale_for(D))
    pos = torch.arange(T)

    def w(name):
        return sd[name].double()

    def lin(x, i, name):
        return x @ w(f"model.layers.{i}.{name}.weight").t()

    def norm(x, weight):
        return weight.double() * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))

    def head_norm(x, i, name):                                       # (T, heads, D): over the head width, one weight
        wt = sd.get(f"model.layers.{i}.self_attn.{name}.weight")
        return x if wt is None else norm(x, wt)

    def rope(x):
        c, s = cos[pos][:, None, :], sin[pos][:, None, :]
        rot = torch.cat([-x[..., D // 2:], x[..., :D // 2]], dim=-1)
        return x * c + rot * s

    x = w("model.embed_tokens.weight")[ids.reshape(-1)]
    mask = torch.full((T, T), float("-inf"), dtype=torch.float64).triu(1)
    for i in range(cfg["num_hidden_layers"]):
        h = norm(x, sd[f"model.layers.{i}.input_layernorm.weight"])
        q = rope(head_norm(lin(h, i, "self_attn.q_proj").view(T, H, D), i, "q_norm"))
        k = rope(head_norm(lin(h, i, "self_attn.k_proj").view(T, Hkv, D), i, "k_norm")).repeat_interleave(H // Hkv, dim=1)
        v = lin(h, i, "self_attn.v_proj").view(T, Hkv, D).repeat_interleave(H // Hkv, dim=1)
        s = torch.einsum("qhd,khd->hqk", q, k) * scale + mask
        a = torch.einsum("hqk,khd->qhd", torch.softmax(s, dim=-1), v).reshape(T, H * D)
        x = x + lin(a, i, "self_attn.o_proj")
        h = norm(x, sd[f"model.layers.{i}.post_attention_layernorm.weight"])
        g = lin(h, i, "mlp.gate_proj")
        x = x + lin(g / (1.0 + torch.exp(-g)) * lin(h, i, "mlp.up_proj"), i, "mlp.down_proj")
    return norm(x, sd["model.norm.weight"]) @ w("lm_head.weight").t()


# ---- golden-style cases on the zoo's shapes ------------------------------------------------------------------------------------
def specs_config(z, vocab, max_pos=4096):
    from oracle import specs
    cfg = specs.llama_config(z["hidden_size"], z["intermediate_size"], z["num_hidden_layers"], z["num_attention_heads"],
                             vocab_size=vocab, max_position_embeddings=max_pos, rope_theta=z.get("rope_theta", 10000.0),
                             rope_scaling=z.get("rope_scaling"), rms_norm_eps=z["rms_norm_eps"], name=z["_name_or_path"])
    cfg.update(num_key_value_heads=z.get("num_key_value_heads", z["num_attention_heads"]), qk_norm=True,
               model_type=z.get("model_type", "llama"))
    return cfg


def zoo_case(name, **over):
    """A golden-style case dict for the zoo's "tiny-qknorm" / "tiny-gqa-qknorm" target shape at small_gamma6's vocabulary and
    draft: tcfg = the PRODUCT's config, ecfg = the multi-head config the oracle runs."""
    from tests import helpers as Hh
    from triforce_amd.models import zoo
    g = dict(Hh.load_golden("small_gamma6"))
    tcfg = specs_config(dict(zoo.CONFIGS[name]), g["dcfg"]["vocab_size"])
    g.update(dict(dict(name=name, tcfg=tcfg, ecfg=dict(tcfg, num_key_value_heads=tcfg["num_attention_heads"]), tseed=3011,
                       nseed=3012, prefill=512, gen_len=24, budget=128), **over))
    return g


def state_dicts_of(tcfg, tseed, nseed, head_std=0.05):
    """(product state dict, expanded multi-head state dict) for a (possibly grouped-query) QK-norm config: the seeded
    multi-head draw with k_proj / v_proj cut to the first Hkv heads, norm weights from ``add_norms``."""
    from oracle import specs
    H, Hkv = tcfg["num_attention_heads"], tcfg["num_key_value_heads"]
    D = tcfg["hidden_size"] // H
    sd = specs.random_state_dict(dict(tcfg, num_key_value_heads=H), tseed, head_std=head_std)
    for name in list(sd):
        if "k_proj" in name or "v_proj" in name:
            sd[name] = sd[name][:Hkv * D].contiguous()
    sd = add_norms(tcfg, sd, nseed)
    return sd, expand_gqa(tcfg, sd)[1]


def zoo_state_dicts(g):
    """(product state dict, expanded state dict for the oracle, draft state dict) of a ``zoo_case``."""
    from oracle import specs
    sd, esd = state_dicts_of(g["tcfg"], g["tseed"], g["nseed"], g["head_std"])
    return sd, esd, specs.random_state_dict(g["dcfg"], g["dseed"], head_std=g["head_std"])


def build_oracle(g, tsd, dsd):
    """The oracle engine of a golden-style case dict ``g`` around a QkNormOracleTarget.  ``tsd`` must be multi-head
    (``expand_gqa`` first for a grouped-query model), with ``g["ecfg"]`` (else ``g["tcfg"]``) its config."""
    recent = 256 - 16 - g["gamma"]
    cfg = g.get("ecfg", g["tcfg"])
    ot, od = QkNormOracleTarget(cfg, tsd), M.OracleDraft(g["dcfg"], dsd)
    okv = M.FullCache(cfg, g["prefill"] + g["gen_len"] + 16)
    ogc = M.RetrievalCacheO(cfg, g["budget"], g["prefill"], g["chunk"], g["gamma"])
    odc = M.StreamingCacheO(g["dcfg"], gamma=g["gamma"], start_size=16, recent_size=recent)
    return M.OracleEngine(ot, okv, ogc, od, odc, g["temperature"], g["top_p"])


def teacher_forced_gaps(eng, prompt, stream):
    """tests/helpers.teacher_forced_gaps on a given oracle engine: for every token of ``stream`` how far its oracle logit is
    below the oracle's best given the same prefix."""
    eng.kv_cache.reset()
    logits = eng.inference(prompt)[0, -1]
    gaps = [float(logits.max() - logits[stream[0]])]
    for i in range(len(stream) - 1):
        logits = eng.model.forward(torch.tensor([[stream[i]]]), eng.kv_cache, None)[0, -1]
        gaps.append(float(logits.max() - logits[stream[i + 1]]))
    return gaps
