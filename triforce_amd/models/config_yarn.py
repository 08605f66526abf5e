"""Llama config schema for the TriForce path (role of models/config_yarn.py:31-193 in the reference).

A plain attribute bag that reads the HF ``config.json`` keys the path consumes
(modeling_llama.py:166-198): no transformers dependency.
"""
import json
import os

_DEFAULTS = dict(
    vocab_size=32000, hidden_size=4096, intermediate_size=11008, num_hidden_layers=32,
    num_attention_heads=32, num_key_value_heads=None, hidden_act="silu", max_position_embeddings=2048,
    rms_norm_eps=1e-6, rope_theta=10000.0, rope_scaling=None, attention_bias=False, pad_token_id=None,
    bos_token_id=1, eos_token_id=2, _name_or_path="",
    # attention bias: kept to tell a Qwen2-family config (model_type "qwen2": q/k/v bias implied) from a
    # Llama one, and to refuse what the path does not compute
    model_type="llama", mlp_bias=False, use_sliding_window=False,
)
GQA_HEAD_DIMS = (64, 128)        # head widths of the grouped-query kernels (tf_attn_decode_gqa_act, tf_attn_prefill_gqa)


def refuse_attention_bias(cfg, what):
    """ValueError for a config with attention bias in a component whose projections are bias-free."""
    if getattr(cfg, "attention_bias", False):
        raise ValueError(f"attention bias (attention_bias=True) is not supported by {what}: q/k/v/o biases run on the "
                         "single-GPU resident engine with fp16 weights only")


def refuse_qk_norm(cfg, what):
    """ValueError for a QK-norm config in a component that has no per-head q/k RMSNorm."""
    if getattr(cfg, "qk_norm", False):
        raise ValueError(f"QK norm (qk_norm=True) is not supported by {what}: the per-head q/k RMSNorm runs on the single-GPU "
                         "resident engine with fp16 weights only")


def _read_rope_parameters(d):
    """``rope_parameters`` (how transformers 5.x writes theta and scaling: ``{"rope_type": ..., "rope_theta": ..., ...}``) ->
    the ``rope_theta`` / ``rope_scaling`` keys this config consumes.  A top-level key that is also present must agree; a form
    that is not understood (per-layer-type dicts) is refused: ignoring it would load another model without an error."""
    rp = d.pop("rope_parameters", None)
    if rp is None:
        return
    if not isinstance(rp, dict) or any(isinstance(v, dict) for v in rp.values()):
        raise ValueError(f"`rope_parameters` must be one flat dict (rope_type, rope_theta, scaling keys), got {rp}")
    rp = dict(rp)
    theta = rp.pop("rope_theta", None)
    if theta is not None:
        if "rope_theta" in d and float(d["rope_theta"]) != float(theta):
            raise ValueError(f"rope_theta ({d['rope_theta']}) and rope_parameters.rope_theta ({theta}) disagree")
        d["rope_theta"] = theta
    kind = rp.get("rope_type", rp.get("type", "default"))
    if kind != "default":
        if d.get("rope_scaling") is not None:
            raise ValueError("both `rope_scaling` and a scaled `rope_parameters` are given")
        d["rope_scaling"] = rp


def refuse_gqa(cfg, what):
    """ValueError for a grouped-query config in a component that has one head count only."""
    if cfg.num_key_value_heads != cfg.num_attention_heads:
        raise ValueError(f"GQA ({cfg.num_attention_heads} query / {cfg.num_key_value_heads} KV heads) is not supported by "
                         f"{what}: grouped-query attention runs on the single-GPU resident engine with fp16 tiers only")


class LlamaConfig:
    def __init__(self, **kw):
        for k, v in _DEFAULTS.items():
            setattr(self, k, kw.pop(k, v))
        # QK norm: per-head RMSNorm of q and k in front of the rotation (the Qwen3 family).  A plain
        # attribute, not a _DEFAULTS key: to_dict() keeps the key set it had, and carries qk_norm only when it is set
        self.qk_norm = bool(kw.pop("qk_norm", False))
        for k, v in kw.items():
            setattr(self, k, v)
        if self.num_key_value_heads is None:
            self.num_key_value_heads = self.num_attention_heads
        self._validate()

    def _validate(self):
        # role of config_yarn.py:170-193 (_rope_scaling_validation), reduced to what the path supports
        if self.hidden_act != "silu":
            raise ValueError(f"hidden_act {self.hidden_act!r} is not supported (silu only)")
        # attention_bias: q/k/v/o projections with a bias (reference models/modeling_llama.py:174-177) — accepted; the MLP
        # stays bias-free and attention stays global
        self.attention_bias = bool(self.attention_bias)
        if self.mlp_bias:
            raise ValueError("mlp_bias=True is not supported (the MLP projections are bias-free)")
        if self.use_sliding_window:
            raise ValueError("use_sliding_window=True is not supported (attention is global)")
        if self.qk_norm and self.attention_bias:
            raise ValueError("qk_norm=True together with attention_bias=True is not supported: no checkpoint of that form "
                             "exists to check the combination against")
        if self.qk_norm and self.hidden_size // self.num_attention_heads not in GQA_HEAD_DIMS:
            raise ValueError(f"qk_norm=True needs head_dim in {GQA_HEAD_DIMS} (tf_qk_norm_rope_append), got "
                             f"{self.hidden_size // self.num_attention_heads}")
        H, Hkv = self.num_attention_heads, self.num_key_value_heads
        if not isinstance(Hkv, int) or Hkv < 1 or H % Hkv:
            raise ValueError(f"GQA: num_attention_heads ({H}) must be a multiple of num_key_value_heads ({Hkv})")
        if Hkv != H and self.hidden_size // H not in GQA_HEAD_DIMS:
            # grouped-query attention (the reference's retrieval cache is MHA-only):
            # the GQA kernels are built for these head widths
            raise ValueError(f"GQA ({H} query / {Hkv} KV heads) needs head_dim in {GQA_HEAD_DIMS}, got "
                             f"{self.hidden_size // H}")
        rs = self.rope_scaling
        if isinstance(rs, dict) and "type" not in rs and "rope_type" in rs:
            rs = self.rope_scaling = dict(rs, type=rs["rope_type"])      # the spelling of Qwen3 cards / transformers 5.x
        if rs is not None:
            if not isinstance(rs, dict) or "type" not in rs or "factor" not in rs:
                raise ValueError(f"`rope_scaling` must be a dict with `type` and `factor`, got {rs}")
            if rs["type"] != "yarn":
                raise ValueError(f"Unknown RoPE scaling type {rs['type']}")
            if float(rs["factor"]) <= 1.0:
                raise ValueError(f"`rope_scaling`'s factor must be > 1, got {rs['factor']}")
            if "original_max_position_embeddings" not in rs:
                raise ValueError("yarn rope_scaling needs original_max_position_embeddings")

    @property
    def head_dim(self):
        return self.hidden_size // self.num_attention_heads

    @property
    def kv_groups(self):
        """Query heads per KV head (1: multi-head attention)."""
        return self.num_attention_heads // self.num_key_value_heads

    @classmethod
    def from_dict(cls, d):
        return cls(**dict(d))

    @classmethod
    def from_pretrained(cls, path):
        with open(os.path.join(path, "config.json")) as f:
            d = json.load(f)
        head_dim = d.get("head_dim")
        d = {k: v for k, v in d.items() if k in _DEFAULTS or k == "qk_norm" or k.startswith("rope")}
        _read_rope_parameters(d)
        if d.get("model_type") == "qwen2" and "attention_bias" not in d:
            d["attention_bias"] = True                   # Qwen2 / Qwen2.5: bias on q/k/v (none on o_proj), no config key
        if d.get("model_type") == "qwen3" and "qk_norm" not in d:
            d["qk_norm"] = True                          # Qwen3: q_norm / k_norm on every attention layer, no config key
        if head_dim is not None:
            hid, H = d.get("hidden_size", _DEFAULTS["hidden_size"]), d.get("num_attention_heads", _DEFAULTS["num_attention_heads"])
            if head_dim != hid // H:
                raise ValueError(f"head_dim ({head_dim}) differs from hidden_size // num_attention_heads ({hid} // {H} = "
                                 f"{hid // H}): a head width decoupled from the hidden size is not supported")
        d["_name_or_path"] = path
        return cls(**d)

    def to_dict(self):
        d = {k: getattr(self, k) for k in _DEFAULTS}
        if self.qk_norm:
            d["qk_norm"] = True
        return d
