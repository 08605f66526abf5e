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


def refuse_gqa(cfg, what):
    """ValueError for a grouped-query config in a component that has one head count only."""
    if cfg.num_key_value_heads != cfg.num_attention_heads:
        raise ValueError(f"GQA ({cfg.num_attention_heads} query / {cfg.num_key_value_heads} KV heads) is not supported by "
                         f"{what}: grouped-query attention runs on the single-GPU resident engine with fp16 tiers only")


class LlamaConfig:
    def __init__(self, **kw):
        for k, v in _DEFAULTS.items():
            setattr(self, k, kw.pop(k, v))
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
        H, Hkv = self.num_attention_heads, self.num_key_value_heads
        if not isinstance(Hkv, int) or Hkv < 1 or H % Hkv:
            raise ValueError(f"GQA: num_attention_heads ({H}) must be a multiple of num_key_value_heads ({Hkv})")
        if Hkv != H and self.hidden_size // H not in GQA_HEAD_DIMS:
            # grouped-query attention (the reference's retrieval cache is MHA-only):
            # the GQA kernels are built for these head widths
            raise ValueError(f"GQA ({H} query / {Hkv} KV heads) needs head_dim in {GQA_HEAD_DIMS}, got "
                             f"{self.hidden_size // H}")
        rs = self.rope_scaling
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
        d = {k: v for k, v in d.items() if k in _DEFAULTS or k.startswith("rope")}
        if d.get("model_type") == "qwen2" and "attention_bias" not in d:
            d["attention_bias"] = True                   # Qwen2 / Qwen2.5: bias on q/k/v (none on o_proj), no config key
        d["_name_or_path"] = path
        return cls(**d)

    def to_dict(self):
        return {k: getattr(self, k) for k in _DEFAULTS}
