"""Shapes of the models the TriForce entry points name (the reference hard-codes hub ids:
test/on_chip.py:48-56, test/offloading_TP.py:56-67); offline they are built from these configs with
random-init weights, or loaded from a local HF directory.  Values are the public model cards'."""
from .config_yarn import LlamaConfig

_YARN_128K = dict(type="yarn", factor=32.0, original_max_position_embeddings=4096)

CONFIGS = {
    # NousResearch/Yarn-Llama-2-7b-128k
    "llama-7B-128K": dict(hidden_size=4096, intermediate_size=11008, num_hidden_layers=32, num_attention_heads=32,
                          max_position_embeddings=131072, rms_norm_eps=1e-5, rope_scaling=_YARN_128K,
                          _name_or_path="NousResearch/Yarn-Llama-2-7b-128k"),
    # NousResearch/Yarn-Llama-2-13b-128k
    "llama-13B-128K": dict(hidden_size=5120, intermediate_size=13824, num_hidden_layers=40, num_attention_heads=40,
                           max_position_embeddings=131072, rms_norm_eps=1e-5, rope_scaling=_YARN_128K,
                           _name_or_path="NousResearch/Yarn-Llama-2-13b-128k"),
    # LargeWorldModel/LWM-Text-Chat-128K: Llama-2-7B with plain RoPE, theta 1e7
    "lwm-128K": dict(hidden_size=4096, intermediate_size=11008, num_hidden_layers=32, num_attention_heads=32,
                     max_position_embeddings=131072, rms_norm_eps=1e-5, rope_theta=1e7,
                     _name_or_path="LargeWorldModel/LWM-Text-Chat-128K"),
    "lwm-128K-base": dict(hidden_size=4096, intermediate_size=11008, num_hidden_layers=32, num_attention_heads=32,
                          max_position_embeddings=131072, rms_norm_eps=1e-5, rope_theta=1e7,
                          _name_or_path="LargeWorldModel/LWM-Text-128K"),
    # JackFram/llama-68m
    "llama-68M": dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=2, num_attention_heads=12,
                      max_position_embeddings=2048, rms_norm_eps=1e-6, _name_or_path="JackFram/llama-68m"),
    # 2-layer D=128 YaRN toy used by BASELINE configs[0] ("tiny target") and the smoke paths
    "tiny": dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2,
                 max_position_embeddings=131072, rms_norm_eps=1e-6,
                 rope_scaling=dict(type="yarn", factor=16.0, original_max_position_embeddings=256),
                 _name_or_path="tiny-yarn-target"),
    # the tiny target with grouped-query attention: 4 query heads over 2 KV heads, D = 128
    "tiny-gqa": dict(hidden_size=512, intermediate_size=768, num_hidden_layers=2, num_attention_heads=4,
                     num_key_value_heads=2, max_position_embeddings=131072, rms_norm_eps=1e-6,
                     rope_scaling=dict(type="yarn", factor=16.0, original_max_position_embeddings=256),
                     _name_or_path="tiny-yarn-gqa-target"),
    # the tiny targets with attention bias: "tiny" with q/k/v/o biases (the Llama-architecture form),
    # "tiny-gqa" with q/k/v biases only (the Qwen2 form: model_type qwen2, no o_proj bias)
    "tiny-bias": dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2,
                      max_position_embeddings=131072, rms_norm_eps=1e-6, attention_bias=True,
                      rope_scaling=dict(type="yarn", factor=16.0, original_max_position_embeddings=256),
                      _name_or_path="tiny-yarn-bias-target"),
    "tiny-gqa-bias": dict(hidden_size=512, intermediate_size=768, num_hidden_layers=2, num_attention_heads=4,
                          num_key_value_heads=2, max_position_embeddings=131072, rms_norm_eps=1e-6, attention_bias=True,
                          model_type="qwen2",
                          rope_scaling=dict(type="yarn", factor=16.0, original_max_position_embeddings=256),
                          _name_or_path="tiny-yarn-gqa-bias-target"),
    # Qwen/Qwen2.5-7B-Instruct-1M shape (grouped-query 28 / 4 heads, q/k/v bias, plain RoPE with theta 1e7).  Written from
    # memory of the model card: there is no hub access offline, so these values are NOT checked against the published
    # config.json.  With g = 7 the decode attention stacks gs = 1 query head at 7 rows (ops.gqa_stack): K / V is read per
    # query head (known limit)
    "qwen2.5-7B-1M": dict(vocab_size=152064, hidden_size=3584, intermediate_size=18944, num_hidden_layers=28,
                          num_attention_heads=28, num_key_value_heads=4, max_position_embeddings=1010000, rms_norm_eps=1e-6,
                          rope_theta=1e7, attention_bias=True, model_type="qwen2", bos_token_id=151643, eos_token_id=151645,
                          _name_or_path="Qwen/Qwen2.5-7B-Instruct-1M"),
    # the tiny targets with QK norm: per-head RMSNorm of q and k before the rotation.  "tiny" with plain RoPE
    # at theta 1e6, "tiny-gqa" as a Qwen3-form config (model_type qwen3 implies the norms when a config.json is read; here
    # the key is spelled out)
    "tiny-qknorm": dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2,
                        max_position_embeddings=131072, rms_norm_eps=1e-6, rope_theta=1e6, qk_norm=True,
                        _name_or_path="tiny-qknorm-target"),
    "tiny-gqa-qknorm": dict(hidden_size=512, intermediate_size=768, num_hidden_layers=2, num_attention_heads=4,
                            num_key_value_heads=2, max_position_embeddings=131072, rms_norm_eps=1e-6, rope_theta=1e6,
                            qk_norm=True, model_type="qwen3", _name_or_path="tiny-gqa-qknorm-target"),
    # Qwen/Qwen3-8B shape (grouped-query 32 / 8 heads, head_dim 128 = hidden / heads, q_norm / k_norm, plain RoPE with theta
    # 1e6).  Written from memory of the model card: there is no hub access offline, so these values are NOT checked against
    # the published config.json
    "qwen3-8B": dict(vocab_size=151936, hidden_size=4096, intermediate_size=12288, num_hidden_layers=36,
                     num_attention_heads=32, num_key_value_heads=8, max_position_embeddings=40960, rms_norm_eps=1e-6,
                     rope_theta=1e6, qk_norm=True, model_type="qwen3", bos_token_id=151643, eos_token_id=151645,
                     _name_or_path="Qwen/Qwen3-8B"),
    # the tiny target and the 68M-shaped draft with the Llama-3 vocabulary (128 256 entries).  No trained
    # draft of that vocabulary exists offline: both are random-init shapes
    "tiny-v128k": dict(vocab_size=128256, hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2,
                       max_position_embeddings=131072, rms_norm_eps=1e-6,
                       rope_scaling=dict(type="yarn", factor=16.0, original_max_position_embeddings=256),
                       _name_or_path="tiny-yarn-target-v128k"),
    "llama-68M-v128k": dict(vocab_size=128256, hidden_size=768, intermediate_size=3072, num_hidden_layers=2,
                            num_attention_heads=12, max_position_embeddings=2048, rms_norm_eps=1e-6,
                            _name_or_path="llama-68m-shape-v128k"),
    # NousResearch/Yarn-Llama-2-70b-32k (grouped-query, 64 / 8 heads).  Written from memory of the model card: there is
    # no hub access offline, so these values are NOT checked against the published config.json
    "llama-70B-32K": dict(hidden_size=8192, intermediate_size=28672, num_hidden_layers=80, num_attention_heads=64,
                          num_key_value_heads=8, max_position_embeddings=32768, rms_norm_eps=1e-5,
                          rope_scaling=dict(type="yarn", factor=8.0, original_max_position_embeddings=4096),
                          _name_or_path="NousResearch/Yarn-Llama-2-70b-32k"),
}


def config(name):
    if name not in CONFIGS:
        raise NotImplementedError(f"unknown model {name!r}; known: {sorted(CONFIGS)}")
    return LlamaConfig.from_dict(CONFIGS[name])


def draft_for(target_name):
    """Name of the 68M-shaped draft that shares the named target's vocabulary (the draft proposes token ids of the target)."""
    V = config(target_name).vocab_size
    for name in ("llama-68M", "llama-68M-v128k"):
        if config(name).vocab_size == V:
            return name
    raise NotImplementedError(f"no 68M-shaped draft with the {V}-entry vocabulary of {target_name!r}")


def find_checkpoint(name):
    """Local directory holding the real checkpoint of a named model, or None (there is no hub access offline).
    Looked up, in order: $TRIFORCE_CKPT_DIR/<repo basename>, the HF cache ($HF_HOME/hub, ~/.cache/huggingface/hub:
    models--<org>--<repo>/snapshots/*), /root/models, /models, /data/models."""
    import glob
    import os
    repo = CONFIGS[name]["_name_or_path"]
    base = repo.split("/")[-1]
    cands = []
    if os.environ.get("TRIFORCE_CKPT_DIR"):
        cands += [os.path.join(os.environ["TRIFORCE_CKPT_DIR"], base), os.path.join(os.environ["TRIFORCE_CKPT_DIR"], repo)]
    hubs = [os.path.join(os.environ["HF_HOME"], "hub")] if os.environ.get("HF_HOME") else []
    hubs.append(os.path.expanduser("~/.cache/huggingface/hub"))
    for hub in hubs:
        cands += sorted(glob.glob(os.path.join(hub, "models--" + repo.replace("/", "--"), "snapshots", "*")))
    for root in ("/root/models", "/models", "/data/models"):
        cands += [os.path.join(root, base), os.path.join(root, repo)]
    for c in cands:
        if os.path.isfile(os.path.join(c, "config.json")) and \
                (glob.glob(os.path.join(c, "*.safetensors")) or glob.glob(os.path.join(c, "*.bin"))):
            return c
    return None
