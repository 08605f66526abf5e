"""Target model (Llama-2-7B/13B-128K, LWM-Text-Chat-128K) on the HIP ops — host-side mirror of
the reference's models/modeling_llama.py: same call signature
``model(input_ids=, kv_cache=, graph_cache=, position_ids=, spec=).logits`` (:384-414), same
dispatch between full-cache forward, retrieval-cache (spec) forward and the q_len==1 retrieval
build (:226-238), same numerics.

A decode-sized forward (<= 32 rows) is 6 launches per layer, all hand-written: qkv GEMM (RMSNorm prologue,
RoPE + KV-append epilogue), split-KV MFMA attention + merge, o GEMM (+residual), gate|up GEMM (RMSNorm prologue,
SwiGLU epilogue), down GEMM (+residual).  Prefill chunks (128 rows) run hipBLASLt GEMMs with the stand-alone
RMSNorm / RoPE-append / SwiGLU kernels and the 128-row block attention.
"""
import torch

from .. import ops
from .cache import RetrievalCache
from .config_yarn import LlamaConfig
from .llama_core import (CausalLMOutput, DecoderLayers, LlamaWeights, load_checkpoint_state_dict, parse_random_spec,
                         retrieval_weights, rope_tables_for, softmax_scale_for)


def _check_gqa_env():
    """A grouped-query target runs the fp16 tiers and the one-launch prefill attention only: refuse the rest at construction."""
    from .cache import kv_cache_dtype, retrieval_kv_dtype, KV_CACHE_ENV, RETRIEVAL_KV_ENV
    from .llama_core import RETRIEVAL_WEIGHTS_ENV
    for env, value in ((KV_CACHE_ENV, kv_cache_dtype()), (RETRIEVAL_KV_ENV, retrieval_kv_dtype()),
                       (RETRIEVAL_WEIGHTS_ENV, retrieval_weights())):
        if value == "fp8":
            raise ValueError(f"GQA is not supported with {env}=fp8: the FP8 tiers have no grouped-query kernels")
    if not ops.ATTN_PREFILL_ONE_LAUNCH:
        raise ValueError("GQA is not supported with TRIFORCE_PREFILL_ONE_LAUNCH=0: the per-block prefill kernel "
                         "(tf_attn_block) has one head count")


class LlamaForCausalLM:
    def __init__(self, config: LlamaConfig, device="cuda:0"):
        self.config = config
        self.device = torch.device(device)
        self.dtype = torch.float16
        self.gqa = config.num_key_value_heads != config.num_attention_heads     # grouped-query target
        if self.gqa:
            _check_gqa_env()
        if getattr(config, "attention_bias", False) and retrieval_weights() == "fp8":
            # attention bias runs the fp16 weights; the FP8 KV tiers only consume what the GEMMs produce
            from .llama_core import RETRIEVAL_WEIGHTS_ENV
            raise ValueError(f"attention bias is not supported with {RETRIEVAL_WEIGHTS_ENV}=fp8: the FP8 weight kernels "
                             "(Fp8Linear) have no bias epilogue")
        if getattr(config, "qk_norm", False) and retrieval_weights() == "fp8":
            # QK norm: the per-head norm sits between the q|k|v GEMM and the rotation the FP8 kernel fuses
            from .llama_core import RETRIEVAL_WEIGHTS_ENV
            raise ValueError(f"QK norm is not supported with {RETRIEVAL_WEIGHTS_ENV}=fp8: no FP8 q|k|v weight (Fp8Linear) "
                             "feeds the per-head norm")
        self.weights = LlamaWeights(config, self.device)
        # TRIFORCE_RETRIEVAL_WEIGHTS=fp8: the retrieval-cache (spec) forward streams FP8 copies of its five GEMM weights
        # (DESIGN section 16); every other forward keeps the fp16 weights
        self.weights.retrieval_fp8 = retrieval_weights() == "fp8"
        cos, sin = rope_tables_for(config)
        self.cos, self.sin = cos.to(self.device), sin.to(self.device)
        self.scale = softmax_scale_for(config.hidden_size // config.num_attention_heads)
        self.layers = DecoderLayers(self.weights, self.cos, self.sin)
        self.vocab_size = config.vocab_size

    # -- construction ------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, name_or_path, torch_dtype=torch.float16, device_map="cuda:0", config=None, **_):
        """Local HF directory, or ``random:<seed>`` with an explicit ``config`` (no hub access offline)."""
        assert torch_dtype == torch.float16, "the TriForce path is fp16"
        seed = parse_random_spec(name_or_path)
        if seed is not None:
            assert config is not None, "random:<seed> needs config="
            return cls(config, device_map).init_random(seed)
        from .aligned import parse_spec
        spec = parse_spec(name_or_path)
        if spec is not None:                                # aligned[:draft_acc[:retrieval_acc[:seed]]]
            assert config is not None, "aligned:... needs config="
            return cls(config, device_map).init_aligned(spec, attn_keys=_.get("attn_keys", 4096))
        cfg = config or LlamaConfig.from_pretrained(name_or_path)
        m = cls(cfg, device_map)
        m.weights.load_state_dict(load_checkpoint_state_dict(name_or_path))
        return m

    @classmethod
    def from_state_dict(cls, config, sd, device="cuda:0"):
        m = cls(config, device)
        m.weights.load_state_dict(sd)
        return m

    def init_random(self, seed):
        self.weights.init_random(seed)
        return self

    def init_aligned(self, spec, attn_keys=4096):
        """Aligned synthetic weights (models/aligned.py), this model in the target role."""
        self.weights.init_aligned(spec, "target", attn_keys=attn_keys)
        return self

    def eval(self):
        return self

    # -- forward -----------------------------------------------------------------------------
    @torch.inference_mode()
    def __call__(self, input_ids, kv_cache=None, graph_cache=None, position_ids=None, spec=False,
                 attention_mask=None, storage_ids=None, gamma_offset=0, rebuild_retrieval=False, dev_len=None):
        return self.forward(input_ids, kv_cache, graph_cache, position_ids, spec, rebuild_retrieval, dev_len)

    def forward(self, input_ids, kv_cache, graph_cache=None, position_ids=None, spec=False, rebuild_retrieval=False,
                dev_len=None, last_rows=None, next_ids=None, logprobs_out=None):
        """last_rows = k: logits of the trailing k rows only (chunked prefill: utils/graph_infer.py chunked_prefill).
        next_ids (q_len,) int64 + logprobs_out (q_len,) fp32 device tensors: logprobs_out[i] receives the log-probability
        (temperature 1, unfiltered) of next_ids[i] under row i — the prompt's log-probabilities; the
        logits returned are unchanged.
        dev_len = (slot_dev, sk_dev) int32 device scalars: the hipGraph-capturable form of the full-cache decode
        forward — the append slot and the key count are read from device memory by the kernels (tf_skinny_qkv_rope
        slot0_dev, tf_attn_decode sk_dev), position_ids must be given, the launch is sized by the cache capacity and
        kv_cache.seq_len is NOT advanced (the caller does that after the replay)."""
        W, layers = self.weights, self.layers
        q_len = input_ids.shape[1]
        if dev_len is not None:
            assert position_ids is not None and not spec and q_len <= ops.SKINNY_MAX_ROWS
        if position_ids is None:                        # reference modeling_llama.py:345-349
            position_ids = torch.arange(kv_cache.seq_len, kv_cache.seq_len + q_len, dtype=torch.long,
                                        device=self.device).unsqueeze(0)
        pos = position_ids.reshape(-1).contiguous()
        eager_full = (not spec) and dev_len is None
        build = eager_full and q_len == 1 and isinstance(graph_cache, RetrievalCache)
        # periodic rebuild (described in the reference's blog, absent from its code): during a
        # target verify, re-select the prefill chunks with the query of the first — already confirmed — token
        rebuild = eager_full and q_len > 1 and rebuild_retrieval and isinstance(graph_cache, RetrievalCache)
        streaming = (not spec) and hasattr(kv_cache, "begin_forward")     # host-offloaded KV (test/offloading.py)
        if streaming:
            kv_cache.begin_forward()
        # decode-sized blocks run the fused kernels: [norm ->] qkv GEMM -> RoPE -> KV append in one launch, the
        # residual adds in the o / down GEMM epilogues, the post-attention norm in the gate|up GEMM prologue
        fused = (ops.FUSE_MODE == "all" and ops.can_fuse_rows(q_len, W.embed, W.wqkv[0], W.wo[0], W.wgu[0], W.wd[0], W.lm_head)
                 and (W.qk_norm or W.wqkv[0].wp_rope is not None))
        # the retrieval-verify tier: a spec forward with FP8 weights (ops.Fp8Linear) in its five GEMMs
        f8 = spec and W.fp8_active()
        if f8 and not fused:
            raise RuntimeError(f"the FP8 retrieval tier needs the fused decode layer ({q_len} rows)")
        assert fused or dev_len is None, "the captured full-cache forward needs the fused decode kernels"
        # FP8 retrieval cache (TRIFORCE_RETRIEVAL_KV=fp8): the spec forward's attention reads codes, then the
        # fp16 rows this forward appends, in one launch
        rkv8 = spec and graph_cache.fp8
        if rkv8 and not fused:
            raise RuntimeError(f"the FP8 retrieval cache needs the fused decode layer ({q_len} rows)")
        # the fused layer keeps residual stream / attention output / SwiGLU output k-octet-major (ops.Act): the GEMMs' B
        # operand is then read in 256-byte runs (ops.py, "activation layouts")
        packed = fused and ops.act_packed(q_len)
        x = ops.embed_rows(W.embed, input_ids, packed)   # (q, hidden) fp16 gather
        ss = ops.ss_buffer(x.shape[1], x.device) if fused else None     # sum(x^2) hand-off between GEMMs
        slot_dev, sk_dev = dev_len if dev_len is not None else (None, None)
        d = None
        for i in range(W.L):
            kl, vl, slot, sk, codes = self._kv_view(i, q_len, fused, kv_cache, graph_cache if spec else None, dev_len)
            # FP8 KV cache (codes): the fresh rows are quantized before the attention that reads them
            if fused and codes:                         # q|k|v+RoPE into staging rows [0, q_len), from there into the cache
                q = layers.qkv_fused(i, x, ss, pos, kl, vl, 0)
                ops.kv_quant_rows(kl[:, :q_len], vl[:, :q_len], *codes, slot, slot0_dev=slot_dev)
            elif fused:
                q = layers.qkv_fused(i, x, ss, pos, kl, vl, slot, slot_dev, f8)
            else:                                       # RoPE-append into the dequantized scratch, deq values written back
                q = layers.qkv(i, x, d, pos, kl, vl, slot)
                if codes:
                    ops.kv_quant_rows(kl[:, slot:slot + q_len], vl[:, slot:slot + q_len], *codes, slot, deq=True)
            if build and not graph_cache.init_graph:
                graph_cache.init_graph_cache(kv_cache, q, i)
            elif build:
                graph_cache.update_graph_cache_retrieval(kv_cache, q, i)
            elif rebuild:                               # generated tail is re-copied by update_graph_cache() after accept
                graph_cache.init_graph_cache(kv_cache, q[:1], i)
            if codes and not fused and (build or rebuild):      # the build used the scratch: rows [0, sk) again
                kl, vl = kv_cache.scratch_layer(i, sk)
            if rkv8:
                a = ops.attn_decode_fp8_tail(q, *graph_cache.layer_codes(i), kl, vl, graph_cache.max_budget, self.scale,
                                             packed=packed)
            else:
                a = self._attention(q, kl, vl, sk, codes if fused else None, sk_dev, packed, spec or dev_len is not None)
            if streaming and dev_len is None:
                kv_cache.layer_done(i, slot, q_len)
            if fused:
                layers.o_fused(i, a, x, ss, f8)                                                 # x += attn_out
                layers.down_fused(i, layers.gate_up_fused(i, x, ss, f8), x, ss, f8)              # x += mlp_out
            else:
                d = layers.mlp(i, x, layers.o_proj(i, a))
        if streaming:
            kv_cache.end_forward()
        if next_ids is None:
            return CausalLMOutput(layers.head_fused(x, ss, f8) if fused else layers.head(x, d, last_rows))
        score = dict(next_ids=next_ids.reshape(-1), logprobs_out=logprobs_out)
        return CausalLMOutput(layers.head_fused(x, ss, f8, **score) if fused else layers.head(x, d, last_rows, **score))

    @staticmethod
    def _kv_view(i, q_len, fused, kv_cache, spec_cache, dev_len):
        """Layer i's (K view, V view, append slot, key count, FP8 codes | None): where the fresh rows go and what the
        attention reads.  With an FP8 KV cache (TRIFORCE_KV_CACHE=fp8) the views are fp16 work space,
        not the cache: the 32-row staging for a decode-sized (fused) block, else the layer scratch holding the dequantized
        rows [0, slot).  A captured forward (dev_len) appends at a slot the device holds and is sized by the capacity."""
        if spec_cache is not None:                      # :226-227  retrieval-cache forward
            assert q_len == spec_cache.gamma + 1, "spec forward takes exactly gamma+1 tokens (cache.py:184-189)"
            if spec_cache.fp8:                          # FP8 retrieval cache: the views are its fp16 spec rows alone
                return (*spec_cache.layer_kv(i), 0, spec_cache.real_budget, None)
            return (*spec_cache.layer_kv(i), spec_cache.spec_slot, spec_cache.real_budget, None)
        if dev_len is not None:                         # captured full-cache forward: lengths live on the device
            slot, sk = 0, kv_cache.max_budget
        else:                                           # :228-238  full-cache forward
            slot = kv_cache.append_slot(i, q_len)
            sk = slot + q_len
        if not kv_cache.fp8:
            return (*kv_cache.layer_kv(i), slot, sk, None)
        kl, vl = (kv_cache.stage_k, kv_cache.stage_v) if fused else kv_cache.scratch_layer(i, slot)
        return kl, vl, slot, sk, kv_cache.layer_codes(i)

    def _attention(self, q, kl, vl, sk, codes, sk_dev, packed, decode):
        """``codes``: the FP8 cache's own kernel (decode-sized blocks only).  ``decode``: the retrieval-cache forward and the
        captured forward, split-KV decode kernel whatever the layout; an eager full-cache block takes it only with k-octet-major
        rows and is a prefill block otherwise.  A grouped-query target (q has more heads than the cache views) takes the GQA
        kernels through the same two calls: ops.attn_decode / ops.attn_prefill dispatch on the head counts."""
        if codes:
            return ops.attn_decode_fp8(q, *codes, sk, self.scale, sk_dev=sk_dev, packed=packed)
        if decode or packed:
            return ops.attn_decode(q, kl, vl, sk, self.scale, sk_dev=sk_dev, packed=packed)
        return ops.attn_prefill(q, kl, vl, sk, self.scale)
