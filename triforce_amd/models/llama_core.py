"""Weights, RoPE tables and the per-layer compute of a Llama decoder on the HIP ops.

Shared by the target model (modeling_llama.py), the 68M draft (modeling_llama_68m.py) and the
tensor-parallel engine (TP_llama.py).  q/k/v and gate/up projection weights are stored fused
(one skinny GEMM each instead of three / two): a decode step is bound by streaming the weights
once, so fewer, larger GEMMs and fused element-wise kernels are what matters on MI355X.
"""
import json
import math
import os
import zlib

import torch

from .. import ops
from .config_yarn import LlamaConfig


# ---- RoPE tables (same arithmetic as the reference, fp32 on the host, stored fp16) ----------
def rope_tables_plain(dim, max_pos, base):
    """reference models/modeling_llama.py:21-41."""
    inv_freq = 1.0 / (base ** (torch.arange(0, dim, 2).float() / dim))
    freqs = torch.outer(torch.arange(max_pos, dtype=inv_freq.dtype), inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().to(torch.float16), emb.sin().to(torch.float16)


def yarn_inv_freq(dim, factor, orig_max_pos, base=10000.0, beta_fast=32, beta_slow=1):
    """(inverse frequencies (dim/2,) fp32, attention factor) of YaRN: reference models/modeling_llama.py:50-107."""
    def corr_dim(n_rot):
        return (dim * math.log(orig_max_pos / (n_rot * 2 * math.pi))) / (2 * math.log(base))

    pos_freqs = base ** (torch.arange(0, dim, 2).float() / dim)
    inv_extrapolation = 1.0 / pos_freqs
    inv_interpolation = 1.0 / (factor * pos_freqs)
    low = float(max(math.floor(corr_dim(beta_fast)), 0))
    high = float(min(math.ceil(corr_dim(beta_slow)), dim - 1))
    if low == high:
        high += 0.001
    ramp = torch.clamp((torch.arange(dim // 2, dtype=torch.float32) - low) / (high - low), 0, 1)
    mask = 1 - ramp
    inv_freq = inv_interpolation * (1 - mask) + inv_extrapolation * mask
    mscale = 1.0 if factor <= 1 else 0.1 * math.log(factor) + 1.0
    return inv_freq, mscale


def rope_tables_yarn(dim, max_pos, factor, orig_max_pos, base=10000.0, beta_fast=32, beta_slow=1):
    """reference models/modeling_llama.py:50-124 (YaRN; base hard-wired to 10000 at :193)."""
    inv_freq, mscale = yarn_inv_freq(dim, factor, orig_max_pos, base, beta_fast, beta_slow)
    freqs = torch.outer(torch.arange(max_pos, dtype=torch.float32), inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1)
    return (emb.cos() * mscale).to(torch.float16), (emb.sin() * mscale).to(torch.float16)


def rope_tables_for(cfg, force_plain=False):
    D = cfg.hidden_size // cfg.num_attention_heads
    rs = cfg.rope_scaling
    if rs is None or force_plain:
        return rope_tables_plain(D, cfg.max_position_embeddings, cfg.rope_theta)
    if getattr(cfg, "qk_norm", False):
        # a QK-norm (Qwen3-family) config: YaRN over the model's own theta.  Llama / Qwen2 configs keep the reference's
        # hard-wired base 10000
        return rope_tables_yarn(D, cfg.max_position_embeddings, rs["factor"], rs["original_max_position_embeddings"],
                                base=float(cfg.rope_theta))
    return rope_tables_yarn(D, cfg.max_position_embeddings, rs["factor"], rs["original_max_position_embeddings"])


def softmax_scale_for(head_dim):
    """fp16(1)/sqrt(fp16(D)) as the reference computes it (modeling_llama.py:240): 0.08837890625 for D=128."""
    return float(1 / torch.sqrt(torch.tensor(head_dim, dtype=torch.float16)))


# ---- retrieval-verify weight tier ----------------------------------------------------------------------
RETRIEVAL_WEIGHTS_ENV = "TRIFORCE_RETRIEVAL_WEIGHTS"
# Standard deviation of the randomly drawn attention biases (init_random of a bias config).  Large against the matrices'
# 0.02 on purpose: trained q/k biases are O(1) and larger, and a bias that moved no logit would make every test of the biased
# path vacuous (tests/test_attn_bias_cpu.py pins that zeroing the biases changes the greedy stream).
BIAS_STD = 0.5
# Standard deviation of the randomly drawn q_norm / k_norm weights around 1 (init_random of a QK-norm config, DESIGN section
# 30): trained ones spread far wider; 0.25 moves the greedy stream of the tiny models well clear of the norm-free one
# (tests/test_qk_norm_cpu.py pins that).
QK_NORM_STD = 0.25


def retrieval_weights():
    """TRIFORCE_RETRIEVAL_WEIGHTS: ``fp16`` (default) or ``fp8`` — the weights the target's retrieval-cache (spec) forward
    streams.  Read when a target model is built; fp8 needs the fused decode layer (TRIFORCE_FUSE=all)."""
    return ops.fp16_or_fp8(RETRIEVAL_WEIGHTS_ENV, None, "the FP8 kernels exist only in that form")


class CausalLMOutput:
    __slots__ = ("logits", "probs")

    def __init__(self, logits, probs=None):
        self.logits = logits
        self.probs = probs


class LlamaWeights:
    """Device-resident fp16 weights with fused qkv / gate-up matrices.

    rank / world_size select a Megatron-style shard (TP_layers.py:126-147): q/k/v/gate/up rows,
    o/down columns; embed, norms and lm_head are replicated (TP_llama.py:91-94).
    """

    def __init__(self, cfg: LlamaConfig, device, rank=0, world_size=1):
        self.cfg, self.device, self.rank, self.world_size = cfg, torch.device(device), rank, world_size
        self.L = cfg.num_hidden_layers
        self.H = cfg.num_attention_heads
        self.D = cfg.hidden_size // self.H
        self.Hkv = cfg.num_key_value_heads                  # < H: grouped-query attention
        if self.Hkv != self.H and world_size > 1:
            raise ValueError(f"GQA ({self.H} query / {self.Hkv} KV heads) is not supported by tensor-parallel weight shards "
                             f"(world_size={world_size})")
        # attention bias: q|k|v biases fused like the weights, an o_proj bias where the checkpoint has one
        # (Llama-architecture checkpoints with attention_bias carry all four; the Qwen2 family has none on o_proj)
        self.attn_bias = bool(getattr(cfg, "attention_bias", False))
        if self.attn_bias and world_size > 1:
            raise ValueError(f"attention bias is not supported by tensor-parallel weight shards (world_size={world_size}): "
                             "the shard's 8-row-panel and exchange GEMMs are bias-free")
        # QK norm: per-head RMSNorm of q and k before the rotation, one [D] weight each per layer
        self.qk_norm = bool(getattr(cfg, "qk_norm", False))
        if self.qk_norm and world_size > 1:
            raise ValueError(f"QK norm is not supported by tensor-parallel weight shards (world_size={world_size}): the "
                             "shard's fused q|k|v GEMMs rotate un-normalised heads")
        self.qn, self.kn = [], []                       # per layer: fp16 (D,) tensors
        self.bqkv, self.bo = [], []                     # per layer: fp16 (N,) tensors; bo[i] is None without an o_proj bias
        assert self.H % world_size == 0 and cfg.intermediate_size % world_size == 0
        self.H_local = self.H // world_size
        self.Hkv_local = self.Hkv // world_size if self.Hkv == self.H else self.Hkv
        self.I_local = cfg.intermediate_size // world_size
        self.eps = cfg.rms_norm_eps
        self.embed = self.lm_head = self.norm = None
        self.wqkv, self.wo, self.wgu, self.wd, self.ln1, self.ln2 = [], [], [], [], [], []
        self.aligned = None       # models/aligned.py: spec + read-out state of an aligned synthetic pair
        self.capture = None       # list -> the forward appends its final residual stream (pre-norm), for calibration
        self.retrieval_fp8 = False    # finalize() builds FP8 copies of the five decode GEMM weights (build_fp8_)
        self.fp8_tier = True          # ... which the spec forward uses while this is set (calibration clears it)

    # -- loading ---------------------------------------------------------------------------
    def _shard_rows(self, w, n_local):
        return w[self.rank * n_local:(self.rank + 1) * n_local]

    def _shard_cols(self, w, n_local):
        return w[:, self.rank * n_local:(self.rank + 1) * n_local]

    def load_state_dict(self, sd):
        dev, hd, kvd = self.device, self.H_local * self.D, self.Hkv_local * self.D

        def get(name):
            return sd[name].to(torch.float16)

        self.embed = get("model.embed_tokens.weight").to(dev)
        self.lm_head = get("lm_head.weight").to(dev) if "lm_head.weight" in sd else self.embed
        self.norm = get("model.norm.weight").to(dev)
        for i in range(self.L):
            p = f"model.layers.{i}."
            q = self._shard_rows(get(p + "self_attn.q_proj.weight"), hd)
            k = self._shard_rows(get(p + "self_attn.k_proj.weight"), kvd)
            v = self._shard_rows(get(p + "self_attn.v_proj.weight"), kvd)
            self.wqkv.append(torch.cat([q, k, v], dim=0).contiguous().to(dev))
            self.wo.append(self._shard_cols(get(p + "self_attn.o_proj.weight"), hd).contiguous().to(dev))
            self._load_attn_bias(sd, i, dev)
            self._load_qk_norm(sd, i, dev)
            g = self._shard_rows(get(p + "mlp.gate_proj.weight"), self.I_local)
            u = self._shard_rows(get(p + "mlp.up_proj.weight"), self.I_local)
            self.wgu.append(torch.cat([g, u], dim=0).contiguous().to(dev))
            self.wd.append(self._shard_cols(get(p + "mlp.down_proj.weight"), self.I_local).contiguous().to(dev))
            self.ln1.append(get(p + "input_layernorm.weight").to(dev))
            self.ln2.append(get(p + "post_attention_layernorm.weight").to(dev))
        return self.finalize()

    def _load_attn_bias(self, sd, i, dev):
        """self_attn.{q,k,v}_proj.bias -> the fused [q | k | v] bias of layer i, self_attn.o_proj.bias if the checkpoint has
        one.  q/k/v biases come all together or not at all, and their presence must agree with config.attention_bias."""
        p = f"model.layers.{i}.self_attn."
        have = [n for n in ("q", "k", "v") if p + n + "_proj.bias" in sd]
        if 0 < len(have) < 3:
            raise ValueError(f"layer {i}: attention bias present for {have} only; q_proj, k_proj and v_proj biases come "
                             "together")
        has_o = p + "o_proj.bias" in sd
        if bool(have) != self.attn_bias or (has_o and not self.attn_bias):
            found = [n + "_proj" for n in have] + (["o_proj"] if has_o else [])
            raise ValueError(f"layer {i}: the checkpoint has attention bias for {found or 'no projection'} but the config says "
                             f"attention_bias={self.attn_bias}")
        if not self.attn_bias:
            return
        b = torch.cat([sd[p + n + "_proj.bias"].to(torch.float16).reshape(-1) for n in ("q", "k", "v")]).contiguous()
        if b.numel() != (self.H_local + 2 * self.Hkv_local) * self.D:
            raise ValueError(f"layer {i}: attention bias has {b.numel()} q|k|v entries, expected "
                             f"{(self.H_local + 2 * self.Hkv_local) * self.D}")
        self.bqkv.append(b.to(dev))
        self.bo.append(sd[p + "o_proj.bias"].to(torch.float16).reshape(-1).contiguous().to(dev) if has_o else None)

    def _load_qk_norm(self, sd, i, dev):
        """self_attn.{q,k}_norm.weight of layer i: both or neither, and their presence must agree with config.qk_norm — a
        checkpoint with norms the path would skip, or without norms it would apply, is another model."""
        p = f"model.layers.{i}.self_attn."
        have = [n for n in ("q", "k") if p + n + "_norm.weight" in sd]
        if len(have) == 1:
            raise ValueError(f"layer {i}: QK norm weight present for {have[0]}_norm only; q_norm and k_norm come together")
        if bool(have) != self.qk_norm:
            raise ValueError(f"layer {i}: the checkpoint has {'q_norm / k_norm weights' if have else 'no q_norm / k_norm weights'}"
                             f" but the config says qk_norm={self.qk_norm}")
        if not self.qk_norm:
            return
        for lst, n in ((self.qn, "q"), (self.kn, "k")):
            w = sd[p + n + "_norm.weight"].to(torch.float16).reshape(-1).contiguous()
            if w.numel() != self.D:
                raise ValueError(f"layer {i}: {n}_norm weight has {w.numel()} entries, expected head_dim = {self.D}")
            lst.append(w.to(dev))

    def _o_bias_drawn(self):
        """Does a random draw give o_proj a bias?  Every bias config but the Qwen2 family's (q/k/v only)."""
        return self.attn_bias and getattr(self.cfg, "model_type", "llama") != "qwen2"

    def init_random(self, seed, std=0.02, bias_std=BIAS_STD):
        """Random-init directly on the device (no checkpoints offline): N(0,std) like
        modeling_llama.py:306-315; every rank draws the full matrix stream and keeps its shard
        only for the small configs — for big models each tensor is drawn shard-sized with a
        (seed, layer, name, rank)-derived generator.  A bias config draws its biases N(0, bias_std) from tags of their own
        (("bqkv", layer, rank), ("bo", layer, rank)): the matrices are the bias-free draw, bit for bit.  A QK-norm config
        draws its norm weights 1 + QK_NORM_STD * N(0, 1) from ("qn", layer) / ("kn", layer) in the same way."""
        dev, cfg = self.device, self.cfg
        hid, hd = cfg.hidden_size, self.H_local * self.D

        def draw(tag, *shape, s=std):
            g = torch.Generator(device=dev)
            g.manual_seed((seed * 1000003 + zlib.crc32(repr(tag).encode())) % (2 ** 31))
            return (torch.randn(*shape, generator=g, device=dev, dtype=torch.float32) * s).to(torch.float16)

        self.embed = draw("embed", cfg.vocab_size, hid)
        self.lm_head = draw("lm_head", cfg.vocab_size, hid)
        self.norm = torch.ones(hid, dtype=torch.float16, device=dev)
        for i in range(self.L):
            self.wqkv.append(draw(("qkv", i, self.rank), hd + 2 * self.Hkv_local * self.D, hid))
            self.wo.append(draw(("o", i, self.rank), hid, hd))
            if self.attn_bias:
                self.bqkv.append(draw(("bqkv", i, self.rank), hd + 2 * self.Hkv_local * self.D, s=bias_std))
                self.bo.append(draw(("bo", i, self.rank), hid, s=bias_std) if self._o_bias_drawn() else None)
            if self.qk_norm:
                self.qn.append((1.0 + draw(("qn", i), self.D, s=QK_NORM_STD).float()).to(torch.float16))
                self.kn.append((1.0 + draw(("kn", i), self.D, s=QK_NORM_STD).float()).to(torch.float16))
            self.wgu.append(draw(("gu", i, self.rank), 2 * self.I_local, hid))
            self.wd.append(draw(("d", i, self.rank), hid, self.I_local))
            self.ln1.append(torch.ones(hid, dtype=torch.float16, device=dev))
            self.ln2.append(torch.ones(hid, dtype=torch.float16, device=dev))
        return self.finalize()

    def overwrite_random_(self, seed, std=0.02, bias_std=BIAS_STD):
        """Re-draw every matrix IN PLACE with the values ``init_random(seed)`` would give (same storage, so captured
        hipGraphs and packed-weight pointers stay valid): lets one process measure two weight sets back to back."""
        dev, cfg = self.device, self.cfg
        assert isinstance(self.lm_head, ops.PackedLinear), "finalize() first"

        def draw_into(dst, tag, s=std):
            g = torch.Generator(device=dev)
            g.manual_seed((seed * 1000003 + zlib.crc32(repr(tag).encode())) % (2 ** 31))
            dst.copy_((torch.randn(*dst.shape, generator=g, device=dev, dtype=torch.float32) * s).to(torch.float16))

        tied = self.embed is self.lm_head.w
        draw_into(self.lm_head.w, "lm_head")
        self.lm_head.refresh_()
        if not tied:
            draw_into(self.embed, "embed")
        self.norm.fill_(1.0)
        for i in range(self.L):
            for lst, tag in ((self.wqkv, "qkv"), (self.wo, "o"), (self.wgu, "gu"), (self.wd, "d")):
                draw_into(lst[i].w, (tag, i, self.rank))
                if lst[i].bias is not None:             # (wqkv / wo of a bias config; refresh_ re-derives the rotary copy)
                    draw_into(lst[i].bias, ("b" + tag, i, self.rank), s=bias_std)
                lst[i].refresh_()
            if self.qk_norm:
                for lst, tag in ((self.qn, "qn"), (self.kn, "kn")):
                    draw_into(lst[i], (tag, i), s=QK_NORM_STD)
                    lst[i].copy_((1.0 + lst[i].float()).to(torch.float16))
            self.ln1[i].fill_(1.0)
            self.ln2[i].fill_(1.0)
        self.aligned = None
        return self

    def init_aligned(self, spec, role, attn_keys=4096):
        """Aligned synthetic weights (models/aligned.py): real shapes, dense values, planted successor table so that
        draft / retrieval / full-cache forwards agree to a tunable degree."""
        from . import aligned
        from .config_yarn import refuse_attention_bias, refuse_gqa, refuse_qk_norm
        refuse_qk_norm(self.cfg, "aligned synthetic weights (models/aligned.py init_aligned)")
        refuse_gqa(self.cfg, "aligned synthetic weights (models/aligned.py init_aligned)")
        refuse_attention_bias(self.cfg, "aligned synthetic weights (models/aligned.py init_aligned)")
        return aligned.init_weights(self, spec, role, attn_keys=attn_keys)

    def finalize(self):
        """Wrap the GEMM weights: on a HIP device each gets its MFMA-packed copy for the decode kernel."""
        PL = ops.PackedLinear
        if isinstance(self.lm_head, PL):
            return self
        tied = self.lm_head is self.embed
        self.lm_head = PL(self.lm_head)
        if tied:
            self.embed = self.lm_head.w
        rope = (self.H_local, self.D) if self.Hkv == self.H else (self.H_local, self.Hkv_local, self.D)
        if self.qk_norm:
            # the norm GEMM writes the raw q|k|v rows in natural order and tf_qk_norm_rope_append does the rest: a plain
            # packed weight, no rotary-order copy
            if self.retrieval_fp8:
                raise ValueError(f"QK norm is not supported with {RETRIEVAL_WEIGHTS_ENV}=fp8: no FP8 q|k|v weight (Fp8Linear) "
                                 "feeds the per-head norm")
            assert len(self.qn) == len(self.kn) == len(self.wqkv), "a QK-norm config needs its norm weights before finalize()"
            self.wqkv = [PL(w) for w in self.wqkv]
            self.wo = [PL(w) for w in self.wo]
        elif self.attn_bias:
            if self.retrieval_fp8:
                raise ValueError(f"attention bias is not supported with {RETRIEVAL_WEIGHTS_ENV}=fp8: the FP8 weight kernels "
                                 "have no bias epilogue")
            assert len(self.bqkv) == len(self.bo) == len(self.wqkv), "a bias config needs its biases before finalize()"
            self.wqkv = [PL(w, rope=rope, bias=b) for w, b in zip(self.wqkv, self.bqkv)]
            self.wo = [PL(w, bias=b) for w, b in zip(self.wo, self.bo)]
            self.bqkv = [pl.bias for pl in self.wqkv]        # the tensors the packed weights hold (refresh_ reads them)
            self.bo = [pl.bias for pl in self.wo]
        else:
            self.wqkv = [PL(w, rope=rope) for w in self.wqkv]
            self.wo = [PL(w) for w in self.wo]
        self.wgu = [PL(w, split=2) for w in self.wgu]
        self.wd = [PL(w) for w in self.wd]
        if self.retrieval_fp8:
            self.build_fp8_()
        return self

    def build_fp8_(self):
        """FP8 copies (ops.Fp8Linear) of q|k|v, o, gate|up, down and lm_head for the retrieval-cache forward; each is
        re-quantized in place whenever its PackedLinear is refreshed."""
        if self.Hkv != self.H:
            raise ValueError(f"GQA ({self.H} query / {self.Hkv} KV heads) is not supported by {RETRIEVAL_WEIGHTS_ENV}=fp8: "
                             "no grouped-query FP8 q|k|v epilogue exists")
        if self.attn_bias:
            raise ValueError(f"attention bias is not supported with {RETRIEVAL_WEIGHTS_ENV}=fp8: the FP8 weight kernels have "
                             "no bias epilogue")
        if self.qk_norm:
            raise ValueError(f"QK norm is not supported with {RETRIEVAL_WEIGHTS_ENV}=fp8: no FP8 q|k|v weight (Fp8Linear) feeds "
                             "the per-head norm")
        for pl in [self.lm_head] + self.wqkv + self.wo + self.wgu + self.wd:
            if pl.fp8 is None:
                pl.fp8 = ops.Fp8Linear(pl)
        return self

    def fp8_active(self):
        """Does the spec forward stream the FP8 copies right now?"""
        return self.retrieval_fp8 and self.fp8_tier and self.lm_head.fp8 is not None

    def nbytes(self):
        ts = [self.embed, self.lm_head, self.norm] + self.wqkv + self.wo + self.wgu + self.wd + self.ln1 + self.ln2
        ts = [ops._w(t) for t in ts] + [b for b in self.bqkv + self.bo if b is not None] + self.qn + self.kn
        return sum(t.numel() * t.element_size() for t in ts)


class DecoderLayers:
    """The decoder layer around its attention, once for the target, the draft and the tensor-parallel engine (whose shard
    is a LlamaWeights with fewer heads and MLP columns).  Attention stays with the engine, and so does the choice of where
    the o / down GEMM writes and what follows it (nothing here knows about process groups).

    Fused form (decode-sized blocks, ops.can_fuse): x is the residual stream — a row-major tensor or an ops.Act — and
    ``ss`` the sums of squares of x that every residual GEMM leaves for the norm prologue of the GEMM after it.
    ``f8``: stream the FP8 copies of the weights (the retrieval-verify tier).  o_fused / down_fused with ``out`` None add
    to x in place and refresh ss in the GEMM's own epilogue; with ``out`` they write the bare product there.

    Un-fused form (prefill chunks; the CPU stand-ins of the tests): x is updated by the norm that follows each GEMM, so
    the MLP output ``d`` of one layer is still pending when the next one starts (None at layer 0)."""

    def __init__(self, W, cos, sin, rotate_k=True):
        self.W, self.cos, self.sin, self.rotate_k = W, cos, sin, rotate_k

    def _kv_heads(self):
        """The KV head count for the q|k|v ops, passed only by a grouped-query model (the multi-head call is unchanged)."""
        W = self.W
        return {} if W.Hkv_local == W.H_local else {"Hkv": W.Hkv_local}

    @staticmethod
    def _bias(w, rope=False):
        """The bias of a projection for ops.linear / ops.qkv_rope (the rotary-order copy for the fused q|k|v kernel), passed
        only by a model with attention bias: the bias-free call is unchanged."""
        if w.bias is None:
            return {}
        return {"bias": w.bias_rope if rope else w.bias}

    def _capture(self, x):
        """W.capture (a list, while aligned weights are calibrated) receives the final residual stream, before the norm."""
        if self.W.capture is not None:
            self.W.capture.append(x.rows() if isinstance(x, ops.Act) else x.clone())

    # -- fused ---------------------------------------------------------------------------------
    def qkv_fused(self, i, x, ss, pos, kl, vl, slot, slot_dev=None, f8=False):
        """[norm ->] q|k|v GEMM -> RoPE -> K/V rows into kl / vl at ``slot`` (or the device scalar slot_dev); returns q."""
        W = self.W
        w = W.wqkv[i]
        if W.qk_norm:                               # norm GEMM -> raw row-major q|k|v rows, then per-head norm -> RoPE -> append
            assert not f8, "a QK-norm model has no FP8 q|k|v weight"
            rows = torch.empty(x.shape[0], w.N, dtype=torch.float16, device=W.device)
            ops.linear(x, w, ln=W.ln1[i], eps=W.eps, ss_in=ss if i > 0 else None, out=rows)
            return ops.qk_norm_rope_append(rows, W.qn[i], W.kn[i], W.eps, self.cos, self.sin, pos, kl, vl, slot, W.H_local, W.D,
                                           rotate_k=self.rotate_k, slot0_dev=slot_dev, **self._kv_heads())
        return ops.qkv_rope(x, w.fp8 if f8 else w, W.ln1[i], W.eps, self.cos, self.sin, pos, kl, vl, slot, W.H_local, W.D,
                            rotate_k=self.rotate_k, slot0_dev=slot_dev, ss_in=ss if i > 0 else None, **self._kv_heads(),
                            **self._bias(w, rope=True))

    def o_fused(self, i, a, x, ss, f8=False, out=None):
        w = self.W.wo[i].fp8 if f8 else self.W.wo[i]
        b = self._bias(self.W.wo[i])
        if out is None:
            return ops.linear(a, w, resid=x, out=x, ss_out=ss, **b)             # x += attn_out
        return ops.linear(a, w, out=out, **b)

    def gate_up_fused(self, i, x, ss, f8=False):
        W = self.W
        w = W.wgu[i]
        return ops.mlp_act(x, w.fp8 if f8 else w, ln=W.ln2[i], eps=W.eps, ss_in=ss)

    def down_fused(self, i, act, x, ss, f8=False, out=None):
        w = self.W.wd[i].fp8 if f8 else self.W.wd[i]
        if out is None:
            return ops.linear(act, w, resid=x, out=x, ss_out=ss)                # x += mlp_out
        return ops.linear(act, w, out=out)

    def head_fused(self, x, ss, f8=False, next_ids=None, logprobs_out=None):
        W = self.W
        self._capture(x)
        logits = ops.linear(x, W.lm_head.fp8 if f8 else W.lm_head, out_f32=True, ln=W.norm, eps=W.eps, ss_in=ss)
        if next_ids is not None:                    # (a prompt chunk of <= 32 rows: every row's logits exist already)
            ops.token_logprobs(logits, next_ids, out=logprobs_out)
        return logits.unsqueeze(0)

    # -- un-fused ------------------------------------------------------------------------------
    def qkv(self, i, x, d, pos, kl, vl, slot, slot_dev=None):
        W = self.W
        if d is None:
            h = ops.rmsnorm(x, W.ln1[i], W.eps)
        else:                                       # x += mlp_out of the previous layer, fused into the norm
            h = ops.rmsnorm(d, W.ln1[i], W.eps, residual=x, sum_out=x)
        if W.qk_norm:
            return ops.qk_norm_rope_append(ops.linear(h, W.wqkv[i]), W.qn[i], W.kn[i], W.eps, self.cos, self.sin, pos, kl, vl,
                                           slot, W.H_local, W.D, rotate_k=self.rotate_k, slot0_dev=slot_dev, **self._kv_heads())
        return ops.rope_append(ops.linear(h, W.wqkv[i], **self._bias(W.wqkv[i])), self.cos, self.sin, pos, kl, vl, slot, W.H_local, W.D,
                               rotate_k=self.rotate_k, slot0_dev=slot_dev, **self._kv_heads())

    def o_proj(self, i, a, out=None):
        return ops.linear(a, self.W.wo[i], out=out, **self._bias(self.W.wo[i]))

    def mlp(self, i, x, o, out=None):
        """x += o (the attention output), then the MLP: returns its output, which the next norm adds to x."""
        W = self.W
        h = ops.rmsnorm(o, W.ln2[i], W.eps, residual=x, sum_out=x)
        return ops.linear(ops.mlp_act(h, W.wgu[i]), W.wd[i], out=out)

    def head(self, x, d, last_rows=None, next_ids=None, logprobs_out=None):
        """last_rows = k: logits of the trailing k rows only (chunked prefill).
        next_ids (rows,) int64 + logprobs_out (rows,) fp32: logprobs_out[i] = log-probability of next_ids[i] under row i
        (DESIGN section 23).  The rows go through the lm_head in blocks of ops.SCORE_BLOCK_ROWS, each block's fp32 logits
        are scored by ops.token_logprobs and dropped: no (chunk, V) logits block exists.  The returned logits are unchanged."""
        W = self.W
        h = ops.rmsnorm(d, W.norm, W.eps, residual=x, sum_out=x)
        self._capture(x)
        if next_ids is not None:
            assert next_ids.numel() == h.shape[0] == logprobs_out.numel()
            for r0 in range(0, h.shape[0], ops.SCORE_BLOCK_ROWS):
                r1 = min(h.shape[0], r0 + ops.SCORE_BLOCK_ROWS)
                ops.token_logprobs(ops.linear(h[r0:r1], W.lm_head, out_f32=True), next_ids[r0:r1], out=logprobs_out[r0:r1])
        if last_rows is not None and last_rows < h.shape[0]:
            h = h[-last_rows:]
        return ops.linear(h, W.lm_head, out_f32=True).unsqueeze(0)           # (1, q, V) fp32


def load_checkpoint_state_dict(path):
    """HF directory with *.safetensors (or pytorch_model*.bin) -> flat state dict on CPU."""
    sd = {}
    st_files = sorted(f for f in os.listdir(path) if f.endswith(".safetensors"))
    if st_files:
        from safetensors.torch import load_file
        for f in st_files:
            sd.update(load_file(os.path.join(path, f)))
        return sd
    bins = sorted(f for f in os.listdir(path) if f.endswith(".bin"))
    if not bins:
        raise FileNotFoundError(f"no *.safetensors / *.bin weights under {path}")
    for f in bins:
        sd.update(torch.load(os.path.join(path, f), map_location="cpu"))
    return sd


def parse_random_spec(name_or_path):
    """``random:<seed>`` -> seed (int) else None."""
    if isinstance(name_or_path, str) and name_or_path.startswith("random"):
        parts = name_or_path.split(":")
        return int(parts[1]) if len(parts) > 1 and parts[1] else 0
    return None


def save_config(cfg, path):
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({k: v for k, v in cfg.to_dict().items() if not k.startswith("_")}, f, indent=1)
