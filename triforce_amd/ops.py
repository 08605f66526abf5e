"""Tensor-level wrappers over the C ABI (include/triforce_hip.h).

PyTorch here is plumbing only: it owns device memory and the stream; every function below
validates its tensors, takes raw device pointers and enqueues hand-written gfx950 kernels on
torch's current HIP stream (so they are captured by ``torch.cuda.graph`` like any torch op).
No CPU path exists: tensors that are not on a HIP device raise.

KV "layer views" are 3-D tensors (H, T, D) with unit stride on D and arbitrary H/T strides, so
the physical layout (head-major [L][H][T][D] in triforce_amd, token-major in the reference)
is the caller's choice.  Other modules must call these as ``ops.<name>(...)``.
"""
import ctypes
import functools

import torch
import torch.nn.functional as F

from . import hip

_HALF = torch.float16


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise hip.TriforceHipError("triforce_amd ops need HIP device tensors (no CPU fallback)")


def _dev_or_pinned(t):
    """Small result records may live in pinned host memory (device-writable under unified addressing): the host then
    polls the record instead of copying it back."""
    if not (t.is_cuda or t.is_pinned()):
        raise hip.TriforceHipError("result record must be a HIP device tensor or pinned host memory")


def _kv(t):
    assert t.dim() == 3 and t.stride(2) == 1 and t.dtype == _HALF, "KV layer view must be (H,T,D) fp16, D contiguous"
    return t.stride(1), t.stride(0)          # stride_t, stride_h


# ------------------------------------------------------------------------------------------
SKINNY_MAX_ROWS = 32
# Decode-layer fusion (env TRIFORCE_FUSE): "all" = decode-sized blocks run the fused layer — norm prologues fed by the
# GEMM-to-GEMM sum-of-squares hand-off, residual / RoPE + KV-append epilogues (5 launches per layer); "none" = one launch per
# op everywhere (9 per layer), the form prefill chunks always take.
import os as _os


def fuse_mode():
    v = _os.environ.get("TRIFORCE_FUSE", "all")
    if v not in ("all", "none"):
        raise ValueError(f"TRIFORCE_FUSE={v!r}: expected all or none")
    return v


FUSE_MODE = fuse_mode()


def fp16_or_fp8(env, override, why):
    """The value of an fp16|fp8 storage knob: ``override`` if given, else the environment variable ``env`` (default fp16).
    fp8 needs the fused decode layer (FUSE_MODE, read at the call); ``why`` is the reason clause that ends that message."""
    v = override if override is not None else _os.environ.get(env, "fp16")
    v = str(v).strip().lower() or "fp16"
    if v not in ("fp16", "fp8"):
        raise ValueError(f"{env}={v!r}: expected fp16 or fp8")
    if v == "fp8" and FUSE_MODE != "all":
        raise ValueError(f"{env}=fp8 needs the fused decode layer (TRIFORCE_FUSE=all, got {FUSE_MODE!r}): {why}")
    return v


def pack_weight(w):
    """[N, K] fp16 -> MFMA-operand order [N/16][K/32][4 (g)][16 (i)][8]: one 16x32 tile = one contiguous KiB."""
    N, K = w.shape
    assert N % 16 == 0 and K % 32 == 0 and w.dtype == _HALF
    return w.view(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()


def rope_row_order(H, Hkv, D, device=None):
    """Row permutation of a fused [q | k | v] weight for the RoPE epilogue of tf_skinny_qkv_rope: every 16-row panel
    of the q and k sections holds rows d0..d0+7 and their rotary partners d0+D/2..d0+D/2+7 of one head; v rows keep
    their order.  The q section has H heads, the k and v sections Hkv (= H: multi-head attention; < H: grouped-query
    weights, tf_skinny_qkv_rope_gqa_act)."""
    assert D % 32 == 0
    d = torch.arange(D // 2, device=device).view(D // 16, 8)
    per_head = torch.cat([d, d + D // 2], dim=1).reshape(-1)                     # (D,)
    qk = (torch.arange(H + Hkv, device=device).view(-1, 1) * D + per_head.view(1, -1)).reshape(-1)
    return torch.cat([qk, torch.arange((H + Hkv) * D, (H + 2 * Hkv) * D, device=device)])


def gqa_stack(g, sq):
    """Row-stacking rule of the grouped-query decode attention (tf_attn_decode_gqa_act): the sq rows of gs query heads of one
    KV head share a workgroup column, gs = the largest divisor of the group size g with gs * sq <= 32; returns
    (gs, g // gs = sub-groups per KV head)."""
    assert g >= 1 and 1 <= sq <= SKINNY_MAX_ROWS
    gs = max(d for d in range(1, g + 1) if g % d == 0 and d * sq <= SKINNY_MAX_ROWS)
    return gs, g // gs


def group_mean_query(q, Hkv):
    """q̄ of the grouped-query retrieval selection: q (H, D) fp16 -> (Hkv, D) fp16, the fp32 mean over
    the H / Hkv query heads of each KV head rounded to fp16.  H == Hkv: q itself, bit for bit."""
    H, D = q.shape
    if H == Hkv:
        return q
    assert H % Hkv == 0
    return q.view(Hkv, H // Hkv, D).float().mean(dim=1).to(q.dtype)


# ---- narrow panels (round 5; csrc/gemv.hip skinny_gemm_n8_kernel) ----------------------------------------------------
# The q|k|v / gate|up shards of a tensor-parallel rank have 86-120 16-row panels: one workgroup per panel leaves 2/3 of the
# 256 CUs idle and each workgroup is bound by what one CU can pull.  Weights with at most N8_MAX_PANELS 16-row panels per
# weight stream get a SECOND packed copy in 8-row panels (twice the workgroups, half the bytes each, no hand-off) that the
# two norm GEMMs use for blocks of <= 24 rows.  TRIFORCE_GEMM_N8 = 0 disables, TRIFORCE_GEMM_N8_MAX_PANELS sets the limit.
N8_ENABLED = _os.environ.get("TRIFORCE_GEMM_N8", "1") != "0"
N8_MAX_PANELS = int(_os.environ.get("TRIFORCE_GEMM_N8_MAX_PANELS", "128"))
N8_MAX_ROWS = 24
N8_MIN_K = 1024


def pack_weight_n8(w):
    """[N, K] fp16 -> narrow-panel operand order [N/8][K/64][4 (g)][2 (chunk parity)][8 (row)][8]: per 8-row panel and
    64-wide super-chunk one contiguous KiB whose 64 16-byte pieces are the A operand of ONE 16x16x32 MFMA — rows 0-7 of
    the operand = the panel's rows over the even 32-wide chunk, rows 8-15 = the same rows over the odd chunk."""
    N, K = w.shape
    assert N % 8 == 0 and K % 64 == 0 and w.dtype == _HALF
    return w.view(N // 8, 8, K // 64, 2, 4, 8).permute(0, 2, 4, 3, 1, 5).contiguous()


def rope_row_order_n8(H, D, device=None):
    """rope_row_order for 8-row panels: every panel of the q and k sections holds rows d0..d0+3 and their rotary partners
    d0+D/2..d0+D/2+3 of one head; v rows keep their order."""
    assert D % 32 == 0
    d = torch.arange(D // 2, device=device).view(D // 8, 4)
    per_head = torch.cat([d, d + D // 2], dim=1).reshape(-1)                     # (D,)
    qk = (torch.arange(2 * H, device=device).view(-1, 1) * D + per_head.view(1, -1)).reshape(-1)
    return torch.cat([qk, torch.arange(2 * H * D, 3 * H * D, device=device)])


def n8_applies(N_stream, K):
    """Does a weight stream of N_stream rows x K get (and use) the narrow-panel copy?"""
    return (N8_ENABLED and N_stream % 16 == 0 and N_stream // 16 <= N8_MAX_PANELS and K % 64 == 0 and K >= N8_MIN_K)


# Split-K workspace of the skinny GEMM (csrc/gemv.hip SgKsplit, tf_sg_workspace): one zero-filled 8 MiB block per device,
# registered when the first weight is packed there (i.e. before any hipGraph capture) and never freed.  Few-panel GEMMs
# (the q|k|v / gate|up shards of a tensor-parallel rank) can then split K across up to 4 workgroups per panel —
# TRIFORCE_GEMM_KSPLIT=1; off by default: measured without gain in situ (profiles/r04_tp_shard_structural_ab.jsonl).
_SG_WS = {}
_SG_WS_BYTES = 8 << 20


def _ensure_sg_workspace(device):
    device = torch.device(device)
    if device.type != "cuda" or device in _SG_WS:
        return
    with torch.cuda.device(device):
        ws = torch.zeros(_SG_WS_BYTES, dtype=torch.uint8, device=device)
        torch.cuda.synchronize(device)
        hip.check(hip.lib().tf_sg_workspace(_ptr(ws), ws.numel()), "tf_sg_workspace")
        if _os.environ.get("TRIFORCE_GEMM_KSPLIT", "0") == "1":          # measured: no gain (csrc/gemv.hip) — opt-in
            hip.lib().tf_sg_tune(3, 200)
        if "TRIFORCE_GEMM_P2_GROUPS" in _os.environ:                     # A/B: two panels per wave while panels / 2 >= this
            hip.lib().tf_sg_tune(2, int(_os.environ["TRIFORCE_GEMM_P2_GROUPS"]))
        if "TRIFORCE_GEMM_FEW_PANELS" in _os.environ:                    # A/B: largest panel count that runs 16 waves per panel
            hip.lib().tf_sg_tune(5, int(_os.environ["TRIFORCE_GEMM_FEW_PANELS"]))
    _SG_WS[device] = ws


def _rope3(rope):
    """(H, Hkv, D) of a PackedLinear ``rope`` mark: (H, D) or (H, Hkv, D)."""
    return (rope[0], rope[0], rope[1]) if len(rope) == 2 else tuple(rope)


def _rope_rows(rope):
    H, Hkv, D = _rope3(rope)
    return (H + 2 * Hkv) * D


class PackedLinear:
    """A weight matrix with (on a HIP device) its pre-packed copy for the skinny decode GEMM.  ``w`` stays
    available for the >32-row prefill GEMMs (hipBLASLt).  ``split`` = number of equal row blocks that were
    fused (2 for gate|up) — each block is packed on its own so the SwiGLU kernel can pair them.  ``rope=(H, D)``
    marks a fused q|k|v weight: a second packed copy in rotary-pair row order feeds tf_skinny_qkv_rope.
    ``rope=(H, Hkv, D)`` with Hkv < H marks a grouped-query weight ([q: H D | k: Hkv D | v: Hkv D] rows): its rotary copy
    feeds tf_skinny_qkv_rope_gqa_act, and it gets neither the 8-row-panel copy nor an FP8 copy (no GQA epilogue exists
    for either).  ``bias`` = fp16 (N,) bias of the projection (attention bias), rows in ``w``'s order; a
    rope weight keeps a second copy ``bias_rope`` in the rotary row order of ``wp_rope``, which is what the fused q|k|v
    kernel reads.  A biased weight gets neither the 8-row-panel copy nor an FP8 copy (bias-free forms)."""

    def __init__(self, w, split=1, pack=None, rope=None, bias=None):
        self.w = w
        self.N, self.K = w.shape
        self.split = split
        pack = w.is_cuda if pack is None else pack
        ok = pack and (self.N // split) % 16 == 0 and self.K % 32 == 0
        if ok and w.is_cuda:
            _ensure_sg_workspace(w.device)
        self.parts = [pack_weight(b) for b in w.chunk(split, dim=0)] if ok else None
        self.wp = self.parts[0] if (ok and split == 1) else None
        self.rope = rope
        self.wp_rope = None
        self.gqa = rope is not None and len(rope) == 3 and rope[1] != rope[0]
        if rope is not None and len(rope) == 3 and not self.gqa:
            self.rope = rope = (rope[0], rope[2])                 # equal head counts: the multi-head spelling
        if ok and rope is not None and rope[-1] % 32 == 0 and self.N == _rope_rows(rope):
            self.wp_rope = pack_weight(w[rope_row_order(*_rope3(rope), w.device)])
        # narrow-panel copies (few-panel shards only): gate|up streams, and the q|k|v weight in its 8-row rotary order
        self.parts_n8 = self.wp_rope_n8 = None
        if ok and w.is_cuda and split == 2 and n8_applies(self.N // split, self.K):
            self.parts_n8 = [pack_weight_n8(b) for b in w.chunk(split, dim=0)]
        self.bias = self.bias_rope = None
        if bias is not None:
            assert split == 1 and bias.dtype == _HALF and tuple(bias.shape) == (self.N,) and bias.device == w.device
            self.bias = bias.contiguous()
            if rope is not None and rope[-1] % 32 == 0 and self.N == _rope_rows(rope):
                self.bias_rope = self.bias[rope_row_order(*_rope3(rope), w.device)].contiguous()
        if self.wp_rope is not None and not self.gqa and bias is None and w.is_cuda and n8_applies(self.N, self.K):
            self.wp_rope_n8 = pack_weight_n8(w[rope_row_order_n8(rope[0], rope[1], w.device)])
        self.fp8 = None           # Fp8Linear of the retrieval-verify tier (models/llama_core.LlamaWeights.build_fp8_)

    def refresh_(self):
        """Re-pack IN PLACE after ``self.w`` was modified in place (captured hipGraphs keep their pointers)."""
        if self.parts is not None:
            for dst, blk in zip(self.parts, self.w.chunk(self.split, dim=0)):
                dst.copy_(pack_weight(blk))
        if self.wp_rope is not None:
            self.wp_rope.copy_(pack_weight(self.w[rope_row_order(*_rope3(self.rope), self.w.device)]))
        if self.bias_rope is not None:                                        # (``bias`` itself is what was modified in place)
            self.bias_rope.copy_(self.bias[rope_row_order(*_rope3(self.rope), self.w.device)])
        if self.parts_n8 is not None:
            for dst, blk in zip(self.parts_n8, self.w.chunk(self.split, dim=0)):
                dst.copy_(pack_weight_n8(blk))
        if self.wp_rope_n8 is not None:
            self.wp_rope_n8.copy_(pack_weight_n8(self.w[rope_row_order_n8(self.rope[0], self.rope[1], self.w.device)]))
        if self.fp8 is not None:
            self.fp8.refresh_()
        return self


# ---- FP8 weights of the retrieval-verify tier (csrc/gemv_fp8.hip; TRIFORCE_RETRIEVAL_WEIGHTS=fp8) ------
# Weight-only e4m3fn codes with one fp32 scale per output row; the kernels decode the codes to fp16 exactly and apply the
# scale to the fp32 accumulator where the 16-bit kernel rounds (include/triforce_hip.h, "FP8-WEIGHT forms").
FP8_MAX = 448.0


def quantize_fp8_rows(w):
    """[N, K] weight -> (codes [N, K] uint8, scale [N] fp32): s[n] = amax_k |W[n, k]| / 448 in fp32 (1 for an all-zero
    row), code = e4m3fn(W / s) rounded to nearest even, clamped to +-448 BEFORE the cast (the cast itself turns values
    past the largest finite e4m3fn value into NaN)."""
    w32 = w.float()
    amax = w32.abs().amax(dim=1)
    s = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    q = (w32 / s[:, None]).clamp_(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), s


def dequantize_fp8_rows(codes, scale):
    """s[n] * decode(code[n, k]) in fp32 (exact: every e4m3fn value is an fp32 value)."""
    return codes.view(torch.float8_e4m3fn).float() * scale.float()[:, None]


def pack_weight_fp8(codes):
    """[N, K] uint8 e4m3fn codes -> [N/16][K/64][4 (g)][16 (i)][16]: per 16-row panel and 64-wide super-chunk one contiguous
    KiB; the 16 bytes of piece (g, i) are row i's k-octet g of the even 32-wide chunk, then its k-octet g of the odd one
    (the A operands of the two f16 MFMAs that 16-byte load feeds)."""
    N, K = codes.shape
    assert N % 16 == 0 and K % 64 == 0 and codes.dtype == torch.uint8
    return codes.view(N // 16, 16, K // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).reshape(N // 16, K // 64, 4, 16, 16).contiguous()


def unpack_weight_fp8(packed):
    """Inverse of pack_weight_fp8."""
    P, S = packed.shape[0], packed.shape[1]
    return packed.view(P, S, 4, 16, 2, 8).permute(0, 3, 1, 4, 2, 5).reshape(P * 16, S * 64).contiguous()


class Fp8Linear:
    """FP8 copy of a PackedLinear for the FP8-weight skinny GEMMs: per weight stream (one; two for a fused gate|up) the
    packed e4m3fn codes and the fp32 row scales, rows in the order the kernel reads them (a q|k|v weight, ``rope``, in
    rope_row_order).  Built from — and re-quantized by ``refresh_()`` from — the PackedLinear's fp16 ``w``."""

    def __init__(self, pl):
        assert isinstance(pl, PackedLinear)
        self.src, self.N, self.K, self.split, self.rope = pl, pl.N, pl.K, pl.split, pl.rope
        if getattr(pl, "bias", None) is not None:
            raise ValueError(f"attention bias: a biased {pl.N} x {pl.K} weight is not supported by the FP8 weight tier "
                             "(Fp8Linear): the FP8 kernels have no bias epilogue")
        if getattr(pl, "gqa", False):
            raise ValueError(f"GQA q|k|v weight (H, Hkv, D = {pl.rope}) is not supported by the FP8 weight tier (Fp8Linear): "
                             "no grouped-query FP8 epilogue exists")
        if not pl.w.is_cuda:
            raise hip.TriforceHipError("FP8 weights need a HIP device tensor (no CPU fallback)")
        if self.K % 64 or (self.N // self.split) % 16 or self.N % self.split:
            raise hip.TriforceHipError(f"FP8 weights: unsupported shape {self.N} x {self.K} (rows per stream % 16, K % 64)")
        if self.rope is not None and (self.rope[1] % 32 or self.N != 3 * self.rope[0] * self.rope[1]):
            raise hip.TriforceHipError(f"FP8 weights: q|k|v weight {self.N} x {self.K} does not match H, D = {self.rope}")
        self.codes, self.scales = [], []
        for blk in self._streams():
            c, s = quantize_fp8_rows(blk)
            self.codes.append(pack_weight_fp8(c))
            self.scales.append(s.contiguous())

    def _streams(self):
        w = self.src.w
        if self.rope is not None:
            return [w[rope_row_order(self.rope[0], self.rope[0], self.rope[1], w.device)]]
        return list(w.chunk(self.split, dim=0))

    def refresh_(self):
        """Re-quantize IN PLACE after the fp16 weight changed (captured hipGraphs keep these pointers)."""
        for dst_c, dst_s, blk in zip(self.codes, self.scales, self._streams()):
            c, s = quantize_fp8_rows(blk)
            dst_c.copy_(pack_weight_fp8(c))
            dst_s.copy_(s)
        return self

    def dequantized(self):
        """The fp32 weight this copy stands for, in the fp16 weight's row order (oracles of the tests)."""
        rows = [dequantize_fp8_rows(unpack_weight_fp8(c), s) for c, s in zip(self.codes, self.scales)]
        w = torch.cat(rows, dim=0)
        if self.rope is not None:
            out = torch.empty_like(w)
            out[rope_row_order(self.rope[0], self.rope[0], self.rope[1], w.device)] = w
            return out
        return w

    def nbytes(self):
        return sum(c.numel() + 4 * s.numel() for c, s in zip(self.codes, self.scales))


def _fp8_rows_ok(x, w):
    if not (x.is_cuda and x.shape[0] <= SKINNY_MAX_ROWS and x.dtype == _HALF and x.shape[1] == w.K):
        raise hip.TriforceHipError(f"FP8 weights run only on the skinny decode kernels (<= {SKINNY_MAX_ROWS} fp16 device rows "
                                   f"of width {w.K}); got {tuple(x.shape)} {x.dtype}")


def _w(w):
    return w.w if isinstance(w, PackedLinear) else w


# ---- activation layouts of the decode path (include/triforce_hip.h, tf_skinny_gemm_act) -------------------------------
# Element (m, k) of an activation block lives at base[m * sm + (k // 8) * sk + k % 8].  The reference's tensors are
# row-major (sm = row stride, sk = 8).  The decode layer of this package keeps its residual stream, attention output and
# SwiGLU output K-OCTET-MAJOR (sm = 8, sk = 8 * rows): the B operand of a 16-row MFMA tile is then 4 runs of 256 bytes
# instead of 16 row fragments of 64 bytes — the 17..32-row GEMMs of the gamma = 16 verifies were bound by exactly those
# fragments (profiles/r03_gemm_rows_ab.jsonl: 13B q|k|v 29.7 us at 8 rows, 44.0 at 17; k-octet-major: 27.6 at 17,
# profiles/r04_gemm_layout_ab.jsonl).  TRIFORCE_ACT_LAYOUT = auto (default: see act_packed) | packed | rows.
ACT_LAYOUT = _os.environ.get("TRIFORCE_ACT_LAYOUT", "auto")
# auto: from 17 rows (two MFMA row tiles) — measured in situ (profiles/r04_act_layout_in_situ.jsonl): 13B gamma = 16
# retrieval verify 9 198 -> 8 319 us, target verify 25 640 -> 24 578; 7B gamma = 16 retrieval verify 5 287 -> 5 024; at
# 7 rows 3 345 -> 3 303 (1 %) and the tensor-parallel shard's eager 1-row step LOSES (host cost of the Act wrappers)
ACT_PACKED_MIN_ROWS = int(_os.environ.get("TRIFORCE_ACT_PACKED_MIN_ROWS", "17"))


def act_packed(rows):
    """Should a decode forward of ``rows`` rows keep its activations k-octet-major?"""
    if ACT_LAYOUT == "packed":
        return True
    if ACT_LAYOUT == "rows":
        return False
    return rows >= ACT_PACKED_MIN_ROWS


class Act:
    """A k-octet-major activation block: ``t`` is a contiguous (K/8, R, 8) fp16 tensor holding rows 0..M-1 of an (M, K)
    block (R >= M).  Quacks like the (M, K) tensor where the model code looks at it (shape, device, dtype, clone)."""
    __slots__ = ("t", "M", "K")

    def __init__(self, t, M):
        assert t.dim() == 3 and t.shape[2] == 8 and t.is_contiguous() and t.dtype == _HALF and t.shape[1] >= M
        self.t, self.M, self.K = t, M, t.shape[0] * 8

    @classmethod
    def empty(cls, M, K, device, R=None):
        return cls(torch.empty(K // 8, M if R is None else R, 8, dtype=_HALF, device=device), M)

    @classmethod
    def from_rows(cls, x, R=None):
        return cls(pack_act(x, R), x.shape[0])

    @classmethod
    def over(cls, flat, M, K):
        """View a flat fp16 buffer of M * K elements (e.g. the all-reduce staging area) as an M-row block."""
        assert flat.numel() == M * K and flat.is_contiguous()
        return cls(flat.view(K // 8, M, 8), M)

    R = property(lambda self: self.t.shape[1])
    sm = property(lambda self: 8)
    sk = property(lambda self: 8 * self.t.shape[1])
    shape = property(lambda self: (self.M, self.K))
    device = property(lambda self: self.t.device)
    dtype = property(lambda self: self.t.dtype)
    is_cuda = property(lambda self: self.t.is_cuda)

    def data_ptr(self):
        return self.t.data_ptr()

    def numel(self):
        return self.M * self.K

    def rows(self):
        """Row-major (M, K) copy."""
        return unpack_act(self.t, self.M)

    def clone(self):
        return Act(self.t.clone(), self.M)

    def copy_(self, other):
        if isinstance(other, Act):
            assert other.shape == self.shape and other.R == self.R
            self.t.copy_(other.t)
        else:
            self.t[:, :self.M].copy_(other.view(self.M, self.K // 8, 8).permute(1, 0, 2))
        return self


def _lay(x):
    """(pointer, sm, sk) of an activation operand: an Act, a row-major 2-D tensor, or None."""
    if x is None:
        return None, 8, 8
    if isinstance(x, Act):
        return _ptr(x.t), x.sm, x.sk
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == _HALF
    return _ptr(x), x.stride(0), 8


def pack_act(x, R=None):
    """Row-major (M, K) fp16 -> k-octet-major block (K/8, R, 8): element (m, k) at [(k // 8), m, k % 8]; R >= M rows
    (rows M..R-1 are zero).  Strides for the *_act entry points: s_m = 8, s_k = 8 * R."""
    M, K = x.shape
    R = M if R is None else R
    assert K % 8 == 0 and R >= M and x.dtype == _HALF
    out = torch.zeros(K // 8, R, 8, dtype=_HALF, device=x.device)
    out[:, :M] = x.reshape(M, K // 8, 8).permute(1, 0, 2)
    return out


def unpack_act(xp, M):
    """Inverse of pack_act: (K/8, R, 8) -> row-major (M, K)."""
    K8, R, _ = xp.shape
    return xp[:, :M].permute(1, 0, 2).reshape(M, K8 * 8).contiguous()


def embed_rows(embed, ids, packed, out=None):
    """x = embed[ids] for the <= 32 rows of a decode forward: a row-major tensor, or (packed) an Act written by
    tf_embed_rows straight in the k-octet-major form.  ``out``: write into this tensor / Act (static graph buffers)."""
    ids = ids.reshape(-1)
    if not packed:
        if embed.is_cuda and embed.dtype == _HALF and embed.is_contiguous() and ids.numel() <= 32 and ids.dtype == torch.int64 \
                and ids.is_contiguous() and embed.shape[1] % 8 == 0 and (out is None or (out.is_contiguous() and out.dtype == _HALF)):
            # the same kernel with row-major strides (round 5: no torch gather kernel left inside the captured decode forwards)
            n, (V, hid) = ids.numel(), embed.shape
            x = torch.empty(n, hid, dtype=_HALF, device=embed.device) if out is None else out
            assert tuple(x.shape) == (n, hid)
            hip.check(hip.lib().tf_embed_rows(_ptr(embed), _ptr(ids), _ptr(x), hid, 8, n, hid, V, _stream()), "tf_embed_rows")
            return x
        if out is None:
            return embed[ids]
        return out.copy_(embed[ids])
    _dev(embed, ids)
    assert embed.dtype == _HALF and embed.is_contiguous() and ids.dtype == torch.int64 and ids.is_contiguous()
    n, (V, hid) = ids.numel(), embed.shape
    x = Act.empty(n, hid, embed.device) if out is None else out
    assert isinstance(x, Act) and x.shape == (n, hid)
    hip.check(hip.lib().tf_embed_rows(_ptr(embed), _ptr(ids), _ptr(x.t), x.sm, x.sk, n, hid, V, _stream()), "tf_embed_rows")
    return x


def set_tokens(dst, vals, pad, pos=None, pos0=0, slot=None, sk=None, sk_val=0):
    """dst (int64, <= 32 entries) = vals padded with ``pad``; pos (int64) = pos0 + arange; slot / sk (int32 scalars) =
    pos0 / sk_val — one launch, the ids passed as kernel arguments (tf_set_tokens).  ``vals``: python ints."""
    n_dst = 0 if dst is None else dst.numel()
    n_vals = len(vals)
    assert n_vals <= 32 and n_dst <= 32 and (dst is None or (dst.dtype == torch.int64 and dst.is_contiguous()))
    assert pos is None or (pos.dtype == torch.int64 and pos.is_contiguous() and pos.numel() <= 64)
    assert (slot is None or slot.dtype == torch.int32) and (sk is None or sk.dtype == torch.int32)
    _dev(dst, pos, slot, sk)
    host = (ctypes.c_int64 * max(n_vals, 1))(*[int(v) for v in vals])
    hip.check(hip.lib().tf_set_tokens(_ptr(dst), n_dst, host, n_vals, int(pad), _ptr(pos), 0 if pos is None else pos.numel(),
                                      int(pos0), _ptr(slot), _ptr(sk), int(sk_val), _stream()), "tf_set_tokens")


def can_fuse(x, *ws):
    """True when the fused decode kernels apply: HIP tensors, <= 32 rows, every weight packed."""
    return (x.is_cuda and x.dim() == 2 and x.shape[0] <= SKINNY_MAX_ROWS and x.dtype == _HALF and x.stride(1) == 1
            and all(isinstance(w, PackedLinear) and w.parts is not None for w in ws))


def can_fuse_rows(rows, embed, *ws):
    """can_fuse before the embedding rows exist: ``rows`` rows of ``embed`` (device fp16 table) against packed weights."""
    return (embed.is_cuda and embed.dtype == _HALF and rows <= SKINNY_MAX_ROWS
            and all(isinstance(w, PackedLinear) and w.parts is not None for w in ws))


def linear(x, w, out_f32=False, ln=None, eps=0.0, resid=None, out=None, ss_in=None, ss_out=None, bias=None):
    """y = x . W^T, fp16 with fp32 accumulation — the reference's nn.Linear / F.linear.  <=32 rows against a
    PackedLinear run the hand-written weight-streaming kernel; larger blocks (prefill) go to hipBLASLt.
    Fused forms of the skinny kernel (only valid when ``can_fuse``): ``ln`` = RMSNorm weight applied to x first
    (h = ln * fp16(x * rsqrt(mean(x^2)+eps))), ``resid`` = fp16 residual added to the fp16 result, ``out`` = where
    to write (may be ``resid`` itself); ``ss_out`` (N/16, 32) fp32 receives the per-panel sums of squares of the
    output rows and ``ss_in`` feeds such partials of x to the norm prologue (see ``ss_buffer``).
    x / resid / out may be ``Act`` blocks (k-octet-major); an Act input gives an Act output unless ``out`` says
    otherwise (fp32 logits are always a row-major tensor).
    ``bias`` (N,) fp16, rows in W's order: y = fp16(acc + float(bias)) before the residual add (tf_skinny_gemm_bias_act);
    prefill blocks take F.linear(x, W, bias).  No bias with fp32 output or FP8 weights."""
    M = x.shape[0]
    f8 = isinstance(w, Fp8Linear)
    if bias is not None:
        assert not f8 and not out_f32 and bias.dtype == _HALF and bias.is_contiguous() and tuple(bias.shape) == (_w(w).shape[0],)
    if f8:
        _fp8_rows_ok(x, w)
        assert w.split == 1 and w.rope is None, "an FP8 gate|up / q|k|v weight runs through mlp_act / qkv_rope"
    if f8 or (isinstance(w, PackedLinear) and w.wp is not None and M <= SKINNY_MAX_ROWS and x.is_cuda):
        assert x.dtype == _HALF and x.shape[1] == w.K
        if out is None:
            if out_f32 or not isinstance(x, Act):
                out = torch.empty(M, w.N, dtype=torch.float32 if out_f32 else _HALF, device=x.device)
            else:
                out = Act.empty(M, w.N, x.device)
        assert tuple(out.shape) == (M, w.N)
        if resid is not None:
            assert tuple(resid.shape) == tuple(out.shape) and resid.dtype == _HALF and not out_f32
        if ss_in is not None:
            assert ss_in.dtype == torch.float32 and ss_in.shape == (w.K // 16, 32) and ss_in.is_contiguous()
        if ss_out is not None:
            assert ss_out.dtype == torch.float32 and ss_out.shape == (w.N // 16, 32) and ss_out.is_contiguous()
        xp, xsm, xsk = _lay(x)
        rp, rsm, rsk = _lay(resid)
        if out_f32:
            assert out.dtype == torch.float32 and out.stride(1) == 1
            yp, ysm, ysk = _ptr(out), out.stride(0), 8
        else:
            yp, ysm, ysk = _lay(out)
        if f8:
            hip.check(hip.lib().tf_skinny_gemm_fp8_act(_ptr(w.codes[0]), _ptr(w.scales[0]), xp, xsm, xsk, _ptr(ln), float(eps),
                                                       _ptr(ss_in), rp, rsm, rsk, _ptr(ss_out), yp, ysm, ysk, M, w.N, w.K,
                                                       1 if out_f32 else 0, _stream()), "tf_skinny_gemm_fp8_act")
            return out
        if bias is not None:
            _dev(bias)
            hip.check(hip.lib().tf_skinny_gemm_bias_act(_ptr(w.wp), xp, xsm, xsk, _ptr(ln), float(eps), _ptr(ss_in), rp, rsm,
                                                        rsk, _ptr(ss_out), yp, ysm, ysk, M, w.N, w.K, 0, _ptr(bias), _stream()),
                      "tf_skinny_gemm_bias_act")
            return out
        hip.check(hip.lib().tf_skinny_gemm_act(_ptr(w.wp), xp, xsm, xsk, _ptr(ln), float(eps), _ptr(ss_in), rp, rsm, rsk,
                                               _ptr(ss_out), yp, ysm, ysk, M, w.N, w.K, 1 if out_f32 else 0, _stream()),
                  "tf_skinny_gemm_act")
        return out
    assert ln is None and resid is None and out is None and ss_in is None and ss_out is None, \
        "fused linear needs the skinny kernel (ops.can_fuse)"
    assert not isinstance(x, Act), "k-octet-major activations exist only on the skinny decode path"
    y = F.linear(x, _w(w)) if bias is None else F.linear(x, _w(w), bias)
    return y.float() if out_f32 else y


def mlp_act(h, wgu, ln=None, eps=0.0, ss_in=None):
    """fp16(silu(gate(h))) * up(h) for a fused gate|up weight: one kernel for <=32 rows (optionally with the
    RMSNorm of h folded in, ``ln``), GEMM + silu_mul otherwise.  An Act input gives an Act output."""
    M = h.shape[0]
    if isinstance(wgu, Fp8Linear):
        _fp8_rows_ok(h, wgu)
        assert wgu.split == 2, "mlp_act takes a fused gate|up weight"
        I = wgu.N // 2
        act = Act.empty(M, I, h.device) if isinstance(h, Act) else torch.empty(M, I, dtype=_HALF, device=h.device)
        hp, hsm, hsk = _lay(h)
        ap, asm, ask = _lay(act)
        hip.check(hip.lib().tf_skinny_gemm_swiglu_fp8_act(_ptr(wgu.codes[0]), _ptr(wgu.scales[0]), _ptr(wgu.codes[1]),
                                                          _ptr(wgu.scales[1]), hp, hsm, hsk, _ptr(ln), float(eps), _ptr(ss_in),
                                                          ap, asm, ask, M, I, wgu.K, _stream()), "tf_skinny_gemm_swiglu_fp8_act")
        return act
    if isinstance(wgu, PackedLinear) and wgu.parts is not None and wgu.split == 2 and M <= SKINNY_MAX_ROWS \
            and h.is_cuda:
        I = wgu.N // 2
        act = Act.empty(M, I, h.device) if isinstance(h, Act) else torch.empty(M, I, dtype=_HALF, device=h.device)
        hp, hsm, hsk = _lay(h)
        ap, asm, ask = _lay(act)
        if wgu.parts_n8 is not None and ln is not None and M <= N8_MAX_ROWS:        # few-panel shard: 8-row panels
            hip.check(hip.lib().tf_skinny_gemm_swiglu_n8(_ptr(wgu.parts_n8[0]), _ptr(wgu.parts_n8[1]), hp, hsm, hsk, _ptr(ln),
                                                         float(eps), _ptr(ss_in), ap, asm, ask, M, I, wgu.K, _stream()),
                      "tf_skinny_gemm_swiglu_n8")
            return act
        hip.check(hip.lib().tf_skinny_gemm_swiglu_act(_ptr(wgu.parts[0]), _ptr(wgu.parts[1]), hp, hsm, hsk, _ptr(ln),
                                                      float(eps), _ptr(ss_in), ap, asm, ask, M, I, wgu.K, _stream()),
                  "tf_skinny_gemm_swiglu_act")
        return act
    assert ln is None and not isinstance(h, Act), "fused mlp_act needs the skinny kernel (ops.can_fuse)"
    return silu_mul(F.linear(h, _w(wgu)))


def ss_buffer(hidden, device):
    """Hand-off buffer for the residual stream's per-panel sums of squares (hidden/16 panels x 32 rows, fp32)."""
    return torch.empty(hidden // 16, 32, dtype=torch.float32, device=device)


def qkv_rope(x, wqkv, ln, eps, cos, sin, positions, k_layer, v_layer, slot0, H, D, rotate_k=True, slot0_dev=None,
             ss_in=None, Hkv=None, bias=None):
    """One kernel for [RMSNorm ->] fused q|k|v GEMM -> RoPE -> KV append: x (rows, hidden) is the residual stream
    (ln = input_layernorm weight, or None when x is already normalised; a row-major tensor or an Act); q (rows,H,D)
    is returned rotated, the k (rotated unless rotate_k is False) and v rows land in the cache at slot0+i.
    ``Hkv`` < H: a grouped-query weight (PackedLinear rope=(H, Hkv, D)), k / v rows go to the Hkv heads of the cache.
    ``bias``: the weight's q|k|v bias IN ROTARY ROW ORDER (PackedLinear.bias_rope), added to the GEMM result before the
    rotation (tf_skinny_qkv_rope[_gqa]_bias_act); never the 8-row-panel or FP8 forms."""
    _dev(ln, cos, sin, positions, k_layer, v_layer, slot0_dev, bias)
    gqa = Hkv is not None and Hkv != H
    f8 = isinstance(wqkv, Fp8Linear)
    if bias is not None:
        assert not f8 and bias is wqkv.bias_rope, "qkv_rope takes the PackedLinear's own rotary-order bias"
    if f8:
        _fp8_rows_ok(x, wqkv)
    assert f8 or (isinstance(wqkv, PackedLinear) and wqkv.wp_rope is not None)
    assert wqkv.rope == ((H, Hkv, D) if gqa else (H, D))
    rows = x.shape[0]
    assert x.is_cuda and x.dtype == _HALF and x.shape[1] == wqkv.K and rows <= SKINNY_MAX_ROWS
    assert positions.dtype == torch.int64 and positions.numel() == rows and positions.is_contiguous()
    assert cos.dtype == _HALF and cos.is_contiguous() and cos.shape[1] == D
    st, sh = _kv(k_layer)
    assert _kv(v_layer) == (st, sh)
    q = torch.empty(rows, H, D, dtype=_HALF, device=x.device)
    xp, xsm, xsk = _lay(x)
    if gqa:
        assert not f8 and k_layer.shape[0] == Hkv and v_layer.shape[0] == Hkv and H % Hkv == 0
        if bias is not None:
            hip.check(hip.lib().tf_skinny_qkv_rope_gqa_bias_act(_ptr(wqkv.wp_rope), xp, xsm, xsk, _ptr(ln), float(eps),
                                                                _ptr(ss_in), _ptr(cos), _ptr(sin), _ptr(positions), _ptr(q),
                                                                _ptr(k_layer), _ptr(v_layer), st, sh, int(slot0),
                                                                _ptr(slot0_dev), rows, H, Hkv, D, wqkv.K,
                                                                1 if rotate_k else 0, _ptr(bias), _stream()),
                      "tf_skinny_qkv_rope_gqa_bias_act")
            return q
        hip.check(hip.lib().tf_skinny_qkv_rope_gqa_act(_ptr(wqkv.wp_rope), xp, xsm, xsk, _ptr(ln), float(eps), _ptr(ss_in),
                                                       _ptr(cos), _ptr(sin), _ptr(positions), _ptr(q), _ptr(k_layer),
                                                       _ptr(v_layer), st, sh, int(slot0), _ptr(slot0_dev), rows, H, Hkv, D,
                                                       wqkv.K, 1 if rotate_k else 0, _stream()), "tf_skinny_qkv_rope_gqa_act")
        return q
    if f8:
        hip.check(hip.lib().tf_skinny_qkv_rope_fp8_act(_ptr(wqkv.codes[0]), _ptr(wqkv.scales[0]), xp, xsm, xsk, _ptr(ln),
                                                       float(eps), _ptr(ss_in), _ptr(cos), _ptr(sin), _ptr(positions), _ptr(q),
                                                       _ptr(k_layer), _ptr(v_layer), st, sh, int(slot0), _ptr(slot0_dev), rows,
                                                       H, D, wqkv.K, 1 if rotate_k else 0, _stream()),
                  "tf_skinny_qkv_rope_fp8_act")
        return q
    if bias is not None:
        hip.check(hip.lib().tf_skinny_qkv_rope_bias_act(_ptr(wqkv.wp_rope), xp, xsm, xsk, _ptr(ln), float(eps), _ptr(ss_in),
                                                        _ptr(cos), _ptr(sin), _ptr(positions), _ptr(q), _ptr(k_layer),
                                                        _ptr(v_layer), st, sh, int(slot0), _ptr(slot0_dev), rows, H, D,
                                                        wqkv.K, 1 if rotate_k else 0, _ptr(bias), _stream()),
                  "tf_skinny_qkv_rope_bias_act")
        return q
    if wqkv.wp_rope_n8 is not None and ln is not None and rows <= N8_MAX_ROWS:      # few-panel shard: 8-row panels
        hip.check(hip.lib().tf_skinny_qkv_rope_n8(_ptr(wqkv.wp_rope_n8), xp, xsm, xsk, _ptr(ln), float(eps), _ptr(ss_in),
                                                  _ptr(cos), _ptr(sin), _ptr(positions), _ptr(q), _ptr(k_layer),
                                                  _ptr(v_layer), st, sh, int(slot0), _ptr(slot0_dev), rows, H, D, wqkv.K,
                                                  1 if rotate_k else 0, _stream()), "tf_skinny_qkv_rope_n8")
        return q
    hip.check(hip.lib().tf_skinny_qkv_rope_act(_ptr(wqkv.wp_rope), xp, xsm, xsk, _ptr(ln), float(eps), _ptr(ss_in),
                                               _ptr(cos), _ptr(sin), _ptr(positions), _ptr(q), _ptr(k_layer),
                                               _ptr(v_layer), st, sh, int(slot0), _ptr(slot0_dev), rows, H, D, wqkv.K,
                                               1 if rotate_k else 0, _stream()), "tf_skinny_qkv_rope_act")
    return q


def rmsnorm(x, w, eps, residual=None, sum_out=None):
    """y = w * fp16((x [+ residual]) * rsqrt(mean(.^2)+eps)); writes the fp16 sum to sum_out if given."""
    _dev(x, w, residual, sum_out)
    assert x.dtype == _HALF and x.is_contiguous() and x.dim() == 2
    y = torch.empty_like(x)
    hip.check(hip.lib().tf_rmsnorm(_ptr(x), _ptr(residual), _ptr(w), _ptr(y), _ptr(sum_out), x.shape[0], x.shape[1],
                                   float(eps), _stream()), "tf_rmsnorm")
    return y


def rope_append(qkv, cos, sin, positions, k_layer, v_layer, slot0, H, D, rotate_k=True, slot0_dev=None, Hkv=None):
    """Split fused qkv rows, rotate q (and k), append k/v rows to the cache at slot0+i.  Returns q (rows,H,D).
    ``Hkv`` < H: grouped-query rows [q: H D | k: Hkv D | v: Hkv D] (tf_rope_append_gqa)."""
    _dev(qkv, cos, sin, positions, k_layer, v_layer)
    rows = qkv.shape[0]
    if Hkv is not None and Hkv != H:
        assert qkv.dtype == _HALF and qkv.stride(1) == 1 and qkv.shape[1] == (H + 2 * Hkv) * D and H % Hkv == 0
        assert positions.dtype == torch.int64 and positions.numel() == rows and positions.is_contiguous()
        assert cos.dtype == _HALF and cos.is_contiguous() and cos.shape[1] == D
        st, sh = _kv(k_layer)
        assert _kv(v_layer) == (st, sh) and k_layer.shape[0] == Hkv and v_layer.shape[0] == Hkv
        q = torch.empty(rows, H, D, dtype=_HALF, device=qkv.device)
        hip.check(hip.lib().tf_rope_append_gqa(_ptr(qkv), qkv.stride(0), _ptr(cos), _ptr(sin), _ptr(positions), _ptr(q),
                                               _ptr(k_layer), _ptr(v_layer), st, sh, int(slot0), _ptr(slot0_dev), rows, H, Hkv,
                                               D, 1 if rotate_k else 0, _stream()), "tf_rope_append_gqa")
        return q
    assert qkv.dtype == _HALF and qkv.stride(1) == 1 and qkv.shape[1] == 3 * H * D
    assert positions.dtype == torch.int64 and positions.numel() == rows and positions.is_contiguous()
    assert cos.dtype == _HALF and cos.is_contiguous() and cos.shape[1] == D
    st, sh = _kv(k_layer)
    assert _kv(v_layer) == (st, sh)
    q = torch.empty(rows, H, D, dtype=_HALF, device=qkv.device)
    hip.check(hip.lib().tf_rope_append(_ptr(qkv), qkv.stride(0), _ptr(cos), _ptr(sin), _ptr(positions), _ptr(q),
                                       _ptr(k_layer), _ptr(v_layer), st, sh, int(slot0), _ptr(slot0_dev), rows, H, D,
                                       1 if rotate_k else 0, _stream()), "tf_rope_append")
    return q


def qk_norm_rope_append(qkv, qn, kn, eps, cos, sin, positions, k_layer, v_layer, slot0, H, D, rotate_k=True, slot0_dev=None,
                        Hkv=None):
    """rope_append for a QK-norm model: every q and k head of the fused rows [q: H D | k: Hkv D | v: Hkv D]
    goes through an RMSNorm over the head width (``qn`` / ``kn``: the [D] fp16 weights, ``eps``) before the rotation; k rows
    (rotated unless rotate_k is False) and the untouched v rows land in the cache at slot0+i.  Returns q (rows,H,D).
    One kernel, tf_qk_norm_rope_append, for decode blocks and prefill chunks, multi-head (Hkv None or H) and grouped-query."""
    _dev(qkv, qn, kn, cos, sin, positions, k_layer, v_layer, slot0_dev)
    Hkv = H if Hkv is None else Hkv
    rows = qkv.shape[0]
    assert qkv.dtype == _HALF and qkv.dim() == 2 and qkv.stride(1) == 1 and qkv.shape[1] == (H + 2 * Hkv) * D and H % Hkv == 0
    assert positions.dtype == torch.int64 and positions.numel() == rows and positions.is_contiguous()
    assert cos.dtype == _HALF and cos.is_contiguous() and cos.shape[1] == D and sin.shape == cos.shape and sin.is_contiguous()
    for w in (qn, kn):
        assert w.dtype == _HALF and tuple(w.shape) == (D,) and w.is_contiguous()
    st, sh = _kv(k_layer)
    assert _kv(v_layer) == (st, sh) and k_layer.shape[0] == Hkv and v_layer.shape[0] == Hkv
    q = torch.empty(rows, H, D, dtype=_HALF, device=qkv.device)
    hip.check(hip.lib().tf_qk_norm_rope_append(_ptr(qkv), qkv.stride(0), _ptr(cos), _ptr(sin), _ptr(positions), _ptr(q),
                                               _ptr(k_layer), _ptr(v_layer), st, sh, int(slot0), _ptr(slot0_dev), rows, H, Hkv,
                                               D, 1 if rotate_k else 0, _ptr(qn), _ptr(kn), float(eps), _stream()),
              "tf_qk_norm_rope_append")
    return q


def qk_norm_rope_ref(qkv, qn, kn, eps, cos, sin, positions, H, D, rotate_k=True, Hkv=None):
    """Host restatement of the QK NORM contract (include/triforce_hip.h) with its rounding points, on any device:
    -> (q (rows, H, D), k (rows, Hkv, D), v (rows, Hkv, D)) fp16 — what tf_qk_norm_rope_append writes to q_out and to the
    cache rows.  fp32 sum of squares (torch's order), inv = 1 / sqrt(ms + eps) in IEEE fp32, fp16 cast, fp16 weight multiply, then
    the fp16 rotation; each fp16 operation is an fp32 operation on fp16 values rounded once, as hmul_rn / hadd_rn are."""
    Hkv = H if Hkv is None else Hkv
    rows = qkv.shape[0]
    q = qkv[:, :H * D].reshape(rows, H, D)
    k = qkv[:, H * D:(H + Hkv) * D].reshape(rows, Hkv, D)
    v = qkv[:, (H + Hkv) * D:(H + 2 * Hkv) * D].reshape(rows, Hkv, D).clone()
    eps32 = torch.tensor(float(eps), dtype=torch.float32, device=qkv.device)

    def norm(x, w):
        f = x.float()
        ms = f.pow(2).sum(-1, keepdim=True) / float(D)
        # fp32 sqrt and divide, each correctly rounded: through float64 (exact for both by 53 >= 2 * 24 + 2), because torch's
        # vectorised fp32 sqrt on the CPU is not correctly rounded (0.65 % of random inputs are one ulp off)
        root = torch.sqrt((ms + eps32).double()).float()
        inv = (1.0 / root.double()).float()
        return (w.float() * (f * inv).to(_HALF).float()).to(_HALF)

    def rope(y):
        c, s = cos[positions].float()[:, None, :], sin[positions].float()[:, None, :]
        f = y.float()
        rot = torch.cat([-f[..., D // 2:], f[..., :D // 2]], dim=-1)
        return ((f * c).to(_HALF).float() + (rot * s).to(_HALF).float()).to(_HALF)

    qy, ky = norm(q, qn), norm(k, kn)
    return rope(qy), (rope(ky) if rotate_k else ky), v


def silu_mul(gate_up):
    _dev(gate_up)
    rows, two_i = gate_up.shape
    assert gate_up.dtype == _HALF and gate_up.is_contiguous()
    out = torch.empty(rows, two_i // 2, dtype=_HALF, device=gate_up.device)
    hip.check(hip.lib().tf_silu_mul(_ptr(gate_up), _ptr(out), rows, two_i // 2, _stream()), "tf_silu_mul")
    return out


def _workspace(device, floats):
    # per-call allocation from torch's caching allocator: no hipMalloc after warm-up, and inside a
    # hipGraph capture the block comes from the graph's private pool, so replays stay valid
    return torch.empty(int(floats), dtype=torch.float32, device=device)


# When set to a list, eager attn_decode calls append (start_event, end_event, sk, H, D): HIP events on the stream
# the kernel is launched on, used by bench.py for the live roofline figure.  Every ATTN_TIMER_EVERY-th call is
# timed: an event record is a queue packet of its own (~3 us of gap on each side of the kernel), so bracketing all
# 32 launches of a target verify would cost the step ~0.4 ms of the very time being measured.
ATTN_TIMER = None
ATTN_TIMER_EVERY = max(1, int(_os.environ.get("TRIFORCE_ATTN_TIMER_EVERY", "8")))
_attn_calls = 0


_NSPLIT_FORCE = int(_os.environ.get("TRIFORCE_ATTN_NSPLIT", "0"))      # A/B only (tools/tp_shard_bench.py): > 0 overrides the rule


@functools.lru_cache(maxsize=4096)
def _pick_nsplit(H, sk):
    if _NSPLIT_FORCE > 0:
        return max(1, min(_NSPLIT_FORCE, (int(sk) + 15) // 16))
    return hip.lib().tf_attn_decode_pick_nsplit(H, sk)


@functools.lru_cache(maxsize=4096)
def _ws_floats(H, sq, D, nsplit):
    return hip.lib().tf_attn_decode_ws_floats(H, sq, D, nsplit)


# Ticket words of the one-launch attention (tf_attn_decode_fused): per device one zeroed block, one 128-word row per
# stream that has launched attention (calls on one stream are ordered; two streams must not share a row).  Allocated
# at the first call, never freed; every launch leaves its row zero.
ATTN_FUSED_MERGE = _os.environ.get("TRIFORCE_ATTN_FUSED_MERGE", "1") != "0"
if _os.environ.get("TRIFORCE_ATTN_RENDEZVOUS", "0") == "1":     # A/B: > 8 splits on a small grid merged inside the launch
    hip.lib().tf_attn_tune(0, 1)
_TICKET_ROWS, _TICKET_WORDS = 64, 128
_tickets = {}


def _ticket_row(device, stream):
    dev = _tickets.get(device)
    if dev is None:
        dev = _tickets[device] = (torch.zeros(_TICKET_ROWS, _TICKET_WORDS, dtype=torch.int32, device=device), {})
    block, rows = dev
    row = rows.get(stream)
    if row is None:
        if len(rows) >= _TICKET_ROWS:
            return None                               # more streams than rows: the two-launch form is always valid
        row = rows[stream] = len(rows)
    return block[row]


def attn_decode(q, k_layer, v_layer, sk, scale, sk_dev=None, nsplit=None, packed=False):
    """flash_attn_with_kvcache(q, k, v, softmax_scale, causal=True) for sq<=32 rows (bottom-right causal).
    q (sq,H,D); returns (sq, H*D) fp16 — a row-major tensor, or with ``packed`` an Act (what o_proj then reads)."""
    _dev(q, k_layer, v_layer, sk_dev)
    sq, H, D = q.shape
    if k_layer.shape[0] != H:                          # fewer KV heads than query heads: the grouped-query kernel
        return attn_decode_gqa(q, k_layer, v_layer, sk, scale, sk_dev=sk_dev, nsplit=nsplit, packed=packed)
    assert q.dtype == _HALF and q.is_contiguous()
    st, sh = _kv(k_layer)
    assert _kv(v_layer) == (st, sh)
    L = hip.lib()
    if nsplit is None:
        nsplit = _pick_nsplit(H, int(sk))
    ws = _workspace(q.device, _ws_floats(H, sq, D, nsplit))
    out = Act.empty(sq, H * D, q.device) if packed else torch.empty(sq, H * D, dtype=_HALF, device=q.device)
    op, osm, osk = _lay(out)
    timed = False
    if ATTN_TIMER is not None and not torch.cuda.is_current_stream_capturing():
        global _attn_calls
        _attn_calls += 1
        timed = _attn_calls % ATTN_TIMER_EVERY == 0
    if timed:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    stream = _stream()
    tickets = _ticket_row(q.device, stream.value or 0) if ATTN_FUSED_MERGE and H <= _TICKET_WORDS else None
    hip.check(L.tf_attn_decode_act(_ptr(q), _ptr(k_layer), _ptr(v_layer), op, osm, osk, st, sh, sq, int(sk), _ptr(sk_dev),
                                   H, D, float(scale), nsplit, _ptr(ws), ws.numel(), _ptr(tickets), stream),
              "tf_attn_decode_act")
    if timed:
        ev1.record()
        ATTN_TIMER.append((ev0, ev1, int(sk), H, D))
    return out


def attn_decode_gqa(q, k_layer, v_layer, sk, scale, sk_dev=None, nsplit=None, packed=False, fused_merge=None, out=None):
    """attn_decode for grouped-query attention: q (sq, H, D) against KV views of Hkv = H / g heads, query
    head h reading KV head h // g.  The sq rows of gs query heads of one KV head are stacked into one gs * sq <= 32 row
    problem (gqa_stack), so K / V is streamed once per KV head whenever g * sq <= 32.  ``fused_merge``: None = the module
    default, True / False = the one- / two-launch form (bit-identical).  ``out``: write into this (sq, H * D) row-major
    tensor or Act instead of a fresh one.  Not timed into ATTN_TIMER."""
    _dev(q, k_layer, v_layer, sk_dev)
    sq, H, D = q.shape
    Hkv = k_layer.shape[0]
    assert q.dtype == _HALF and q.is_contiguous() and v_layer.shape[0] == Hkv
    if Hkv < 1 or H % Hkv or sq > SKINNY_MAX_ROWS:
        raise hip.TriforceHipError(f"attn_decode_gqa: {H} query heads over {Hkv} KV heads, {sq} rows")
    st, sh = _kv(k_layer)
    assert _kv(v_layer) == (st, sh)
    gs, sub = gqa_stack(H // Hkv, sq)
    cols = Hkv * sub                                   # workgroup columns = (KV head, sub-group) pairs
    if nsplit is None:
        nsplit = _pick_nsplit(cols, int(sk))
    ws = _workspace(q.device, _ws_floats(cols, gs * sq, D, nsplit))
    if out is None:
        out = Act.empty(sq, H * D, q.device) if packed else torch.empty(sq, H * D, dtype=_HALF, device=q.device)
    assert tuple(out.shape) == (sq, H * D)
    op, osm, osk = _lay(out)
    stream = _stream()
    fused = ATTN_FUSED_MERGE if fused_merge is None else fused_merge
    tickets = _ticket_row(q.device, stream.value or 0) if fused and cols <= _TICKET_WORDS else None
    hip.check(hip.lib().tf_attn_decode_gqa_act(_ptr(q), _ptr(k_layer), _ptr(v_layer), op, osm, osk, st, sh, sq, int(sk),
                                               _ptr(sk_dev), H, Hkv, D, float(scale), nsplit, _ptr(ws), ws.numel(),
                                               _ptr(tickets), stream), "tf_attn_decode_gqa_act")
    return out


# ---- FP8 KV cache (TRIFORCE_KV_CACHE=fp8; include/triforce_hip.h "FP8 KV CACHE") -------------------------
KV_FP8_EMIN, KV_FP8_EMAX = -15, 7


def kv_quantize_ref(x):
    """Host restatement of the FP8 KV contract: x (..., D) fp16 rows -> (codes float8_e4m3fn, exponent bytes uint8 = e + 127,
    deq fp16).  e = the smallest integer with 448 * 2^e >= max |x| of the row, clamped to [-15, 7]."""
    a = x.float().abs().amax(dim=-1)
    e = torch.full(a.shape, KV_FP8_EMIN, dtype=torch.int32, device=x.device)
    for k in range(KV_FP8_EMIN, KV_FP8_EMAX):                  # the predicate falls as k grows: count the k that fail it
        e += (448.0 * 2.0 ** k < a).to(torch.int32)
    p = torch.pow(torch.tensor(2.0, device=x.device), e.float()).unsqueeze(-1)
    codes = (x.float() / p).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)     # x / 2^e = x * 2^-e exactly
    deq = (codes.float() * p).to(_HALF)
    return codes, (e + 127).to(torch.uint8), deq


def _f8_kv(t):
    assert t.dim() == 3 and t.stride(2) == 1 and t.dtype == torch.float8_e4m3fn, "FP8 KV layer view must be (H,T,D) e4m3fn"
    return t.stride(1), t.stride(0)


def _f8_exp(t):
    assert t.dim() == 2 and t.stride(1) == 1 and t.dtype == torch.uint8, "exponent view must be (H,T) uint8"
    return t.stride(0)


def kv_quant_rows(k_rows, v_rows, k_codes, v_codes, k_exp, v_exp, slot0, slot0_dev=None, deq=False):
    """Quantize n fresh rows (k_rows / v_rows: (H,n,D) fp16 views) into an FP8 cache layer (codes (H,T,D), exponents (H,T))
    at token slot0 (or the device scalar slot0_dev); deq=True writes the dequantized values back over the input rows."""
    _dev(k_rows, v_rows, k_codes, v_codes, k_exp, v_exp, slot0_dev)
    H, n, D = k_rows.shape
    ist, ish = _kv(k_rows)
    assert _kv(v_rows) == (ist, ish) and v_rows.shape == k_rows.shape
    cst, csh = _f8_kv(k_codes)
    assert _f8_kv(v_codes) == (cst, csh) and k_codes.shape[0] == H and k_codes.shape[2] == D
    esh = _f8_exp(k_exp)
    assert _f8_exp(v_exp) == esh
    if slot0_dev is None and (slot0 < 0 or slot0 + n > k_codes.shape[1]):
        raise IndexError(f"kv_quant_rows: rows [{slot0}, {slot0 + n}) leave the {k_codes.shape[1]}-row cache")
    hip.check(hip.lib().tf_kv_quant_rows(_ptr(k_rows), _ptr(v_rows), ist, ish, _ptr(k_codes), _ptr(v_codes), _ptr(k_exp),
                                         _ptr(v_exp), cst, csh, esh, int(slot0), _ptr(slot0_dev), n, H, D,
                                         _ptr(k_rows) if deq else None, _ptr(v_rows) if deq else None, _stream()),
              "tf_kv_quant_rows")


def attn_decode_fp8(q, k_codes, v_codes, k_exp, v_exp, sk, scale, sk_dev=None, nsplit=None, packed=False):
    """attn_decode over an FP8 cache layer: bit-identical to attn_decode on the dequantized K / V for the same nsplit.
    Not timed into ATTN_TIMER (bench.py's roofline divides fp16 bytes by the kernel time)."""
    _dev(q, k_codes, v_codes, k_exp, v_exp, sk_dev)
    sq, H, D = q.shape
    assert q.dtype == _HALF and q.is_contiguous()
    st, sh = _f8_kv(k_codes)
    assert _f8_kv(v_codes) == (st, sh)
    esh = _f8_exp(k_exp)
    assert _f8_exp(v_exp) == esh
    if nsplit is None:
        nsplit = _pick_nsplit(H, int(sk))
    ws = _workspace(q.device, _ws_floats(H, sq, D, nsplit))
    out = Act.empty(sq, H * D, q.device) if packed else torch.empty(sq, H * D, dtype=_HALF, device=q.device)
    op, osm, osk = _lay(out)
    stream = _stream()
    tickets = _ticket_row(q.device, stream.value or 0) if ATTN_FUSED_MERGE and H <= _TICKET_WORDS else None
    hip.check(hip.lib().tf_attn_decode_fp8_act(_ptr(q), _ptr(k_codes), _ptr(v_codes), _ptr(k_exp), _ptr(v_exp), op, osm, osk,
                                               st, sh, esh, sq, int(sk), _ptr(sk_dev), H, D, float(scale), nsplit, _ptr(ws),
                                               ws.numel(), _ptr(tickets), stream), "tf_attn_decode_fp8_act")
    return out


def kv_dequant_rows_pair(src_k, src_v, exp_k, exp_v, dst_k, dst_v, src_t0, dst_t0, n):
    """dst[l,h,dst_t0+i] = deq(src[l,h,src_t0+i]) for K and V in one launch: src (L,H,T,D) e4m3fn views, exp (L,H,T) uint8
    views (token stride 1), dst (L,H,T',D) fp16 views."""
    if n <= 0:
        return
    _dev(src_k, src_v, exp_k, exp_v, dst_k, dst_v)
    L, H, _, D = src_k.shape
    for t in (src_k, src_v):
        assert t.dim() == 4 and t.stride(3) == 1 and t.dtype == torch.float8_e4m3fn
    assert src_k.stride() == src_v.stride() and src_k.shape == src_v.shape
    for t in (exp_k, exp_v):
        assert t.dim() == 3 and t.stride(2) == 1 and t.dtype == torch.uint8 and t.shape[:2] == (L, H)
    assert exp_k.stride() == exp_v.stride()
    assert dst_k.shape[0] == L and dst_k.shape[1] == H and dst_k.shape[3] == D and _lhtd(dst_k) == _lhtd(dst_v)
    if src_t0 < 0 or dst_t0 < 0 or src_t0 + n > src_k.shape[2] or dst_t0 + n > dst_k.shape[2]:
        raise IndexError(f"kv_dequant_rows_pair: rows [{src_t0}, {src_t0 + n}) of {src_k.shape[2]} -> [{dst_t0}, {dst_t0 + n}) "
                         f"of {dst_k.shape[2]} leave the cache (the kernel does not bounds-check)")
    dsl, dst_t, dsh = _lhtd(dst_k)
    hip.check(hip.lib().tf_kv_dequant_rows_pair(_ptr(src_k), _ptr(src_v), src_k.stride(0), src_k.stride(2), src_k.stride(1),
                                                _ptr(exp_k), _ptr(exp_v), exp_k.stride(0), exp_k.stride(1), _ptr(dst_k),
                                                _ptr(dst_v), dsl, dst_t, dsh, int(src_t0), int(dst_t0), int(n), L, H, D,
                                                _stream()), "tf_kv_dequant_rows_pair")


# ---- FP8 retrieval cache (TRIFORCE_RETRIEVAL_KV=fp8; include/triforce_hip.h "FP8 RETRIEVAL CACHE") --------
def attn_decode_fp8_tail(q, k_codes, v_codes, k_exp, v_exp, k_tail, v_tail, sk_codes, scale, n_tail=None, nsplit=None,
                         packed=False):
    """attn_decode over keys [0, sk_codes) of an FP8 layer (codes (H,T,D), exponents (H,T)) followed by the first n_tail rows
    (default: all) of the fp16 views k_tail / v_tail (H,n,D), in one launch: bit-identical to attn_decode on
    [deq(codes) | tail rows] for the same nsplit."""
    _dev(q, k_codes, v_codes, k_exp, v_exp, k_tail, v_tail)
    sq, H, D = q.shape
    assert q.dtype == _HALF and q.is_contiguous()
    st, sh = _f8_kv(k_codes)
    assert _f8_kv(v_codes) == (st, sh)
    esh = _f8_exp(k_exp)
    assert _f8_exp(v_exp) == esh
    tst, tsh = _kv(k_tail)
    assert _kv(v_tail) == (tst, tsh) and k_tail.shape == v_tail.shape and k_tail.shape[0] == H
    n_tail = k_tail.shape[1] if n_tail is None else int(n_tail)
    if not (1 <= sk_codes <= k_codes.shape[1] and sk_codes <= k_exp.shape[1] and 1 <= n_tail <= k_tail.shape[1]):
        raise IndexError(f"attn_decode_fp8_tail: {sk_codes} coded keys of {k_codes.shape[1]}, {n_tail} tail rows of "
                         f"{k_tail.shape[1]} (the kernel does not bounds-check)")
    if nsplit is None:
        nsplit = _pick_nsplit(H, int(sk_codes) + n_tail)
    ws = _workspace(q.device, _ws_floats(H, sq, D, nsplit))
    out = Act.empty(sq, H * D, q.device) if packed else torch.empty(sq, H * D, dtype=_HALF, device=q.device)
    op, osm, osk = _lay(out)
    stream = _stream()
    tickets = _ticket_row(q.device, stream.value or 0) if ATTN_FUSED_MERGE and H <= _TICKET_WORDS else None
    hip.check(hip.lib().tf_attn_decode_fp8_tail_act(_ptr(q), _ptr(k_codes), _ptr(v_codes), _ptr(k_exp), _ptr(v_exp), _ptr(k_tail),
                                                    _ptr(v_tail), op, osm, osk, st, sh, esh, tst, tsh, sq, int(sk_codes), n_tail,
                                                    None, H, D, float(scale), nsplit, _ptr(ws), ws.numel(), _ptr(tickets),
                                                    stream), "tf_attn_decode_fp8_tail_act")
    return out


def retrieval_gather_fp8_ref(k_src, v_src, idx, chunk):
    """Host restatement of retrieval_gather_fp8 from fp16 rows: (k codes, v codes, k exponents, v exponents) of the gathered
    rows, (H, sets * chunk, D) and (H, sets * chunk) — kv_quantize_ref of the rows retrieval_gather would copy."""
    rows = (idx.long().unsqueeze(-1) * chunk + torch.arange(chunk, device=idx.device)).reshape(idx.shape[0], -1)   # (H, sets * chunk)
    pick = rows.unsqueeze(-1).expand(-1, -1, k_src.shape[2])
    kc, ke, _ = kv_quantize_ref(torch.gather(k_src, 1, pick))
    vc, ve, _ = kv_quantize_ref(torch.gather(v_src, 1, pick))
    return kc, vc, ke, ve


def retrieval_gather_fp8(k_src, v_src, idx, k_codes, v_codes, k_exp, v_exp, chunk, src_exp=None):
    """retrieval_gather into an FP8 layer (codes (H,T,D), exponents (H,T)), K and V in one launch.  k_src / v_src: (H,T',D) fp16
    views, quantized (bit-identical to retrieval_gather_fp8_ref); or with src_exp = (k exponents, v exponents) the e4m3fn
    codes of an FP8 layer, copied with their exponent bytes."""
    _dev(k_src, v_src, idx, k_codes, v_codes, k_exp, v_exp)
    H, T, D = k_src.shape
    if src_exp is None:
        sst, ssh = _kv(k_src)
        assert _kv(v_src) == (sst, ssh)
        sek = sev = None
        sesh = 0
    else:
        sst, ssh = _f8_kv(k_src)
        assert _f8_kv(v_src) == (sst, ssh)
        sek, sev = src_exp
        _dev(sek, sev)
        sesh = _f8_exp(sek)
        assert _f8_exp(sev) == sesh and sek.shape[1] >= T
    cst, csh = _f8_kv(k_codes)
    assert _f8_kv(v_codes) == (cst, csh) and k_codes.shape[0] == H and k_codes.shape[2] == D
    esh = _f8_exp(k_exp)
    assert _f8_exp(v_exp) == esh
    assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.shape[0] == H
    sets = idx.shape[1]
    if sets * chunk > k_codes.shape[1] or sets * chunk > k_exp.shape[1]:
        raise IndexError(f"retrieval_gather_fp8: {sets} chunks of {chunk} rows leave the {k_codes.shape[1]}-row cache")
    hip.check(hip.lib().tf_retrieval_gather_fp8(_ptr(k_src), _ptr(v_src), sst, ssh, _ptr(sek), _ptr(sev), sesh, _ptr(idx),
                                                _ptr(k_codes), _ptr(v_codes), _ptr(k_exp), _ptr(v_exp), cst, csh, esh, sets,
                                                int(chunk), H, D, _stream()), "tf_retrieval_gather_fp8")


def _lht_exp(t):
    assert t.dim() == 3 and t.stride(2) == 1 and t.dtype == torch.uint8, "(L,H,T) uint8 exponents expected"
    return t.stride(0), t.stride(1)                  # stride_l, stride_h


def _lhtd_f8(t):
    assert t.dim() == 4 and t.stride(3) == 1 and t.dtype == torch.float8_e4m3fn, "(L,H,T,D) e4m3fn expected"
    return t.stride(0), t.stride(2), t.stride(1)     # stride_l, stride_t, stride_h


class KvQuantPairPlan:
    """Rows of K and V into an FP8 cache over fixed tensors, all layers in one launch: dst codes (L,H,T,D) / exponents
    (L,H,T) rows [dst_t0, dst_t0 + n) = src rows [src_t0, src_t0 + n).  src_k / src_v: (L,H,T',D) fp16 views (quantized by the
    FP8 KV contract), or with ``src_exp`` = (k exponents, v exponents) e4m3fn codes (copied with their exponent bytes)."""

    def __init__(self, src_k, src_v, dst_kc, dst_vc, dst_ke, dst_ve, src_exp=None):
        _dev(src_k, src_v, dst_kc, dst_vc, dst_ke, dst_ve)
        L, H, _, D = src_k.shape
        assert src_k.shape == src_v.shape and dst_kc.shape == dst_vc.shape and dst_ke.shape == dst_ve.shape
        assert dst_kc.shape[0] == L and dst_kc.shape[1] == H and dst_kc.shape[3] == D and dst_ke.shape[:2] == (L, H)
        if src_exp is None:
            src = _lhtd(src_k)
            assert _lhtd(src_v) == src
            exp = (None, None, 0, 0)
            self.src_rows = src_k.shape[2]
        else:
            src = _lhtd_f8(src_k)
            assert _lhtd_f8(src_v) == src
            sek, sev = src_exp
            _dev(sek, sev)
            assert _lht_exp(sek) == _lht_exp(sev) and sek.shape[:2] == (L, H) and sev.shape == sek.shape
            exp = (_ptr(sek), _ptr(sev)) + _lht_exp(sek)
            self.src_rows = min(src_k.shape[2], sek.shape[2])
        dst = _lhtd_f8(dst_kc)
        assert _lhtd_f8(dst_vc) == dst and _lht_exp(dst_ke) == _lht_exp(dst_ve)
        self.keep = (src_k, src_v, dst_kc, dst_vc, dst_ke, dst_ve, src_exp)
        self.dst_rows = min(dst_kc.shape[2], dst_ke.shape[2])
        self.head = (_ptr(src_k), _ptr(src_v)) + src + exp + (_ptr(dst_kc), _ptr(dst_vc)) + dst \
            + (_ptr(dst_ke), _ptr(dst_ve)) + _lht_exp(dst_ke)
        self.dims = (L, H, D)
        self.fn = hip.lib().tf_kv_quant_rows_pair

    def __call__(self, src_t0, dst_t0, n):
        if n <= 0:
            return
        if src_t0 < 0 or dst_t0 < 0 or src_t0 + n > self.src_rows or dst_t0 + n > self.dst_rows:
            raise IndexError(f"kv_quant_rows_pair: rows [{src_t0}, {src_t0 + n}) of {self.src_rows} -> [{dst_t0}, {dst_t0 + n}) of "
                             f"{self.dst_rows} leave the cache (the kernel does not bounds-check)")
        hip.check(self.fn(*self.head, int(src_t0), int(dst_t0), int(n), *self.dims, _stream()), "tf_kv_quant_rows_pair")


def kv_quant_rows_pair(src_k, src_v, dst_kc, dst_vc, dst_ke, dst_ve, src_t0, dst_t0, n, src_exp=None):
    """One call of a KvQuantPairPlan over these tensors (the tensors are validated on every call)."""
    if n <= 0:
        return
    KvQuantPairPlan(src_k, src_v, dst_kc, dst_vc, dst_ke, dst_ve, src_exp)(src_t0, dst_t0, n)


def attn_block(q, k_layer, v_layer, sk, scale, nsplit=None, tree_mask=None, mask_row0=0, tree_start=0):
    """Attention of a block of <=128 query rows in one pass over the keys.  tree_mask None: bottom-right causal
    (a prefill chunk).  tree_mask (n_rows, words) int32 bit rows: Sequoia tree attention — keys [0, tree_start)
    visible to all rows, key tree_start+j visible to row i iff bit j of tree_mask[mask_row0+i] is set."""
    _dev(q, k_layer, v_layer, tree_mask)
    sq, H, D = q.shape
    assert q.dtype == _HALF and q.is_contiguous() and sq <= 128
    st, sh = _kv(k_layer)
    assert _kv(v_layer) == (st, sh)
    L = hip.lib()
    if nsplit is None:
        nsplit = L.tf_attn_block_pick_nsplit(H, sq, int(sk))
    ws = _workspace(q.device, L.tf_attn_block_ws_floats(H, D, nsplit))
    out = torch.empty(sq, H * D, dtype=_HALF, device=q.device)
    words = 0
    if tree_mask is not None:
        assert tree_mask.dtype == torch.int32 and tree_mask.dim() == 2 and tree_mask.is_contiguous()
        assert mask_row0 + sq <= tree_mask.shape[0]
        words = tree_mask.shape[1]
    hip.check(L.tf_attn_block(_ptr(q), _ptr(k_layer), _ptr(v_layer), _ptr(out), st, sh, sq, int(sk), H, D, float(scale),
                              nsplit, _ptr(ws), ws.numel(), _ptr(tree_mask), words, int(mask_row0), int(tree_start),
                              _stream()), "tf_attn_block")
    return out


def attn_tree(q, k_layer, v_layer, sk, scale, tree_mask, tree_start, mask_row0=0):
    """Tree attention for any number of query rows (<=128 per pass)."""
    sq = q.shape[0]
    if sq <= 128:
        return attn_block(q, k_layer, v_layer, sk, scale, tree_mask=tree_mask, mask_row0=mask_row0, tree_start=tree_start)
    outs = []
    for r0 in range(0, sq, 128):
        r1 = min(sq, r0 + 128)
        outs.append(attn_block(q[r0:r1].contiguous(), k_layer, v_layer, sk, scale, tree_mask=tree_mask,
                               mask_row0=mask_row0 + r0, tree_start=tree_start))
    return torch.cat(outs, dim=0)


def pack_tree_mask(visible):
    """(rows, T) bool/0-1 tensor -> (rows, ceil(T/32)) int32 bit rows (bit j%32 of word j//32 = column j)."""
    rows, T = visible.shape
    words = (T + 31) // 32
    v = torch.zeros(rows, words * 32, dtype=torch.int64, device=visible.device)
    v[:, :T] = (visible != 0).to(torch.int64)
    w = (v.view(rows, words, 32) << torch.arange(32, device=visible.device, dtype=torch.int64)).sum(dim=-1)
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w)            # two's-complement into int32
    return w.to(torch.int32).contiguous()


# 0: a prefill chunk's attention as one tf_attn_block launch per 128 rows (A/B; default: tf_attn_prefill, one launch)
ATTN_PREFILL_ONE_LAUNCH = _os.environ.get("TRIFORCE_PREFILL_ONE_LAUNCH", "1") != "0"


def attn_prefill(q, k_layer, v_layer, sk, scale):
    """Causal attention for a prefill block of any length: <=32 rows use the decode kernel, longer blocks are cut
    (up to 4096 rows) go to tf_attn_prefill: the 128-row blocks of the chunk, block j seeing keys
    [0, sk - sq + end_j), run in one launch and share the KV stream through L2."""
    sq = q.shape[0]
    if sq <= 32:
        return attn_decode(q, k_layer, v_layer, sk, scale)
    if k_layer.shape[0] != q.shape[1]:                 # grouped-query: every block above 32 rows, 33..128 included
        return attn_prefill_gqa(q, k_layer, v_layer, sk, scale)
    if sq <= 128:
        return attn_block(q, k_layer, v_layer, sk, scale)
    if not ATTN_PREFILL_ONE_LAUNCH or sq > 4096:
        outs = []
        for r0 in range(0, sq, 128):
            r1 = min(sq, r0 + 128)
            outs.append(attn_block(q[r0:r1].contiguous(), k_layer, v_layer, sk - (sq - r1), scale))
        return torch.cat(outs, dim=0)
    _dev(q, k_layer, v_layer)
    _, H, D = q.shape
    assert q.dtype == _HALF and q.is_contiguous()
    st, sh = _kv(k_layer)
    assert _kv(v_layer) == (st, sh)
    L = hip.lib()
    nsplit = L.tf_attn_prefill_pick_nsplit(H, sq, int(sk))
    ws = _workspace(q.device, L.tf_attn_prefill_ws_floats(H, sq, D, nsplit))
    out = torch.empty(sq, H * D, dtype=_HALF, device=q.device)
    hip.check(L.tf_attn_prefill(_ptr(q), _ptr(k_layer), _ptr(v_layer), _ptr(out), st, sh, sq, int(sk), H, D, float(scale),
                                nsplit, _ptr(ws), ws.numel(), _stream()), "tf_attn_prefill")
    return out


def attn_prefill_gqa(q, k_layer, v_layer, sk, scale):
    """Causal attention of a prefill block of 33..4096 rows for grouped-query attention (tf_attn_prefill_gqa): tf_attn_prefill
    with query head h reading KV head h // g.  Longer blocks are cut into 4096-row pieces."""
    _dev(q, k_layer, v_layer)
    sq, H, D = q.shape
    Hkv = k_layer.shape[0]
    if not ATTN_PREFILL_ONE_LAUNCH:
        raise ValueError("TRIFORCE_PREFILL_ONE_LAUNCH=0 is not supported with a GQA model: the per-block kernel "
                         "(tf_attn_block) has one head count")
    if Hkv < 1 or H % Hkv:
        raise hip.TriforceHipError(f"attn_prefill_gqa: {H} query heads over {Hkv} KV heads")
    if sq > 4096:
        outs = []
        for r0 in range(0, sq, 4096):
            r1 = min(sq, r0 + 4096)
            outs.append(attn_prefill_gqa(q[r0:r1].contiguous(), k_layer, v_layer, sk - (sq - r1), scale))
        return torch.cat(outs, dim=0)
    assert q.dtype == _HALF and q.is_contiguous() and v_layer.shape[0] == Hkv
    st, sh = _kv(k_layer)
    assert _kv(v_layer) == (st, sh)
    L = hip.lib()
    nsplit = L.tf_attn_prefill_pick_nsplit(H, sq, int(sk))
    ws = _workspace(q.device, L.tf_attn_prefill_ws_floats(H, sq, D, nsplit))
    out = torch.empty(sq, H * D, dtype=_HALF, device=q.device)
    hip.check(L.tf_attn_prefill_gqa(_ptr(q), _ptr(k_layer), _ptr(v_layer), _ptr(out), st, sh, sq, int(sk), H, Hkv, D,
                                    float(scale), nsplit, _ptr(ws), ws.numel(), _stream()), "tf_attn_prefill_gqa")
    return out


def draft_model_struct(embed, ln1, wqkv, wo, ln2, wgu, wd, norm, lm_head, cos, sin, H, D, eps, scale):
    """TfDraftModel for tf_draft_forward_68m from the draft's weights (PackedLinear lists); None when a weight is not
    packed for the fused kernels (CPU tensors, odd shapes).  The struct holds raw pointers: keep the tensors alive."""
    L = len(wqkv)
    ws = list(wqkv) + list(wo) + list(wgu) + list(wd) + [lm_head]
    if L > hip.TF_DRAFT_MAX_LAYERS or D != 64 or not all(isinstance(w, PackedLinear) and w.parts is not None for w in ws):
        return None
    if any(w.wp_rope is None for w in wqkv) or any(w.split != 2 for w in wgu) or not embed.is_cuda:
        return None
    m = hip.TfDraftModel()
    m.embed = embed.data_ptr()
    for i in range(L):
        m.ln1[i], m.ln2[i] = ln1[i].data_ptr(), ln2[i].data_ptr()
        m.wqkv[i], m.wo[i], m.wdown[i] = wqkv[i].wp_rope.data_ptr(), wo[i].wp.data_ptr(), wd[i].wp.data_ptr()
        m.wgate[i], m.wup[i] = wgu[i].parts[0].data_ptr(), wgu[i].parts[1].data_ptr()
    m.norm, m.lm_head, m.cos, m.sin = norm.data_ptr(), lm_head.wp.data_ptr(), cos.data_ptr(), sin.data_ptr()
    m.layers, m.hidden, m.heads, m.head_dim = L, embed.shape[1], H, D
    m.inter, m.vocab, m.eps, m.scale = wgu[0].N // 2, lm_head.N, float(eps), float(scale)
    return m


def draft_cache_struct(cache, L):
    """TfDraftCache over the per-layer K / V views of a StreamingLLM cache."""
    c = hip.TfDraftCache()
    st = sh = None
    for i in range(L):
        kl, vl = cache.layer_kv(i)
        _dev(kl, vl)
        assert _kv(vl) == _kv(kl) and (st is None or (st, sh) == _kv(kl))
        st, sh = _kv(kl)
        c.k[i], c.v[i] = kl.data_ptr(), vl.data_ptr()
    c.stride_t, c.stride_h = st, sh
    return c


class DraftPersist:
    """Device state of the one-launch draft forward (tf_draft_forward_68m_persist): the control block (arrival counters,
    launch epoch, sticky error word, top-p scratch) and the activation workspace, both owned by ONE draft model — its
    launches are stream-ordered (eager calls and graph replays of one engine).  ``mirror``: a pinned host word that
    receives the error code without a device read (None until ``enable_mirror``)."""

    def __init__(self, model, device):
        L = hip.lib()
        self.device = torch.device(device)
        self.ctl = torch.zeros(int(L.tf_draft_persist_ctl_bytes()), dtype=torch.uint8, device=self.device)
        self.ws = torch.empty(int(L.tf_draft_persist_ws_bytes(ctypes.byref(model))), dtype=torch.uint8, device=self.device)
        self.mirror = None
        assert self.ctl.data_ptr() % 64 == 0 and self.ws.data_ptr() % 256 == 0
        self.enable_mirror()

    def check(self):
        """Raise if a launch on this control block has timed out (its outputs are NaN from then on): one plain host load."""
        if self.mirror is not None and int(self.mirror[0]) != 0:
            raise hip.TriforceHipError(f"one-launch draft forward: wait on edge {int(self.mirror[0]) - 1} timed out "
                                       "(a workgroup never became resident, or an arrival was lost); outputs are NaN until "
                                       "DraftPersist.reset()")

    def enable_mirror(self):
        if self.mirror is None:
            self.mirror = torch.zeros(1, dtype=torch.int32).pin_memory()
            hip.check(hip.lib().tf_draft_persist_reset(_ptr(self.ctl), self.mirror.data_ptr(), 1), "tf_draft_persist_reset")
        return self.mirror

    def error(self):
        """0, or 1 + the index of the edge whose wait timed out (sticky).  Reads the pinned mirror when there is one (no device
        synchronisation), else the control block (blocking)."""
        if self.mirror is not None:
            return int(self.mirror[0])
        return int(hip.lib().tf_draft_persist_error(_ptr(self.ctl)))

    def reset(self):
        hip.check(hip.lib().tf_draft_persist_reset(_ptr(self.ctl), None, 0), "tf_draft_persist_reset")


DRAFT_PERSIST = _os.environ.get("TRIFORCE_DRAFT_PERSIST", "1") != "0"


def draft_persist_supported(model, n, kv_len):
    return hip.lib().tf_draft_persist_supported(ctypes.byref(model), int(n), int(kv_len)) == 0


def draft_forward(model, cache, ids, slot0, kv_len, probs=None, persist=None):
    """tf_draft_forward_68m: ids (n,) int64 -> fp32 logits (n, vocab) [and the top-p probability row of the last token
    when ``probs`` = (temperature, top_p)] in one native call — ONE launch (tf_draft_forward_68m_persist) when ``persist``
    (a DraftPersist) is given and the shape is one it takes, else the 13-launch chain; the two are bit-identical."""
    _dev(ids)
    n = ids.numel()
    assert ids.dtype == torch.int64 and ids.is_contiguous() and 1 <= n <= SKINNY_MAX_ROWS
    L = hip.lib()
    logits = torch.empty(n, model.vocab, dtype=torch.float32, device=ids.device)
    p = torch.empty(model.vocab, dtype=torch.float32, device=ids.device) if probs is not None else None
    T, top_p = probs if probs is not None else (1.0, 1.0)
    if persist is not None and DRAFT_PERSIST and draft_persist_supported(model, n, kv_len):
        hip.check(L.tf_draft_forward_68m_persist(ctypes.byref(model), ctypes.byref(cache), _ptr(ids), n, int(slot0),
                                                 int(kv_len), _ptr(logits), _ptr(p), float(T), float(top_p),
                                                 _ptr(persist.ws), persist.ws.numel(), _ptr(persist.ctl), _stream()),
                  "tf_draft_forward_68m_persist")
        return logits, p
    nbytes = L.tf_draft_forward_ws_bytes(ctypes.byref(model), n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=ids.device)
    hip.check(L.tf_draft_forward_68m(ctypes.byref(model), ctypes.byref(cache), _ptr(ids), n, int(slot0), int(kv_len),
                                     _ptr(logits), _ptr(p), float(T), float(top_p), _ptr(ws), nbytes, _stream()),
              "tf_draft_forward_68m")
    return logits, p


def attn_rope_on_read(q, k_layer, v_layer, cos, sin, kv_len, scale):
    """Draft attention: cached keys are un-rotated and rotated on read with positions 0..kv_len-1."""
    _dev(q, k_layer, v_layer, cos, sin)
    sq, H, D = q.shape
    assert q.dtype == _HALF and q.is_contiguous()
    st, sh = _kv(k_layer)
    assert _kv(v_layer) == (st, sh)
    out = torch.empty(sq, H * D, dtype=_HALF, device=q.device)
    hip.check(hip.lib().tf_attn_rope_on_read(_ptr(q), _ptr(k_layer), _ptr(v_layer), _ptr(cos), _ptr(sin), _ptr(out),
                                             st, sh, sq, int(kv_len), H, D, float(scale), _stream()),
              "tf_attn_rope_on_read")
    return out


def retrieval_score(k_layer, q, chunks, chunk):
    """(H, chunks) fp16 un-scaled scores q . mean(K chunk)."""
    _dev(k_layer, q)
    H, T, D = k_layer.shape
    st, sh = _kv(k_layer)
    assert q.shape == (H, D) and q.dtype == _HALF and q.is_contiguous() and chunks * chunk <= T
    scores = torch.empty(H, chunks, dtype=_HALF, device=q.device)
    hip.check(hip.lib().tf_retrieval_score(_ptr(k_layer), st, sh, _ptr(q), _ptr(scores), chunks, chunk, H, D,
                                           _stream()), "tf_retrieval_score")
    return scores


def _index_layer(index_layer, H, D):
    assert index_layer.dim() == 3 and index_layer.shape[0] == H and index_layer.shape[2] == D and index_layer.dtype == _HALF \
        and index_layer.stride(2) == 1 and index_layer.stride(1) == D, "(H, Cmax, D) fp16 index layer expected"
    return index_layer.stride(0)


def chunk_mean(k_layer, index_layer, c0, c1, chunk):
    """index_layer[h, c] = fp16 mean of rows [c * chunk, (c + 1) * chunk) of k_layer[h] for c in [c0, c1): the chunk means
    retrieval_score forms, kept (the chunk-mean index).  Other chunks are not written."""
    _dev(k_layer, index_layer)
    H, T, D = k_layer.shape
    st, sh = _kv(k_layer)
    ish = _index_layer(index_layer, H, D)
    if not 0 <= c0 <= c1 or c1 > index_layer.shape[1] or c1 * chunk > T:
        raise IndexError(f"chunk_mean: chunks [{c0}, {c1}) of {chunk} rows leave the {index_layer.shape[1]}-chunk index or "
                         f"the {T}-row cache (the kernel does not bounds-check)")
    hip.check(hip.lib().tf_chunk_mean(_ptr(k_layer), st, sh, _ptr(index_layer), ish, int(c0), int(c1), int(chunk), H, D,
                                      _stream()), "tf_chunk_mean")


def retrieval_score_indexed(index_layer, q, chunks):
    """(H, chunks) fp16 scores from the chunk-mean index: bit-identical to retrieval_score over the K it was built from."""
    _dev(index_layer, q)
    H, Cmax, D = index_layer.shape
    ish = _index_layer(index_layer, H, D)
    assert q.shape == (H, D) and q.dtype == _HALF and q.is_contiguous()
    if not 1 <= chunks <= Cmax:
        raise IndexError(f"retrieval_score_indexed: {chunks} chunks of a {Cmax}-chunk index")
    scores = torch.empty(H, chunks, dtype=_HALF, device=q.device)
    hip.check(hip.lib().tf_retrieval_score_indexed(_ptr(index_layer), ish, _ptr(q), _ptr(scores), int(chunks), H, D,
                                                   _stream()), "tf_retrieval_score_indexed")
    return scores


def retrieval_topk(scores, sets):
    """(H, sets) int32: chunk 0 first, then the sets-1 best of [1,C), descending, ties -> lowest chunk.
    The order is the fp16 BIT-PATTERN order (sign-magnitude): -0 below +0, +NaN first (above +inf).  "Ties" are equal bit
    patterns: a (+0, -0) pair is not a tie - unlike IEEE equality, and equally admissible against torch.topk, whose order
    among equal scores is unspecified."""
    _dev(scores)
    H, C = scores.shape
    assert scores.dtype == _HALF and scores.is_contiguous()
    idx = torch.empty(H, sets, dtype=torch.int32, device=scores.device)
    hip.check(hip.lib().tf_retrieval_topk(_ptr(scores), _ptr(idx), C, sets, H, _stream()), "tf_retrieval_topk")
    return idx


def retrieval_gather(k_src, v_src, idx, k_dst, v_dst, chunk):
    _dev(k_src, v_src, idx, k_dst, v_dst)
    H, _, D = k_src.shape
    sst, ssh = _kv(k_src)
    assert _kv(v_src) == (sst, ssh)
    dst_t, dsh = _kv(k_dst)
    assert _kv(v_dst) == (dst_t, dsh)
    assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.shape[0] == H
    hip.check(hip.lib().tf_retrieval_gather(_ptr(k_src), _ptr(v_src), sst, ssh, _ptr(idx), _ptr(k_dst), _ptr(v_dst),
                                            dst_t, dsh, idx.shape[1], chunk, H, D, _stream()), "tf_retrieval_gather")


def _lhtd(t):
    assert t.dim() == 4 and t.stride(3) == 1 and t.dtype == _HALF, "(L,H,T,D) fp16 expected"
    return t.stride(0), t.stride(2), t.stride(1)     # stride_l, stride_t, stride_h


def kv_copy_rows(src, dst, src_t0, dst_t0, n):
    """dst[l,h,dst_t0+i] = src[l,h,src_t0+i] for all layers/heads; src/dst are (L,H,T,D) views."""
    if n <= 0:
        return
    _dev(src, dst)
    L, H, _, D = src.shape
    assert dst.shape[0] == L and dst.shape[1] == H and dst.shape[3] == D
    if src_t0 < 0 or dst_t0 < 0 or src_t0 + n > src.shape[2] or dst_t0 + n > dst.shape[2]:
        raise IndexError(f"kv_copy_rows: rows [{src_t0}, {src_t0 + n}) of {src.shape[2]} -> [{dst_t0}, {dst_t0 + n}) of "
                         f"{dst.shape[2]} leave the cache (the kernel does not bounds-check)")
    ssl, sst, ssh = _lhtd(src)
    dsl, dst_t, dsh = _lhtd(dst)
    hip.check(hip.lib().tf_kv_copy_rows(_ptr(src), ssl, sst, ssh, _ptr(dst), dsl, dst_t, dsh, int(src_t0), int(dst_t0),
                                        int(n), L, H, D, _stream()), "tf_kv_copy_rows")


def kv_shift_rows(cache, src_t0, dst_t0, n):
    """In-place move of rows [src_t0, src_t0+n) down to [dst_t0, ...) (overlap allowed), all layers/heads."""
    if n <= 0 or src_t0 == dst_t0:
        return
    _dev(cache)
    L, H, T, D = cache.shape
    if src_t0 < 0 or dst_t0 < 0 or src_t0 + n > T or dst_t0 + n > T:
        raise IndexError(f"kv_shift_rows: rows [{src_t0}, {src_t0 + n}) -> [{dst_t0}, {dst_t0 + n}) leave the {T}-row cache")
    sl, st, sh = _lhtd(cache)
    hip.check(hip.lib().tf_kv_shift_rows(_ptr(cache), sl, st, sh, int(src_t0), int(dst_t0), int(n), L, H, D,
                                         _stream()), "tf_kv_shift_rows")


def kv_copy_rows_pair(src_k, src_v, dst_k, dst_v, src_t0, dst_t0, n):
    """kv_copy_rows for the K and the V tensor of one cache in ONE launch (same shapes / strides), else two."""
    if n <= 0:
        return
    if not (src_k.shape == src_v.shape and dst_k.shape == dst_v.shape and _lhtd(src_k) == _lhtd(src_v)
            and _lhtd(dst_k) == _lhtd(dst_v)):
        kv_copy_rows(src_k, dst_k, src_t0, dst_t0, n)
        kv_copy_rows(src_v, dst_v, src_t0, dst_t0, n)
        return
    _dev(src_k, src_v, dst_k, dst_v)
    L, H, _, D = src_k.shape
    assert dst_k.shape[0] == L and dst_k.shape[1] == H and dst_k.shape[3] == D
    if src_t0 < 0 or dst_t0 < 0 or src_t0 + n > src_k.shape[2] or dst_t0 + n > dst_k.shape[2]:
        raise IndexError(f"kv_copy_rows: rows [{src_t0}, {src_t0 + n}) of {src_k.shape[2]} -> [{dst_t0}, {dst_t0 + n}) of "
                         f"{dst_k.shape[2]} leave the cache (the kernel does not bounds-check)")
    ssl, sst, ssh = _lhtd(src_k)
    dsl, dst_t, dsh = _lhtd(dst_k)
    hip.check(hip.lib().tf_kv_copy_rows_pair(_ptr(src_k), _ptr(src_v), ssl, sst, ssh, _ptr(dst_k), _ptr(dst_v), dsl, dst_t,
                                             dsh, int(src_t0), int(dst_t0), int(n), L, H, D, _stream()),
              "tf_kv_copy_rows_pair")


def kv_shift_rows_pair(k_cache, v_cache, src_t0, dst_t0, n):
    """kv_shift_rows for the K and the V tensor of one cache in ONE launch (same shapes / strides), else two."""
    if n <= 0 or src_t0 == dst_t0:
        return
    if not (k_cache.shape == v_cache.shape and _lhtd(k_cache) == _lhtd(v_cache)):
        kv_shift_rows(k_cache, src_t0, dst_t0, n)
        kv_shift_rows(v_cache, src_t0, dst_t0, n)
        return
    _dev(k_cache, v_cache)
    L, H, T, D = k_cache.shape
    if src_t0 < 0 or dst_t0 < 0 or src_t0 + n > T or dst_t0 + n > T:
        raise IndexError(f"kv_shift_rows: rows [{src_t0}, {src_t0 + n}) -> [{dst_t0}, {dst_t0 + n}) leave the {T}-row cache")
    sl, st, sh = _lhtd(k_cache)
    hip.check(hip.lib().tf_kv_shift_rows_pair(_ptr(k_cache), _ptr(v_cache), sl, st, sh, int(src_t0), int(dst_t0), int(n),
                                              L, H, D, _stream()), "tf_kv_shift_rows_pair")


# ---- launch plans (round 5) ---------------------------------------------------------------------------------------------
# The decode loop issues the same few launches over the same buffers every step — the tail copy of the retrieval cache, the
# draft window shift, the token / position set-up — and the host time between a decision record and the next launch is GPU idle
# time (profiles/r05a_gap_analysis_decode_steps_inner_graph.txt: 36-108 us in front of each of them under the profiler).  A plan
# validates its tensors ONCE (what the wrappers above do on every call: device, dtype, shapes, strides, slicing views) and keeps
# the ctypes arguments; a call then checks its row range with integer arithmetic and goes straight into the library.


class KvCopyPairPlan:
    """kv_copy_rows_pair(src_k, src_v, dst_k, dst_v, ...) over fixed tensors."""

    def __init__(self, src_k, src_v, dst_k, dst_v):
        assert src_k.shape == src_v.shape and dst_k.shape == dst_v.shape and _lhtd(src_k) == _lhtd(src_v) \
            and _lhtd(dst_k) == _lhtd(dst_v), "K and V must share shapes and strides"
        _dev(src_k, src_v, dst_k, dst_v)
        L, H, _, D = src_k.shape
        assert dst_k.shape[0] == L and dst_k.shape[1] == H and dst_k.shape[3] == D
        self.keep = (src_k, src_v, dst_k, dst_v)
        self.src_rows, self.dst_rows = src_k.shape[2], dst_k.shape[2]
        self.head = (_ptr(src_k), _ptr(src_v)) + _lhtd(src_k) + (_ptr(dst_k), _ptr(dst_v)) + _lhtd(dst_k)
        self.dims = (L, H, D)
        self.fn = hip.lib().tf_kv_copy_rows_pair

    def __call__(self, src_t0, dst_t0, n):
        if n <= 0:
            return
        if src_t0 < 0 or dst_t0 < 0 or src_t0 + n > self.src_rows or dst_t0 + n > self.dst_rows:
            raise IndexError(f"kv_copy_rows: rows [{src_t0}, {src_t0 + n}) of {self.src_rows} -> [{dst_t0}, {dst_t0 + n}) of "
                             f"{self.dst_rows} leave the cache (the kernel does not bounds-check)")
        hip.check(self.fn(*self.head, int(src_t0), int(dst_t0), int(n), *self.dims, _stream()), "tf_kv_copy_rows_pair")


class KvShiftPairPlan:
    """kv_shift_rows_pair(k_cache, v_cache, ...) over fixed tensors."""

    def __init__(self, k_cache, v_cache):
        assert k_cache.shape == v_cache.shape and _lhtd(k_cache) == _lhtd(v_cache), "K and V must share shapes and strides"
        _dev(k_cache, v_cache)
        L, H, T, D = k_cache.shape
        self.keep, self.rows = (k_cache, v_cache), T
        self.head = (_ptr(k_cache), _ptr(v_cache)) + _lhtd(k_cache)
        self.dims = (L, H, D)
        self.fn = hip.lib().tf_kv_shift_rows_pair

    def __call__(self, src_t0, dst_t0, n):
        if n <= 0 or src_t0 == dst_t0:
            return
        if src_t0 < 0 or dst_t0 < 0 or src_t0 + n > self.rows or dst_t0 + n > self.rows:
            raise IndexError(f"kv_shift_rows: rows [{src_t0}, {src_t0 + n}) -> [{dst_t0}, {dst_t0 + n}) leave the {self.rows}-row cache")
        hip.check(self.fn(*self.head, int(src_t0), int(dst_t0), int(n), *self.dims, _stream()), "tf_kv_shift_rows_pair")


class SetTokensPlan:
    """set_tokens over fixed buffers: dst (its first n_dst entries are written, n_dst <= dst.numel()), pos, slot, sk."""

    def __init__(self, dst, pos=None, slot=None, sk=None):
        assert dst is None or (dst.dtype == torch.int64 and dst.is_contiguous() and dst.numel() <= 32)
        assert pos is None or (pos.dtype == torch.int64 and pos.is_contiguous() and pos.numel() <= 64)
        assert (slot is None or slot.dtype == torch.int32) and (sk is None or sk.dtype == torch.int32)
        _dev(dst, pos, slot, sk)
        self.keep = (dst, pos, slot, sk)
        self.n_dst = 0 if dst is None else dst.numel()
        self.p_dst, self.p_pos, self.n_pos = _ptr(dst), _ptr(pos), 0 if pos is None else pos.numel()
        self.p_slot, self.p_sk = _ptr(slot), _ptr(sk)
        self.fn = hip.lib().tf_set_tokens
        self.arr = ctypes.c_int64 * 32

    def __call__(self, vals, pad, pos0=0, sk_val=0, n_dst=None):
        n_vals = len(vals)
        n_dst = self.n_dst if n_dst is None else n_dst
        assert n_vals <= 32 and n_dst <= self.n_dst
        hip.check(self.fn(self.p_dst, n_dst, self.arr(*vals), n_vals, int(pad), self.p_pos, self.n_pos, int(pos0), self.p_slot,
                          self.p_sk, int(sk_val), _stream()), "tf_set_tokens")


def kv_gather_rows(k_cache, v_cache, offset, idx, max_index=None):
    """Rows offset+idx[j] -> offset+j of every layer/head of the (L,H,T,D) K and V views (idx: device int32,
    strictly increasing) — gather_kv_incremental (reference cache.py:333-343).  max_index: the largest entry of idx as
    the host knows it (the list the device tensor was built from), so that the source rows can be bounds-checked
    without reading the device tensor back."""
    _dev(k_cache, v_cache, idx)
    L, H, T, D = k_cache.shape
    sl, st, sh = _lhtd(k_cache)
    assert _lhtd(v_cache) == (sl, st, sh) and idx.dtype == torch.int32 and idx.is_contiguous()
    if offset < 0 or offset + idx.numel() > T or (max_index is not None and offset + max_index >= T):
        raise IndexError(f"kv_gather_rows: {idx.numel()} rows at offset {offset} (largest index {max_index}) leave the "
                         f"{T}-row cache")
    hip.check(hip.lib().tf_kv_gather_rows(_ptr(k_cache), _ptr(v_cache), sl, st, sh, int(offset), _ptr(idx),
                                          idx.numel(), L, H, D, _stream()), "tf_kv_gather_rows")


def sample_without_replacement(logits, rand, k, temperature):
    """(rows*k,) int64: per row the k token ids with the largest log(rand)/softmax(logits/T), descending —
    `(rand.log() / q).topk(k).indices.flatten()` of the reference's sampling callable, one kernel."""
    _dev(logits, rand)
    rows, V = logits.shape
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and logits.stride(0) == V
    assert rand.dtype == _HALF and rand.shape == logits.shape and rand.stride(1) == 1 and rand.stride(0) == V
    out = torch.empty(rows * k, dtype=torch.int64, device=logits.device)
    hip.check(hip.lib().tf_sample_without_replacement(_ptr(logits), _ptr(rand), _ptr(out), rows, V, int(k),
                                                      float(temperature), _stream()), "tf_sample_without_replacement")
    return out


TREE_ACCEPT_OUT = 64
TREE_ACCEPT_MAX_PATH = 60       # accepted nodes the record can hold (TREE_MAX_PATH in csrc/sampling.hip)


def tree_accept(p_rows, draft_logits, tokens, succ_off, succ, uniforms, temperature, out):
    """Sequoia tree walk on the device: out[64] int64 <- (len(accept_list), next_token, terminal,
    uniforms_consumed, accept_list...); see include/triforce_hip.h."""
    _dev(p_rows, draft_logits, tokens, succ_off, succ, uniforms, out)
    N, V = p_rows.shape
    assert p_rows.dtype == torch.float32 and p_rows.is_contiguous() and draft_logits.shape == p_rows.shape
    assert draft_logits.dtype == torch.float32 and draft_logits.is_contiguous()
    assert tokens.dtype == torch.int64 and tokens.numel() == N and succ_off.dtype == torch.int32
    assert succ_off.numel() == N + 1 and succ.dtype == torch.int32 and uniforms.dtype == torch.float32
    assert out.dtype == torch.int64 and out.numel() >= TREE_ACCEPT_OUT
    hip.check(hip.lib().tf_tree_accept(_ptr(p_rows), _ptr(draft_logits), _ptr(tokens), _ptr(succ_off), _ptr(succ),
                                       _ptr(uniforms), V, float(temperature), _ptr(out), _stream()), "tf_tree_accept")


TOPP_MAX_VOCAB = 32768


TOPP_MULTI = _os.environ.get("TRIFORCE_TOPP_MULTI", "1") != "0"
_topp_multi_state = {}


def _device_key(device):
    """The key of per-device state: the device's index, a device without one ("cuda") being the current device."""
    dev = torch.device(device)
    return torch.cuda.current_device() if dev.index is None else dev.index


def _probs_like(logits):
    """The output of a normaliser over (rows, V) fp32 device logits, behind the checks all of them make."""
    _dev(logits)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous()
    return torch.empty_like(logits)


def _topp_multi(device):
    """(control block, workspace) of tf_topp_probs_multi for this device, allocated at the first call OUTSIDE a capture (a
    graph's warm-up passes always come first); None while capturing without one.  One per device: the launches of a process are
    stream-ordered or synchronised against each other (warm-up stream -> capture -> replays); a caller that runs top-p on two
    streams at once sets TRIFORCE_TOPP_MULTI=0."""
    key = _device_key(device)
    st = _topp_multi_state.get(key)
    if st is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        L = hip.lib()
        st = (torch.zeros(int(L.tf_topp_multi_ctl_bytes()), dtype=torch.uint8, device=device),
              torch.empty(int(L.tf_topp_multi_ws_bytes(32, 32768)), dtype=torch.uint8, device=device))
        _topp_multi_state[key] = st
    return st


def topp_probs(logits, temperature, top_p, panel_max=None):
    """softmax(top_p_filter(logits / temperature)) for (rows, V) fp32 logits, V <= 32768 (above: topp_probs_large) — one fused kernel: every row over 16
    workgroups with in-launch hand-offs (tf_topp_probs_multi) where the shape allows, else one workgroup per row
    (tf_topp_probs); bit-identical.  ``panel_max``: the per-panel row maxima the lm_head GEMM left (ops.linear(...,
    out_f32=True, ss_out=...)): the multi-workgroup form then skips its first hand-off."""
    probs = _probs_like(logits)
    rows, V = logits.shape
    # (<= 16 rows: from 17 rows the launch has 8 slices of 4 000 entries per row — 36.8 -> 30.2 us on model-like rows, but
    #  52.6 -> 81.5 on near-flat ones: profiles/r06_topp_one_workgroup_vs_multi.jsonl; those calls keep one workgroup per row)
    if TOPP_MULTI and rows <= 16 and V % 4 == 0 and 64 <= V <= 32768 and logits.data_ptr() % 16 == 0:
        st = _topp_multi(logits.device)
        if st is not None:
            rc = hip.lib().tf_topp_probs_multi(_ptr(logits), _ptr(panel_max), _ptr(probs), rows, V, float(temperature),
                                               float(top_p), _ptr(st[0]), _ptr(st[1]), st[1].numel(), _stream())
            if rc == 0:
                return probs
            if rc != -34:                                        # TF_ERANGE: more workgroups than CUs — the one-per-row kernel
                hip.check(rc, "tf_topp_probs_multi")
    hip.check(hip.lib().tf_topp_probs(_ptr(logits), _ptr(probs), logits.shape[0], logits.shape[1], float(temperature),
                                      float(top_p), _stream()), "tf_topp_probs")
    return probs


def topk_topp_probs(logits, temperature, top_k, top_p):
    """softmax(top_p_filter(top_k_filter(logits / temperature))) for (rows, V) fp32 logits, V <= 32768 (above: topk_topp_probs_large), top_k >= 1 — one fused
    kernel, one workgroup per row (tf_topk_topp_probs): every entry tied with the k-th value survives the top-k filter, the
    rest is tf_topp_probs over the survivors; top_k >= V is tf_topp_probs bit for bit."""
    probs = _probs_like(logits)
    hip.check(hip.lib().tf_topk_topp_probs(_ptr(logits), _ptr(probs), logits.shape[0], logits.shape[1], float(temperature),
                                           int(top_k), float(top_p), _stream()), "tf_topk_topp_probs")
    return probs


# Vocabularies above TOPP_MAX_VOCAB: the same two normalisers with the row streamed through a workspace
# instead of held in LDS.  TOPP_MAX_VOCAB stays the limit of everything else that says so (utils/SpecTree_TP.py gates the tree
# sampler on it).
TOPP_LARGE_MAX_VOCAB = 262144
TOPP_LARGE_MAX_ROWS = 32
_topp_large_state = {}


def topp_large_ws_bytes(rows, V):
    """TF_TOPP_LARGE_WS_BYTES(rows, V) of include/triforce_hip.h: per row the x / e values and the candidate list, each padded
    to whole slabs of 4 096 entries."""
    return int(rows) * (((int(V) + 4095) >> 12) * 4096 * 2) * 4


def topp_route(V, top_p, is_device=True, dtype=torch.float32):
    """Which normaliser utils.sampling.norm_logits takes for (rows, V) logits: "fused" (tf_topp_probs / tf_topk_topp_probs,
    V <= TOPP_MAX_VOCAB), "large" (the _large forms, up to TOPP_LARGE_MAX_VOCAB) or "torch" (the sort restatement: CPU
    tensors, other dtypes, top_p <= 0, larger vocabularies)."""
    if not is_device or dtype != torch.float32 or not 0.0 < top_p:
        return "torch"
    if V <= TOPP_MAX_VOCAB:
        return "fused"
    return "large" if V <= TOPP_LARGE_MAX_VOCAB else "torch"


def _topp_large_ws(device, rows, V):
    """Workspace of the _large normalisers for this device: allocated (or grown) at a call OUTSIDE a capture — a graph's
    warm-up passes always come first — and then kept, so a captured launch never allocates.  One per device: the launches of a
    process are stream-ordered or synchronised against each other, as for _topp_multi."""
    key = _device_key(device)
    need = topp_large_ws_bytes(rows, V)
    bufs = _topp_large_state.setdefault(key, [])
    if not bufs or bufs[-1].numel() < need:
        if torch.cuda.is_current_stream_capturing():
            raise hip.TriforceHipError(f"topp_probs_large: no workspace for ({rows}, {V}) on device {key} inside a capture "
                                       "(run the call once outside the capture first)")
        # sized for every row count this vocabulary can be called with; an outgrown buffer is kept, not freed: a captured
        # graph may still replay launches that hold its address
        bufs.append(torch.empty(topp_large_ws_bytes(TOPP_LARGE_MAX_ROWS, V), dtype=torch.uint8,
                                device=torch.device("cuda", key)))
    return bufs[-1]


def _topp_large_call(name, logits, *args):
    """probs for (rows, V) fp32 logits through the C entry ``name``(logits, probs, rows, V, *args, workspace, bytes, stream), at
    most TOPP_LARGE_MAX_ROWS rows per launch (stream-ordered: they share the workspace)."""
    probs = _probs_like(logits)
    rows, V = logits.shape
    launch = getattr(hip.lib(), name)
    ws = _topp_large_ws(logits.device, min(rows, TOPP_LARGE_MAX_ROWS), V)
    for r0 in range(0, rows, TOPP_LARGE_MAX_ROWS):
        n = min(TOPP_LARGE_MAX_ROWS, rows - r0)
        hip.check(launch(_ptr(logits[r0:r0 + n]), _ptr(probs[r0:r0 + n]), n, V, *args, _ptr(ws), ws.numel(), _stream()), name)
    return probs


def topp_probs_large(logits, temperature, top_p):
    """softmax(top_p_filter(logits / temperature)) for (rows, V) fp32 logits, V <= 262144 — tf_topp_probs_large: one workgroup
    per row, the row streamed through a per-device workspace; bit-identical to topp_probs where both apply."""
    return _topp_large_call("tf_topp_probs_large", logits, float(temperature), float(top_p))


def topk_topp_probs_large(logits, temperature, top_k, top_p):
    """topk_topp_probs for (rows, V) fp32 logits, V <= 262144, top_k >= 1 — tf_topk_topp_probs_large."""
    return _topp_large_call("tf_topk_topp_probs_large", logits, float(temperature), int(top_k), float(top_p))


def minp_probs(logits, temperature, top_k, top_p, min_p):
    """softmax(min_p_filter(top_p_filter(top_k_filter(logits / temperature)))) for (rows, V) fp32 logits, V <= 32768 (above:
    minp_probs_large), 0 < min_p <= 1 — tf_minp_probs, one workgroup per row: behind the select of topp_probs /
    topk_topp_probs an entry stays iff e_i = expf(x_i - max) >= min_p.  top_k <= 0 or top_k >= V: no top-k filter.  Where
    min-p removes nothing the output is topp_probs' / topk_topp_probs' (one workgroup per row) bit for bit."""
    probs = _probs_like(logits)
    hip.check(hip.lib().tf_minp_probs(_ptr(logits), _ptr(probs), logits.shape[0], logits.shape[1], float(temperature),
                                      int(top_k), float(top_p), float(min_p), _stream()), "tf_minp_probs")
    return probs


def minp_probs_large(logits, temperature, top_k, top_p, min_p):
    """minp_probs for (rows, V) fp32 logits, V <= 262144 — tf_minp_probs_large, the row streamed through the per-device
    workspace of topp_probs_large; bit-identical to minp_probs where both apply."""
    return _topp_large_call("tf_minp_probs_large", logits, float(temperature), int(top_k), float(top_p), float(min_p))


PENALTY_MAX_ROWS = 64


class PenaltyState:
    """What the target tier's penalties remember, per engine: ``gen_count`` (V,) int32 — occurrences among
    the generated tokens of the current answer, the pending token excluded — and ``prompt_seen`` (V,) uint8 — 1 where the token
    occurs in the context the answer is conditioned on.  Allocated once; the kernels hold its addresses (captured graphs)."""

    def __init__(self, V, device):
        self.V = int(V)
        self.gen_count = torch.zeros(self.V, dtype=torch.int32, device=device)
        self.prompt_seen = torch.zeros(self.V, dtype=torch.uint8, device=device)

    def reset(self, context_ids):
        """A new answer: ``prompt_seen`` becomes the set of ``context_ids`` (any shape, ids outside [0, V) ignored), no token
        generated yet.  Torch fill / scatter in place, once per prompt."""
        ids = torch.as_tensor(context_ids, dtype=torch.long, device=self.gen_count.device).reshape(-1)
        ids = ids[(ids >= 0) & (ids < self.V)]
        self.prompt_seen.zero_()
        self.prompt_seen.index_fill_(0, ids, 1)
        self.gen_count.zero_()


def penalize_logits(logits, ids, state, penalties, out=None):
    """(rows, V) fp32 device logits -> the penalised rows of include/triforce_hip.h "SAMPLING PENALTIES" (tf_penalize_logits, one
    launch, 1 <= rows <= 64): row i counts ``state.gen_count`` plus ids[0 .. i].  ``ids``: None, or an int64 device tensor whose
    first ``rows`` entries are the block's input tokens.  ``penalties``: .repetition / .frequency / .presence.  ``out``: fp32
    (rows, V) device tensor, unit stride on V (``logits`` itself is allowed); allocated when None.  The state is only read."""
    _dev(logits, ids, state.gen_count, state.prompt_seen, out)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.numel() > 0
    rows, V = logits.shape
    assert V == state.V and rows <= PENALTY_MAX_ROWS
    if out is None:
        out = torch.empty((rows, V), dtype=torch.float32, device=logits.device)
    assert out.dtype == torch.float32 and tuple(out.shape) == (rows, V) and out.stride(1) == 1
    if ids is not None:
        ids = ids.reshape(-1)
        assert ids.dtype == torch.int64 and ids.numel() >= rows and ids.is_contiguous()
    ls = logits.stride(0) if rows > 1 else max(logits.stride(0), V)
    os_ = out.stride(0) if rows > 1 else max(out.stride(0), V)
    hip.check(hip.lib().tf_penalize_logits(_ptr(logits), ls, _ptr(out), os_, _ptr(ids), _ptr(state.gen_count),
                                           _ptr(state.prompt_seen), rows, V, float(penalties.repetition),
                                           float(penalties.frequency), float(penalties.presence), _stream()),
              "tf_penalize_logits")
    return out


def penalty_commit(state, ids_row, n):
    """state.gen_count[ids_row[j]] += 1 for j < n (tf_penalty_commit: one small launch, 0 <= n <= 64; duplicates accumulate, ids
    outside [0, V) are skipped).  ``ids_row``: int64 device tensor with at least n entries."""
    _dev(state.gen_count, ids_row)
    ids_row = ids_row.reshape(-1)
    assert ids_row.dtype == torch.int64 and ids_row.is_contiguous() and 0 <= n <= min(ids_row.numel(), PENALTY_MAX_ROWS)
    hip.check(hip.lib().tf_penalty_commit(_ptr(state.gen_count), _ptr(ids_row), int(n), state.V, _stream()),
              "tf_penalty_commit")


# ---- prompt-lookup n-gram draft (include/triforce_hip.h "N-GRAM DRAFT") ------------------------------------
NGRAM_MAX_N = 8
NGRAM_MAX_BLOCK = 32
NGRAM_MAX_COMMIT = 64
_ngram_ws = {}


@functools.lru_cache(maxsize=None)
def _ngram_shape():
    out = (ctypes.c_int32 * 2)()
    hip.check(hip.lib().tf_ngram_draft_shape(out), "tf_ngram_draft_shape")
    return int(out[0]), int(out[1])


def ngram_draft_threads():
    """Threads of tf_ngram_draft's fixed grid: thread t owns the candidates 4 g .. 4 g + 3 for g = t, t + threads, ..."""
    return _ngram_shape()[0]


def ngram_workspace(device):
    """A zeroed workspace of tf_ngram_draft (packed key + ticket): every launch leaves it zero again."""
    return torch.zeros(_ngram_shape()[1] // 8, dtype=torch.int64, device=device)


def _ngram_default_ws(device):
    """The per-device workspace of ngram_draft calls that bring none, allocated at the first call outside a capture (a graph's
    warm-up passes always come first).  Its launches must be stream-ordered: a caller with two streams brings its own."""
    key = _device_key(device)
    ws = _ngram_ws.get(key)
    if ws is None:
        assert not torch.cuda.is_current_stream_capturing(), "ngram_draft: first call inside a capture without ws="
        ws = _ngram_ws[key] = ngram_workspace(device)
    return ws


def ngram_draft(hist, len_dev, blk, N, V, q=None, info=None, ws=None):
    """Prompt lookup over ctx = hist[0:L] ++ blk (L = len_dev[0] clamped to [0, hist.numel()]): the one-hot row ``q`` (fp32, V)
    of the token that followed the most recent, longest (<= N) earlier occurrence of the context's last tokens, and ``info``
    (int32, 4) = (token, match length, match position or -1, context length) — the rule of include/triforce_hip.h "N-GRAM
    DRAFT".  ``hist`` int32, ``len_dev`` int32 scalar tensor, ``blk`` int64 with 1 <= numel <= 32, 1 <= N <= 8.  Device
    tensors: tf_ngram_draft, one launch, capturable (``ws``: ngram_workspace(), default one per device).  CPU tensors: the
    torch restatement ngram_draft_host (the tests' oracle; it lets the CPU suite drive the real loop).  Returns (q, info)."""
    blk = blk.reshape(-1)
    m, V, N = blk.numel(), int(V), int(N)
    assert hist.dtype == torch.int32 and hist.dim() == 1 and hist.is_contiguous() and hist.numel() >= 1
    assert len_dev.dtype == torch.int32 and len_dev.numel() == 1 and blk.dtype == torch.int64 and blk.is_contiguous()
    assert 1 <= m <= NGRAM_MAX_BLOCK and 1 <= N <= NGRAM_MAX_N and V >= 1
    if q is None:
        q = torch.empty(V, dtype=torch.float32, device=hist.device)
    if info is None:
        info = torch.empty(4, dtype=torch.int32, device=hist.device)
    assert q.dtype == torch.float32 and q.numel() == V and q.is_contiguous()
    assert info.dtype == torch.int32 and info.numel() == 4 and info.is_contiguous()
    if not hist.is_cuda:
        return ngram_draft_host(hist, len_dev, blk, N, V, q, info)
    _dev(hist, len_dev, blk, q, info)
    if ws is None:
        ws = _ngram_default_ws(hist.device)
    assert ws.is_cuda and ws.dtype == torch.int64 and ws.numel() * 8 >= _ngram_shape()[1]
    hip.check(hip.lib().tf_ngram_draft(_ptr(hist), hist.numel(), _ptr(len_dev), _ptr(blk), m, N, V, _ptr(q), _ptr(info), _ptr(ws),
                                       _stream()), "tf_ngram_draft")
    return q, info


def ngram_draft_host(hist, len_dev, blk, N, V, q=None, info=None):
    """tf_ngram_draft restated in torch for CPU tensors: same reads, same row, same info."""
    blk = blk.reshape(-1)
    L = min(max(int(len_dev), 0), hist.numel())
    ctx = torch.cat([hist[:L].to(torch.int64), blk.to(torch.int64)])
    T = ctx.numel()
    valid = (ctx >= 0) & (ctx < V)
    best, at = 0, -1
    if T >= 2:
        j = torch.arange(T - 1)
        run = torch.ones(T - 1, dtype=torch.bool)
        length = torch.zeros(T - 1, dtype=torch.int64)
        for k in range(min(int(N), T - 1)):                # l(j): the run of k = 0, 1, .. with ctx[j - k] == ctx[T - 1 - k]
            src = j - k
            inside = src >= 0
            src = src.clamp(min=0)
            run &= inside & valid[src] & (ctx[src] == ctx[T - 1 - k])
            length += run
        best = int(length.max())
        if best >= 1:
            at = int((length == best).nonzero()[-1])       # the most recent among equals
    d = int(ctx[at + 1]) if best >= 1 else int(ctx[T - 1])
    if not 0 <= d < V:
        d = 0
    if q is None:
        q = torch.empty(V, dtype=torch.float32)
    if info is None:
        info = torch.empty(4, dtype=torch.int32)
    q.zero_()
    q[d] = 1.0
    info.copy_(torch.tensor([d, best, at, T], dtype=torch.int32))
    return q, info


def ngram_commit(hist, len_dev, src, n):
    """hist[L + i] = (int32)src[i] for i < n, then len_dev += n (tf_ngram_commit: one wave, outside every graph; 0 <= n <= 64).
    L + n > hist.numel() writes nothing: the caller checks the capacity first (models/ngram_draft.NgramCache.commit raises
    IndexError).  ``src``: int64 tensor with at least n entries.  CPU tensors: the same in torch."""
    src = src.reshape(-1)
    n = int(n)
    assert hist.dtype == torch.int32 and hist.dim() == 1 and hist.is_contiguous() and hist.numel() >= 1
    assert len_dev.dtype == torch.int32 and len_dev.numel() == 1
    assert src.dtype == torch.int64 and src.is_contiguous() and 0 <= n <= min(src.numel(), NGRAM_MAX_COMMIT)
    if not hist.is_cuda:
        L = int(len_dev)
        if n > 0 and 0 <= L and L + n <= hist.numel():
            hist[L:L + n] = src[:n].to(torch.int32)
            len_dev.fill_(L + n)
        return
    _dev(hist, len_dev, src)
    hip.check(hip.lib().tf_ngram_commit(_ptr(hist), hist.numel(), _ptr(len_dev), _ptr(src), n, _stream()), "tf_ngram_commit")


# Rows of normalised hidden state that DecoderLayers.head scores per lm_head GEMM when it is asked for the prompt's
# log-probabilities: the fp32 logits block is SCORE_BLOCK_ROWS x V (131 MB at 32 000) instead of chunk x V.
SCORE_BLOCK_ROWS = 1024
TOKEN_LOGPROBS_MAX_IDS = 32


def token_logprobs(logits, targets=None, out=None, lse=None):
    """out[r] = log_softmax(logits[r])[targets[r]] at temperature 1, no top-k / top-p filter, for (rows, V) fp32 device logits
    (unit stride on V, any row stride >= V, any V) — tf_token_logprobs, one launch; a target outside [0, V) gives 0.
    ``targets``: an int64 device tensor of ``rows`` ids; or a python list of <= 32 ids, which travel as kernel arguments
    (tf_token_logprobs_ids: no upload); or None when only ``lse`` (fp32, rows) = log sum exp of every row is wanted.
    ``out`` / ``lse``: contiguous fp32 device tensors of ``rows`` entries to write (``out`` is allocated when there are
    targets and none is given).  Returns ``out`` (``lse`` when there are no targets)."""
    _dev(logits, out, lse)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.numel() > 0
    rows, V = logits.shape
    stride = logits.stride(0) if rows > 1 else max(logits.stride(0), V)
    assert stride >= V, "rows of the logits block overlap"
    if targets is None:
        assert lse is not None, "token_logprobs needs targets or lse"
    elif out is None:
        out = torch.empty(rows, dtype=torch.float32, device=logits.device)
    for t in (out, lse):
        assert t is None or (t.dtype == torch.float32 and t.numel() == rows and t.is_contiguous())
    if isinstance(targets, (list, tuple)):
        assert len(targets) == rows <= TOKEN_LOGPROBS_MAX_IDS
        host = (ctypes.c_int64 * rows)(*[int(t) for t in targets])
        hip.check(hip.lib().tf_token_logprobs_ids(_ptr(logits), stride, host, rows, V, _ptr(out), _ptr(lse), _stream()),
                  "tf_token_logprobs_ids")
        return out
    if targets is not None:
        _dev(targets)
        targets = targets.reshape(-1)
        assert targets.dtype == torch.int64 and targets.numel() == rows and targets.is_contiguous()
    hip.check(hip.lib().tf_token_logprobs(_ptr(logits), stride, _ptr(targets), rows, V, _ptr(out), _ptr(lse), _stream()),
              "tf_token_logprobs")
    return lse if targets is None else out


def sample_inverse_cdf(probs, u, token_out):
    """token_out[0] <- first index with inclusive cumsum(probs) > u[0]*sum(probs).  All device tensors."""
    _dev(probs, u)
    _dev_or_pinned(token_out)
    assert probs.dtype == torch.float32 and probs.is_contiguous() and probs.dim() == 1
    assert u.dtype == torch.float32 and token_out.dtype == torch.int64
    hip.check(hip.lib().tf_sample_inverse_cdf(_ptr(probs), _ptr(u), _ptr(token_out), probs.numel(), _stream()),
              "tf_sample_inverse_cdf")


def accept_chain(p, q, tokens, uniforms, g2, inclusive, eos_token_id, out):
    """out[4] int64 <- (count, next_token, reason, uniforms_consumed); see include/triforce_hip.h."""
    _dev(p, q, tokens, uniforms)
    _dev_or_pinned(out)
    V = p.shape[-1]
    assert p.dtype == torch.float32 and p.is_contiguous() and p.shape[0] >= g2 + 1
    assert q.dtype == torch.float32 and q.is_contiguous() and q.shape[0] >= g2 and q.shape[-1] == V
    assert tokens.dtype == torch.int64 and tokens.numel() >= g2 and uniforms.numel() >= g2 + 1
    assert out.dtype == torch.int64 and out.numel() >= 4
    hip.check(hip.lib().tf_accept_chain(_ptr(p), _ptr(q), _ptr(tokens), _ptr(uniforms), int(g2), V,
                                        1 if inclusive else 0, int(eos_token_id), _ptr(out), _stream()),
              "tf_accept_chain")


def middle_accept(p, q_d, tokens, uniforms, n, gamma, out):
    """One Middle_Spec step on device: out[3] int64 <- (accepted, follow_up_token, drafted_token)."""
    _dev(p, q_d, tokens, uniforms)
    _dev_or_pinned(out)
    V = p.shape[-1]
    assert p.dtype == torch.float32 and p.is_contiguous() and q_d.dtype == torch.float32 and q_d.numel() == V
    assert tokens.dtype == torch.int64 and tokens.numel() >= gamma + 1 and uniforms.numel() >= 2
    hip.check(hip.lib().tf_middle_accept(_ptr(p), _ptr(q_d), _ptr(tokens), _ptr(uniforms), int(n), int(gamma), V,
                                         _ptr(out), _stream()), "tf_middle_accept")


def mid_record_tokens(rec, tokens, n):
    """tokens[n + 1] (, tokens[n + 2]) <- what the middle_accept record ``rec`` (accepted, follow-up, drafted) implies."""
    _dev(rec, tokens)
    assert rec.dtype == torch.int64 and tokens.dtype == torch.int64 and tokens.is_contiguous() and rec.numel() >= 3
    hip.check(hip.lib().tf_mid_record_tokens(_ptr(rec), _ptr(tokens), tokens.numel(), int(n), _stream()), "tf_mid_record_tokens")


# ---- the same three kernels with their uniforms behind a device cursor: u_k = ubuf[cursor[0] + k] (capturable) -------------
def sample_inverse_cdf_cur(probs, ubuf, cursor, off, token_out):
    """token_out[0] <- sample(probs) with u = ubuf[cursor[0] + off]; the cursor is left alone."""
    _dev(probs, ubuf, cursor)
    _dev_or_pinned(token_out)
    assert probs.dtype == torch.float32 and probs.is_contiguous() and probs.dim() == 1
    assert ubuf.dtype == torch.float32 and cursor.dtype == torch.int64 and token_out.dtype == torch.int64
    hip.check(hip.lib().tf_sample_inverse_cdf_cur(_ptr(probs), _ptr(ubuf), _ptr(cursor), int(off), _ptr(token_out),
                                                  probs.numel(), _stream()), "tf_sample_inverse_cdf_cur")


def middle_accept_cur(p, q_d, tokens, ubuf, cursor, n, gamma, out):
    """middle_accept over ubuf[cursor + 1], ubuf[cursor + 2]; cursor += 3; out[4] <- (accepted, follow-up, drafted, cursor
    value the decision started from)."""
    _dev(p, q_d, tokens, ubuf, cursor)
    _dev_or_pinned(out)
    V = p.shape[-1]
    assert p.dtype == torch.float32 and p.is_contiguous() and q_d.dtype == torch.float32 and q_d.numel() == V
    assert tokens.dtype == torch.int64 and tokens.numel() >= gamma + 1 and out.numel() >= 4
    assert ubuf.dtype == torch.float32 and cursor.dtype == torch.int64
    hip.check(hip.lib().tf_middle_accept_cur(_ptr(p), _ptr(q_d), _ptr(tokens), tokens.numel(), _ptr(ubuf), _ptr(cursor), int(n),
                                             int(gamma), V, _ptr(out), _stream()), "tf_middle_accept_cur")


MID2_RECORD = 8       # (acc1, b1, d1, cursor at entry, stage2_ran, acc2, b2, d2): the record of a depth-2 middle_accept2_cur


def middle_accept2_cur(p, q1, q3, tokens, ubuf, cursor, n, gamma, out, depth=2):
    """Positions n and (when stage 1 accepts and its follow-up equals the guess in tokens[n + 2]) n + 2 of Middle_Spec decided
    from ONE verify's rows ``p`` (tf_middle_accept2_cur): q1 / q3 are the draft rows tokens[n + 1] /
    tokens[n + 3] were drawn from with ubuf[cursor], ubuf[cursor + 3]; cursor += 3 or 6; out[8] <- (acc1, b1, d1, cursor at
    entry, stage2_ran, acc2, b2, d2).  CPU tensors: the torch restatement below (the tests' oracle)."""
    V = p.shape[-1]
    assert p.dtype == torch.float32 and p.is_contiguous() and p.shape[0] >= gamma + 1
    assert q1.dtype == torch.float32 and q1.numel() == V and (depth == 1 or (q3.dtype == torch.float32 and q3.numel() == V))
    assert tokens.dtype == torch.int64 and tokens.is_contiguous() and tokens.numel() >= gamma + 1
    assert depth in (1, 2) and 0 <= n and n + 2 * (depth - 1) + 1 <= gamma and out.dtype == torch.int64
    assert out.numel() >= 5 + 3 * (depth - 1) and ubuf.dtype == torch.float32 and cursor.dtype == torch.int64
    if not p.is_cuda:
        return middle_accept2_host(p, q1, q3, tokens, ubuf, cursor, n, gamma, out, depth)
    _dev(p, q1, q3, tokens, ubuf, cursor)
    _dev_or_pinned(out)
    hip.check(hip.lib().tf_middle_accept2_cur(_ptr(p), _ptr(q1), _ptr(q3), _ptr(tokens), tokens.numel(), _ptr(ubuf), _ptr(cursor),
                                              int(n), int(gamma), V, int(depth), _ptr(out), _stream()), "tf_middle_accept2_cur")


MID_MAX_DEPTH = 4     # the stage loop's limit in csrc/sampling.hip


def mid_record_len(depth):
    """Entries of the record of a depth-`depth` accept: (acc, b, d, cursor at entry, further stages run) + (acc, b, d) per further stage."""
    return 5 + 3 * (depth - 1)


MID3_RECORD = mid_record_len(3)     # 11


def middle_accept_n_cur(p, qs, tokens, ubuf, cursor, n, gamma, out, depth=None):
    """Up to `depth` (default len(qs), <= MID_MAX_DEPTH) successive positions n, n + 2, .. of Middle_Spec decided from ONE
    verify's rows ``p`` (tf_middle_accept_n_cur).  ``qs`` holds one draft row per stage (q1, q3, q5, ..: the
    rows tokens[n + 1], tokens[n + 3], .. were drawn from with ubuf[cursor + 3 s]); stage s runs iff every earlier stage
    accepted and its follow-up equals the guess in tokens[n + 2 s].  cursor += 3 x stages run; out[5 + 3 (depth - 1)] <- the
    record, every entry written.  CPU tensors: the torch restatement below (the tests' oracle)."""
    qs = list(qs)
    depth = len(qs) if depth is None else int(depth)
    V = p.shape[-1]
    assert p.dtype == torch.float32 and p.is_contiguous() and p.shape[0] >= gamma + 1
    assert 1 <= depth <= MID_MAX_DEPTH and len(qs) >= depth and 0 <= n and n + 2 * (depth - 1) + 1 <= gamma
    assert all(q is not None and q.dtype == torch.float32 and q.numel() == V for q in qs[:depth]), "one draft row per stage"
    assert tokens.dtype == torch.int64 and tokens.is_contiguous() and tokens.numel() >= gamma + 1
    assert out.dtype == torch.int64 and out.numel() >= mid_record_len(depth)
    assert ubuf.dtype == torch.float32 and cursor.dtype == torch.int64
    if not p.is_cuda:
        return middle_accept_n_host(p, qs, tokens, ubuf, cursor, n, gamma, out, depth)
    _dev(p, tokens, ubuf, cursor, *qs[:depth])
    _dev_or_pinned(out)
    q = [_ptr(qs[s]) if s < depth else None for s in range(MID_MAX_DEPTH)]
    hip.check(hip.lib().tf_middle_accept_n_cur(_ptr(p), q[0], q[1], _ptr(tokens), tokens.numel(), _ptr(ubuf), _ptr(cursor), int(n),
                                               int(gamma), V, depth, _ptr(out), _stream(), q[2], q[3], out.numel()),
              "tf_middle_accept_n_cur")


def _invcdf_host(probs, u):
    """block_sample<false> in torch: the first index of non-zero mass whose inclusive cumulative sum exceeds u * total (the
    last non-zero index when rounding takes u * total past the end)."""
    c = torch.cumsum(probs, 0)
    hit = ((probs > 0) & (c > u * c[-1])).nonzero()
    if hit.numel():
        return int(hit[0])
    nz = (probs > 0).nonzero()
    return int(nz[-1]) if nz.numel() else 0


def middle_accept_host(p, q_d, tokens, ubuf, cursor, n, gamma, out):
    """tf_middle_accept_cur restated in torch for CPU tensors (same reads, same writes, same record)."""
    at = int(cursor[0])
    d = int(tokens[n + 1])
    ratio = p[n, d] / q_d[d]                                   # (0 / 0 = NaN: every comparison with it is False -> rejected)
    m = ratio if bool(ratio != ratio) else torch.clamp(ratio, max=1.0)
    acc = int(bool(ubuf[at + 1] < m))
    b = _invcdf_host(p[n + acc], ubuf[at + 2])
    limit = gamma + 1 if tokens.numel() >= gamma + 2 else gamma
    if n + 1 + acc <= limit:
        tokens[n + 1 + acc] = b
    cursor[0] = at + 3
    out[:4] = torch.tensor([acc, b, d, at], dtype=torch.int64)


def middle_accept2_host(p, q1, q3, tokens, ubuf, cursor, n, gamma, out, depth=2):
    """tf_middle_accept2_cur restated in torch for CPU tensors (the two-row form of middle_accept_n_host)."""
    return middle_accept_n_host(p, (q1, q3), tokens, ubuf, cursor, n, gamma, out, depth)


def middle_accept_n_host(p, qs, tokens, ubuf, cursor, n, gamma, out, depth):
    """tf_middle_accept_n_cur restated in torch for CPU tensors: a loop over stages, each one the single-stage arithmetic of
    middle_accept_host at position n + 2 s with the uniforms behind cursor + 3 s; the token and the cursor are written once,
    for the last stage that ran."""
    at = int(cursor[0])
    limit = gamma + 1 if tokens.numel() >= gamma + 2 else gamma
    stages = []
    for s in range(depth):
        pos = n + 2 * s
        d = int(tokens[pos + 1])
        ratio = p[pos, d] / qs[s][d]
        m = ratio if bool(ratio != ratio) else torch.clamp(ratio, max=1.0)
        acc = int(bool(ubuf[at + 3 * s + 1] < m))
        b = _invcdf_host(p[pos + acc], ubuf[at + 3 * s + 2])
        stages.append((acc, b, d))
        if not (s + 1 < depth and acc == 1 and b == int(tokens[pos + 2])):
            break
    acc, b, _ = stages[-1]
    if pos + 1 + acc <= limit:
        tokens[pos + 1 + acc] = b
    cursor[0] = at + 3 * len(stages)
    rec = list(stages[0]) + [at, len(stages) - 1]
    for s in range(1, depth):
        rec += list(stages[s]) if s < len(stages) else [0, 0, 0]
    out[:len(rec)] = torch.tensor(rec, dtype=torch.int64)


def accept_chain_cur(p, q, tokens, ubuf, cursor, g2, inclusive, eos_token_id, out):
    """accept_chain over ubuf[cursor ...]; cursor += the numbers consumed (out[3])."""
    _dev(p, q, tokens, ubuf, cursor)
    _dev_or_pinned(out)
    V = p.shape[-1]
    assert p.dtype == torch.float32 and p.is_contiguous() and p.shape[0] >= g2 + 1
    assert q.dtype == torch.float32 and q.is_contiguous() and q.shape[0] >= g2 and q.shape[-1] == V
    assert tokens.dtype == torch.int64 and tokens.numel() >= g2 and out.dtype == torch.int64 and out.numel() >= 4
    assert ubuf.dtype == torch.float32 and cursor.dtype == torch.int64
    hip.check(hip.lib().tf_accept_chain_cur(_ptr(p), _ptr(q), _ptr(tokens), _ptr(ubuf), _ptr(cursor), int(g2), V,
                                            1 if inclusive else 0, int(eos_token_id), _ptr(out), _stream()),
              "tf_accept_chain_cur")


def accept_chain_step(p, q, tok_buf, ubuf, cursor, g2, inclusive, eos_token_id, pad, s_src, sets, out):
    """accept_chain_cur over tok_buf[1:] that also writes the pass tokens into tok_buf and, for each (pos, slot, sk, qlen) in
    ``sets`` (<= 2), the next target verify's positions / append slot / key count (include/triforce_hip.h)."""
    _dev(p, q, tok_buf, ubuf, cursor, s_src)
    _dev_or_pinned(out)
    V = p.shape[-1]
    assert p.dtype == torch.float32 and p.is_contiguous() and p.shape[0] >= g2 + 1
    assert q.dtype == torch.float32 and q.is_contiguous() and q.shape[0] >= g2 and q.shape[-1] == V
    assert tok_buf.dtype == torch.int64 and tok_buf.is_contiguous() and tok_buf.numel() >= g2 + 2
    assert out.dtype == torch.int64 and out.numel() >= 4 and s_src.dtype == torch.int32 and len(sets) <= 2
    flat = []
    for pos, slot, sk, qlen in list(sets) + [(None, None, None, 0)] * (2 - len(sets)):
        assert pos is None or (pos.dtype == torch.int64 and pos.is_contiguous() and slot.dtype == torch.int32 and sk.dtype == torch.int32)
        flat += [_ptr(pos), 0 if pos is None else pos.numel(), _ptr(slot), _ptr(sk), int(qlen)]
    hip.check(hip.lib().tf_accept_chain_step(_ptr(p), _ptr(q), _ptr(tok_buf), tok_buf.numel(), _ptr(ubuf), _ptr(cursor), int(g2), V,
                                             1 if inclusive else 0, int(eos_token_id), int(pad), _ptr(s_src), len(sets), *flat,
                                             _ptr(out), _stream()), "tf_accept_chain_step")


def kv_h2d_async(dst_dev, src_host, n_tokens, stream):
    """Pinned host (H,T,D) -> device (H,T',D): tokens [0, n_tokens) of every head, on `stream` (a torch Stream)."""
    _dev(dst_dev)
    H, _, D = dst_dev.shape
    assert src_host.shape[0] == H and src_host.shape[2] == D and src_host.dtype == _HALF and not src_host.is_cuda
    hip.check(hip.lib().tf_kv_h2d_async(_ptr(dst_dev), dst_dev.stride(0), _ptr(src_host), src_host.stride(0),
                                        int(n_tokens) * D, H, ctypes.c_void_p(stream.cuda_stream)), "tf_kv_h2d_async")


def kv_d2h_async(dst_host, src_dev, t0, n_tokens, stream):
    """Device (H,T',D) tokens [t0, t0+n) -> pinned host (H,T,D) same token range, on `stream`."""
    _dev(src_dev)
    H, _, D = src_dev.shape
    assert dst_host.shape[0] == H and dst_host.shape[2] == D and dst_host.dtype == _HALF and not dst_host.is_cuda
    dst = ctypes.c_void_p(dst_host.data_ptr() + int(t0) * D * 2)
    src = ctypes.c_void_p(src_dev.data_ptr() + int(t0) * D * 2)
    hip.check(hip.lib().tf_kv_d2h_async(dst, dst_host.stride(0), src, src_dev.stride(0), int(n_tokens) * D, H,
                                        ctypes.c_void_p(stream.cuda_stream)), "tf_kv_d2h_async")
