"""FP8 weights of the retrieval-verify tier (TRIFORCE_RETRIEVAL_WEIGHTS=fp8) without a GPU: the host
quantizer against the numerics contract of include/triforce_hip.h, the packing as a pure permutation, the argument checks
of the C ABI (nothing is launched), the knob, and the gfx950 build of the kernels."""
import ctypes
import os
import re
import shutil

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4M3 = torch.float8_e4m3fn


def _ops():
    from triforce_amd import ops
    return ops


def _finite_codes():
    """Every e4m3fn code but the two NaNs (0x7f, 0xff)."""
    return torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)


def _spacing(v):
    """e4m3fn spacing at magnitude v (3 mantissa bits; subnormals below 2^-6 step 2^-9)."""
    v = v.abs().double()
    e = torch.floor(torch.log2(torch.clamp(v, min=2.0 ** -6)))
    return torch.pow(2.0, e - 3)


def test_code_table_round_trips_through_the_quantizer():
    ops = _ops()
    codes = _finite_codes()
    vals = codes.view(E4M3).float()
    assert float(vals.abs().max()) == 448.0
    # one row holding every finite value: amax = 448 -> s = 1 exactly, and every value quantizes to itself
    q, s = ops.quantize_fp8_rows(vals.half().view(1, -1))
    assert s.dtype == torch.float32 and float(s[0]) == 1.0
    got = q[0]
    neg_zero = codes == 0x80
    assert torch.equal(got[~neg_zero], codes[~neg_zero])
    assert float(got[neg_zero].view(E4M3).float()[0]) == 0.0
    # the fp16 tensor holds every e4m3fn value exactly
    assert torch.equal(vals.half().float(), vals)


def test_round_to_nearest_even_at_the_midpoints():
    ops = _ops()
    # [1, 2): spacing 1/8.  1.0625 lies between 1.0 (mantissa 000) and 1.125 (001): even -> 1.0; 1.1875 between 1.125 and
    # 1.25 (010): even -> 1.25.  [256, 448]: spacing 32; 272 between 256 (000) and 288 (001) -> 256, 304 -> 320 (010).
    # subnormals step 2^-9: 1.5 * 2^-9 between 2^-9 (001) and 2^-8 (010) -> 2^-8.
    x = torch.tensor([448.0, 1.0625, 1.1875, -1.0625, -1.1875, 272.0, 304.0, 1.5 * 2 ** -9, 0.5 * 2 ** -9])
    want = torch.tensor([448.0, 1.0, 1.25, -1.0, -1.25, 256.0, 320.0, 2 ** -8, 0.0])
    q, s = ops.quantize_fp8_rows(x.view(1, -1))
    assert float(s[0]) == 1.0
    assert torch.equal(q[0].view(E4M3).float(), want)


def test_values_past_448_are_clamped_not_nan():
    ops = _ops()
    # the hazard: this torch turns an out-of-range value into NaN when it casts to e4m3fn
    assert torch.isnan(torch.tensor([500.0]).to(E4M3).float()).all()
    # the quantizer clamps W / s to +-448 before the cast: W / s can land a rounding above 448 for the row's amax
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(512, 96, generator=g) * torch.rand(512, 1, generator=g) * 30).half()
    w[0, 0], w[1, 3] = 500.0, -60000.0
    q, s = ops.quantize_fp8_rows(w)
    dq = q.view(E4M3).float()
    assert not torch.isnan(dq).any()
    assert torch.equal(dq.abs().amax(dim=1), torch.full((512,), 448.0))    # every row's amax maps to the top code
    assert float(dq[0, 0]) == 448.0 and float(dq[1, 3]) == -448.0


def test_zero_rows_get_scale_one():
    ops = _ops()
    w = torch.zeros(4, 64, dtype=torch.float16)
    w[2, 7] = 3.0
    q, s = ops.quantize_fp8_rows(w)
    assert torch.equal(s, torch.tensor([1.0, 1.0, 3.0 / 448.0, 1.0]))
    assert int(q[[0, 1, 3]].view(E4M3).float().abs().sum()) == 0


@pytest.mark.parametrize("std", [0.02, 1.0, 1e-4])
def test_dequantized_values_lie_within_half_a_spacing(std):
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    w = (torch.randn(256, 320, generator=g) * std).half()
    w[3] = 0
    w[7, 5] = 40 * std                                   # an outlier row: most of it lands in the subnormal codes
    q, s = ops.quantize_fp8_rows(w)
    assert q.dtype == torch.uint8 and q.shape == w.shape and s.shape == (256,)
    dq = ops.dequantize_fp8_rows(q, s).double()
    v = w.double() / s.double()[:, None]
    err = (dq - w.double()).abs()
    # half an e4m3 spacing at |W / s|, times s — plus the fp32 rounding of the quotient W / s the contract casts (a few ulp)
    bound = (0.5 * _spacing(v) + 2.0 ** -21 * v.abs()) * s.double()[:, None]
    assert (err <= bound * (1 + 1e-9)).all(), float((err / bound).max())
    assert torch.equal(s, (w.float().abs().amax(dim=1) / 448.0).where(w.float().abs().amax(dim=1) > 0, torch.ones(256)))


def test_pack_weight_fp8_is_a_pure_permutation():
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    N, K = 48, 192
    codes = torch.randint(0, 256, (N, K), generator=g, dtype=torch.int32).to(torch.uint8)
    p = ops.pack_weight_fp8(codes)
    assert p.shape == (N // 16, K // 64, 4, 16, 16) and p.is_contiguous()
    assert torch.equal(ops.unpack_weight_fp8(p), codes)
    assert torch.equal(torch.sort(p.reshape(-1)).values, torch.sort(codes.reshape(-1)).values)
    # piece (g, i) of super-chunk s of panel P: row 16P+i, k-octet g of chunk 2s (bytes 0-7), then of chunk 2s+1 (bytes 8-15)
    for P, sc, gg, i in ((0, 0, 0, 0), (1, 2, 3, 15), (2, 1, 2, 7)):
        n, k0 = 16 * P + i, 64 * sc + 8 * gg
        assert torch.equal(p[P, sc, gg, i, :8], codes[n, k0:k0 + 8])
        assert torch.equal(p[P, sc, gg, i, 8:], codes[n, k0 + 32:k0 + 40])
    # one 16x64 tile is one contiguous KiB
    flat = p.reshape(-1)
    assert torch.equal(flat[1024:2048].view(4, 16, 16), p[0, 1])
    with pytest.raises(AssertionError):
        ops.pack_weight_fp8(codes[:, :160])                # K % 64


def test_fp8_entry_points_reject_bad_arguments_before_launching():
    """TF_EINVAL for NULL scales, K % 64, N % 16 and M > 32 — the pointers below are never dereferenced (no launch)."""
    from triforce_amd import hip
    lib = hip.lib()
    P = ctypes.c_void_p(4096)
    N0 = ctypes.c_void_p(0)

    def gemm(scale=P, M=4, N=64, K=128, x_sk=8):
        return lib.tf_skinny_gemm_fp8_act(P, scale, P, K, x_sk, N0, 0.0, N0, N0, 8, 8, N0, P, N, 8, M, N, K, 0, N0)

    def swiglu(gs=P, us=P, M=4, I=64, K=128):
        return lib.tf_skinny_gemm_swiglu_fp8_act(P, gs, P, us, P, K, 8, N0, 0.0, N0, P, I, 8, M, I, K, N0)

    def qkv(scale=P, M=4, H=2, D=64, K=128):
        return lib.tf_skinny_qkv_rope_fp8_act(P, scale, P, K, 8, N0, 0.0, N0, P, P, P, P, P, P, 64, 64 * 64, 0, N0, M, H, D,
                                              K, 1, N0)

    for rc in (gemm(scale=N0), gemm(K=96), gemm(K=32), gemm(N=40), gemm(M=33), gemm(M=0), gemm(x_sk=4),
               swiglu(gs=N0), swiglu(us=N0), swiglu(K=160), swiglu(I=24), swiglu(M=33),
               qkv(scale=N0), qkv(K=96), qkv(M=33), qkv(D=48)):
        assert rc == -22
    # out_f32 with a residual / ss_out, ss_in without a norm weight
    assert lib.tf_skinny_gemm_fp8_act(P, P, P, 128, 8, N0, 0.0, N0, P, 8, 8, N0, P, 64, 8, 4, 64, 128, 1, N0) == -22
    assert lib.tf_skinny_gemm_fp8_act(P, P, P, 128, 8, N0, 0.0, P, N0, 8, 8, N0, P, 64, 8, 4, 64, 128, 0, N0) == -22


def test_fp8_holder_needs_a_device_tensor():
    from triforce_amd import hip
    ops = _ops()
    pl = ops.PackedLinear(torch.zeros(64, 128, dtype=torch.float16), pack=False)
    assert pl.fp8 is None
    with pytest.raises(hip.TriforceHipError):
        ops.Fp8Linear(pl)


def test_retrieval_weights_knob(monkeypatch):
    from triforce_amd.models import llama_core as C
    ops = _ops()
    monkeypatch.delenv("TRIFORCE_RETRIEVAL_WEIGHTS", raising=False)
    assert C.retrieval_weights() == "fp16"
    monkeypatch.setenv("TRIFORCE_RETRIEVAL_WEIGHTS", "fp8")
    monkeypatch.setattr(ops, "FUSE_MODE", "all")
    assert C.retrieval_weights() == "fp8"
    monkeypatch.setattr(ops, "FUSE_MODE", "none")
    with pytest.raises(ValueError, match="TRIFORCE_FUSE"):
        C.retrieval_weights()
    monkeypatch.setattr(ops, "FUSE_MODE", "all")
    monkeypatch.setenv("TRIFORCE_RETRIEVAL_WEIGHTS", "int4")
    with pytest.raises(ValueError):
        C.retrieval_weights()


def test_fusion_switch_is_two_valued(monkeypatch):
    ops = _ops()
    monkeypatch.delenv("TRIFORCE_FUSE", raising=False)
    assert ops.fuse_mode() == "all"
    monkeypatch.setenv("TRIFORCE_FUSE", "none")
    assert ops.fuse_mode() == "none"
    monkeypatch.setenv("TRIFORCE_FUSE", "rope")                     # a retired level: refused, not read as "none"
    with pytest.raises(ValueError, match="all or none"):
        ops.fuse_mode()


def test_tensor_parallel_engine_refuses_fp8(monkeypatch):
    from triforce_amd.models.TP_llama import DistributedLlama
    monkeypatch.setenv("TRIFORCE_RETRIEVAL_WEIGHTS", "fp8")
    with pytest.raises(NotImplementedError, match="TRIFORCE_RETRIEVAL_WEIGHTS"):
        DistributedLlama("random:0", config=None, device="cpu")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_fp8_kernels_compile_for_gfx950_with_f16_mfma_and_exact_decode():
    """Built with the library's flags: every FP8 form decodes with v_cvt_scalef32_pk_f16_fp8 and multiplies on the f16 MFMA
    (weight-only: no fp8 x fp8 or MX-scaled MFMA, which would quantize the activations), without register spills."""
    from tools import isa_lint
    from triforce_amd.build import FLAGS, SOURCES
    assert "gemv_fp8.hip" in SOURCES
    extra = [f for f in FLAGS if f == "-mllvm" or f.startswith("-amdgpu-")]
    text = isa_lint.compile_to_asm(os.path.join(ROOT, "triforce_amd", "csrc", "gemv_fp8.hip"), extra=extra)
    kernels = re.findall(r"\.name:\s+(_Z22skinny_gemm_fp8_kernel\S+)", text)
    assert len(kernels) >= 16, kernels[:4]          # {1, 2 row tiles} x {plain, gate|up, f32, q|k|v} x {norm or not} x waves
    assert "v_cvt_scalef32_pk_f16_fp8" in text and "v_mfma_f32_16x16x32_f16" in text
    mfmas = set(re.findall(r"\b(v_mfma_\w+)", text))
    assert mfmas == {"v_mfma_f32_16x16x32_f16"}, mfmas
    spills = re.findall(r"\.name:\s+(_Z22skinny_gemm_fp8_kernel\S+)[\s\S]*?\.vgpr_spill_count:\s+(\d+)", text)
    assert spills and all(int(n) == 0 for _, n in spills)
