"""FP8 KV cache (TRIFORCE_KV_CACHE=fp8) without a GPU: the host restatement of the numerics contract
(include/triforce_hip.h "FP8 KV CACHE"), the knob, the refusals of the tiers that do not implement it, and the shape gate of
the C ABI entry points."""
import ctypes

import pytest
import torch

ENV = "TRIFORCE_KV_CACHE"


def _ops():
    from triforce_amd import ops
    return ops


def _all_fp16():
    v = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    return v[torch.isfinite(v)]


def _row(lead, vals):
    """Rows of 128: `lead` first, then `vals` (zero-padded)."""
    n = (vals.numel() + 126) // 127
    pad = torch.zeros(n * 127, dtype=torch.float16)
    pad[:vals.numel()] = vals
    return torch.cat([torch.full((n, 1), float(lead), dtype=torch.float16), pad.view(n, 127)], dim=1)


def test_exponent_is_the_smallest_that_covers_the_row_max():
    ops = _ops()
    a = _all_fp16().abs().unique()
    x = torch.zeros(a.numel(), 128, dtype=torch.float16)
    x[:, 3] = a
    _, b, _ = ops.kv_quantize_ref(x)
    e = b.long() - 127
    af = a.double()
    ok = 448.0 * torch.pow(2.0, e.double()) >= af                 # covers (or e is clamped at 7)
    assert bool((ok | (e == 7)).all())
    smaller = 448.0 * torch.pow(2.0, e.double() - 1) < af           # e - 1 does not (or e is clamped at -15)
    assert bool((smaller | (e == -15)).all())
    assert int(e.min()) == -15 and int(e.max()) == 7


def test_exponent_clamps_and_zero_rows():
    ops = _ops()
    x = torch.zeros(4, 128, dtype=torch.float16)
    x[1, 0] = 2.0 ** -24                                           # the smallest subnormal: e = -15
    x[2, 5] = 65504.0                                              # above 448 * 2^7: e = 7, saturates
    x[3, 7] = -57344.0                                             # exactly 448 * 2^7
    codes, b, deq = ops.kv_quantize_ref(x)
    assert (b.long() - 127).tolist() == [-15, -15, 7, 7]
    assert int(codes.view(torch.uint8)[0].max()) == 0
    assert float(deq[2, 5]) == 57344.0 and float(deq[3, 7]) == -57344.0
    assert codes.view(torch.uint8)[2, 5] == 0x7E                    # 448: the largest finite e4m3fn code, never NaN


def test_codes_round_to_nearest_even():
    ops = _ops()
    # e = 0 (row max 448): between 256 and 288 the e4m3 spacing is 32, 272 is a tie -> 256 (even mantissa); 304 -> 320
    x = torch.zeros(1, 128, dtype=torch.float16)
    x[0, :4] = torch.tensor([448.0, 272.0, 304.0, -272.0])
    _, b, deq = ops.kv_quantize_ref(x)
    assert int(b[0]) == 127
    assert deq[0, :4].tolist() == [448.0, 256.0, 320.0, -256.0]
    # subnormal range at e = -15: codes step 2^-9 -> values step 2^-24; 1.5 * 2^-24 is a tie -> 2 * 2^-24
    x = torch.zeros(1, 128, dtype=torch.float16)
    x[0, :3] = torch.tensor([2.0 ** -24, 3 * 2.0 ** -24, 0.0]).half()
    _, b, deq = ops.kv_quantize_ref(x)
    assert int(b[0]) == 127 - 15 and deq[0, :2].tolist() == [2.0 ** -24, 3 * 2.0 ** -24]


def test_dequantization_is_exact_in_fp16_over_every_value_and_exponent():
    """deq = fp16(code) * 2^e computed in fp64 equals the fp16 result for every finite fp16 input at every exponent, and
    the error is at most half an e4m3 spacing at that exponent (saturation excepted)."""
    ops = _ops()
    allv = _all_fp16()
    for e in range(-15, 8):
        lead = 448.0 * 2.0 ** e
        vals = allv[allv.abs() <= lead]
        x = _row(lead, vals)
        codes, b, deq = ops.kv_quantize_ref(x)
        assert bool((b.long() - 127 == e).all()), e
        exact = codes.double() * 2.0 ** e
        assert torch.equal(exact, deq.double()), f"deq not exact in fp16 at e = {e}"
        xd = x.double()
        # e4m3 spacing of |x| / 2^e: 2^(floor(log2) - 3), 2^-9 in the subnormal range
        m = (xd.abs() / 2.0 ** e).clamp(min=2.0 ** -6)
        sp = torch.pow(2.0, torch.floor(torch.log2(m)) - 3) * 2.0 ** e
        assert bool(((deq.double() - xd).abs() <= sp / 2).all()), f"error above half a spacing at e = {e}"
    # saturation: everything above 57 344 maps to +-57 344
    x = _row(65504.0, allv)
    _, b, deq = ops.kv_quantize_ref(x)
    assert bool((b == 134).all()) and float(deq.abs().max()) == 57344.0


def test_knob_parsing(monkeypatch):
    from triforce_amd.models import cache as C
    monkeypatch.delenv(ENV, raising=False)
    assert C.kv_cache_dtype() == "fp16"
    monkeypatch.setenv(ENV, "FP8")
    assert C.kv_cache_dtype() == "fp8"
    assert C.kv_cache_dtype("fp16") == "fp16"                      # the keyword overrides the environment
    monkeypatch.setenv(ENV, "int4")
    with pytest.raises(ValueError, match=ENV):
        C.kv_cache_dtype()
    with pytest.raises(ValueError, match=ENV):
        C.kv_cache_dtype("bf16")


def test_fp8_needs_the_fused_decode_layer(monkeypatch):
    from triforce_amd.models import cache as C
    monkeypatch.setenv(ENV, "fp8")
    monkeypatch.setattr(C.ops, "FUSE_MODE", "none")
    with pytest.raises(ValueError, match="TRIFORCE_FUSE"):
        C.kv_cache_dtype()


class _Cfg:
    num_key_value_heads = num_attention_heads = 4
    hidden_size = 512
    num_hidden_layers = 2
    world_size, local_rank = 1, 0


class _Model:
    config = _Cfg()
    device = torch.device("cpu")


def test_offloading_and_distributed_caches_refuse_fp8(monkeypatch):
    from triforce_amd.models import cache as C
    monkeypatch.setenv(ENV, "fp8")
    with pytest.raises(NotImplementedError, match=ENV):
        C.OffloadingFlashSimpleCache(_Model(), 64)
    with pytest.raises(NotImplementedError, match=ENV):
        C.DistributedSimpleCache(_Cfg(), 64, device="cpu")


def test_tensor_parallel_engine_refuses_fp8(monkeypatch):
    from triforce_amd.models.TP_llama import DistributedLlama
    monkeypatch.setenv(ENV, "fp8")
    with pytest.raises(NotImplementedError, match=ENV):
        DistributedLlama("random:0", device="cpu")


def test_fp8_cache_layout_and_refusals_on_the_host(monkeypatch):
    """The FP8 FlashSimpleCache's storage (CPU tensors suffice for the layout) and its .k / .v refusal."""
    from triforce_amd.models import cache as C

    class M128(_Model):
        class config(_Cfg):
            hidden_size = 512                                       # 4 heads x 128

    c = C.FlashSimpleCache(M128(), 96, kv_dtype="fp8")
    assert c.fp8 and c.kc.dtype == torch.float8_e4m3fn and c.kc.shape == (2, 4, 96, 128)
    assert c.ke.dtype == torch.uint8 and c.ke.shape == (2, 4, 96) and int(c.ke.min()) == 127 - 15
    assert c.stage_k.shape == (4, 32, 128) and c.scratch_k.shape == (4, 96, 128)
    assert c.key_cache.shape == (2, 1, 96, 4, 128)
    with pytest.raises(AttributeError, match=ENV):
        c.k
    with pytest.raises(AttributeError, match=ENV):
        c.v
    # codes + exponent bytes + fp16 staging (32 rows) + fp16 one-layer scratch
    assert c.nbytes() == 2 * 2 * 4 * 96 * 128 + 2 * 2 * 4 * 96 + 2 * 4 * 32 * 128 * 2 + 2 * 4 * 96 * 128 * 2
    monkeypatch.delenv(ENV, raising=False)
    d = C.FlashSimpleCache(M128(), 96)
    assert not d.fp8 and d.k.dtype == torch.float16 and d.k.shape == (2, 4, 96, 128)


def test_c_abi_shape_gate():
    """The three entry points refuse D != 128, sq > 32, misaligned strides — before any launch, so without a GPU."""
    from triforce_amd import hip
    lib = hip.lib()
    p = ctypes.c_void_p(16)                                         # non-NULL: only the shape checks can refuse
    null = ctypes.c_void_p(0)
    # tf_attn_decode_fp8_act(q, kc, vc, ke, ve, out, out_sm, out_sk, stride_t, stride_h, exp_sh, sq, sk, sk_dev, H, D, ...)
    def attn(D=128, sq=7, st=128, sh=128 * 4096, esh=4096, ws=1 << 30):
        return lib.tf_attn_decode_fp8_act(p, p, p, p, p, p, 4096, 8, st, sh, esh, sq, 4096, null, 32, D, 0.1, 8, p, ws,
                                          null, null)
    assert attn(D=64) == -22
    assert attn(sq=33) == -22 and attn(sq=0) == -22
    assert attn(st=136) == -22 and attn(sh=128 * 4096 + 8) == -22 and attn(st=64) == -22
    assert attn(esh=100) == -22
    assert attn(ws=10) == -28                                        # too small a workspace: -ENOSPC
    # tf_kv_quant_rows(k, v, in_st, in_sh, kc, vc, ke, ve, c_st, c_sh, e_sh, slot0, slot0_dev, n, H, D, kdeq, vdeq, stream)
    def quant(D=128, in_st=128, c_st=128, kdeq=null, vdeq=null, n=0):
        return lib.tf_kv_quant_rows(p, p, in_st, 4096, p, p, p, p, c_st, 4096 * 128, 4096, 0, null, n, 32, D, kdeq, vdeq, null)
    assert quant() == 0                                              # n == 0: a no-op once the arguments are valid
    assert quant(D=64) == -22 and quant(in_st=127) == -22 and quant(c_st=64) == -22
    assert quant(kdeq=p) == -22                                      # deq outputs: both or neither
    # tf_kv_dequant_rows_pair(sk, sv, ssl, sst, ssh, ek, ev, esl, esh, dk, dv, dsl, dst, dsh, s0, d0, n, L, H, D, stream)
    def deq(D=128, sst=128, dst_t=128):
        return lib.tf_kv_dequant_rows_pair(p, p, 1 << 24, sst, 1 << 19, p, p, 1 << 17, 4096, p, p, 1 << 24, dst_t, 1 << 19, 0,
                                           0, 0, 2, 32, D, null)
    assert deq() == 0 and deq(D=64) == -22 and deq(sst=120) == -22 and deq(dst_t=132) == -22
