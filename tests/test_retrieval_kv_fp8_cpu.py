"""FP8 storage of the retrieval cache (TRIFORCE_RETRIEVAL_KV=fp8) without a GPU: the knob, the storage it
allocates and the storage it leaves alone, the refusals, the host restatement of the gather, and the argument gates of the three
C ABI entry points (include/triforce_hip.h "FP8 RETRIEVAL CACHE")."""
import ctypes

import pytest
import torch

ENV = "TRIFORCE_RETRIEVAL_KV"


class _Cfg:
    num_key_value_heads = num_attention_heads = 4
    hidden_size = 512                                               # 4 heads x 128
    num_hidden_layers = 2
    world_size, local_rank = 1, 0


class _Model:
    config = _Cfg()
    device = torch.device("cpu")


def test_knob_parsing(monkeypatch):
    from triforce_amd.models import cache as C
    monkeypatch.delenv(ENV, raising=False)
    assert C.retrieval_kv_dtype() == "fp16"
    monkeypatch.setenv(ENV, " FP8 ")
    assert C.retrieval_kv_dtype() == "fp8"
    assert C.retrieval_kv_dtype("fp16") == "fp16"                   # the keyword overrides the environment
    monkeypatch.setenv(ENV, "")
    assert C.retrieval_kv_dtype() == "fp16"
    monkeypatch.setenv(ENV, "int4")
    with pytest.raises(ValueError, match=ENV):
        C.retrieval_kv_dtype()
    with pytest.raises(ValueError, match=ENV):
        C.retrieval_kv_dtype("bf16")
    with pytest.raises(ValueError, match=ENV):
        C.RetrievalCache(_Model(), 64, 128)
    assert not C.RetrievalCache(_Model(), 64, 128, kv_dtype="fp16").fp8


def test_fp8_needs_the_fused_decode_layer(monkeypatch):
    from triforce_amd.models import cache as C
    monkeypatch.setattr(C.ops, "FUSE_MODE", "none")
    monkeypatch.setenv(ENV, "fp8")
    with pytest.raises(ValueError, match="TRIFORCE_FUSE"):
        C.retrieval_kv_dtype()
    with pytest.raises(ValueError, match="TRIFORCE_FUSE"):
        C.RetrievalCache(_Model(), 64, 128)
    monkeypatch.delenv(ENV)
    with pytest.raises(ValueError, match="TRIFORCE_FUSE"):
        C.RetrievalCache(_Model(), 64, 128, kv_dtype="fp8")
    assert not C.RetrievalCache(_Model(), 64, 128).fp8              # fp16 does not need it


def test_unset_knob_allocates_exactly_the_parents_tensors(monkeypatch):
    from triforce_amd.models import cache as C
    monkeypatch.delenv(ENV, raising=False)
    c = C.RetrievalCache(_Model(), max_budget=64, prefill=128, chunk_size=8, gamma=6)
    tensors = {k: v for k, v in vars(c).items() if torch.is_tensor(v)}
    assert sorted(tensors) == ["k", "key_cache", "v", "value_cache"]
    assert c.k.shape == c.v.shape == (2, 4, 71, 128) and c.k.dtype == torch.float16
    assert c.key_cache.shape == (2, 1, 71, 4, 128) and c.key_cache.data_ptr() == c.k.data_ptr()
    assert not c.fp8 and c.spec_slot == 64 and c.nbytes() == 2 * 2 * 4 * 71 * 128 * 2
    assert c.layer_kv(1)[0].data_ptr() == c.k[1].data_ptr()
    for name in ("kc", "vc", "ke", "ve", "spec_k", "spec_v"):
        with pytest.raises(AttributeError):
            getattr(c, name)


def test_fp8_storage_layout_and_the_k_v_refusal(monkeypatch):
    from triforce_amd.models import cache as C
    monkeypatch.setenv(ENV, "fp8")
    c = C.RetrievalCache(_Model(), max_budget=64, prefill=128, chunk_size=8, gamma=6)
    assert c.fp8 and c.real_budget == 71
    assert c.kc.dtype == c.vc.dtype == torch.float8_e4m3fn and c.kc.shape == c.vc.shape == (2, 4, 64, 128)
    assert c.ke.dtype == torch.uint8 and c.ke.shape == c.ve.shape == (2, 4, 64) and int(c.ke.min()) == 127 - 15
    assert c.spec_k.dtype == torch.float16 and c.spec_k.shape == c.spec_v.shape == (2, 4, 7, 128)
    assert c.key_cache.shape == (2, 1, 64, 4, 128)
    for name in ("k", "v"):
        with pytest.raises(AttributeError, match=ENV):
            getattr(c, name)
    k, v = c.layer_kv(1)                                            # what the spec branch appends to
    assert k.data_ptr() == c.spec_k[1].data_ptr() and v.data_ptr() == c.spec_v[1].data_ptr() and k.shape == (4, 7, 128)
    codes = c.layer_codes(1)
    assert [t.data_ptr() for t in codes] == [c.kc[1].data_ptr(), c.vc[1].data_ptr(), c.ke[1].data_ptr(), c.ve[1].data_ptr()]
    # codes + exponent bytes + the fp16 spec rows
    assert c.nbytes() == 2 * (2 * 4 * 64 * 128) + 2 * (2 * 4 * 64) + 2 * (2 * 4 * 7 * 128 * 2)
    c.kc.view(torch.uint8).fill_(3)
    c.ke.fill_(130)
    c.spec_k.fill_(1.0)
    c.reanchor(136)
    c.reset()
    assert int(c.kc.view(torch.uint8).max()) == 0 and int(c.ke.max()) == 127 - 15 and float(c.spec_k.abs().max()) == 0
    assert c.prefill == 128
    # the keyword wins over the environment, both ways
    assert not C.RetrievalCache(_Model(), 64, 128, kv_dtype="fp16").fp8
    monkeypatch.delenv(ENV)
    assert C.RetrievalCache(_Model(), 64, 128, kv_dtype="fp8").fp8


def test_nbytes_ratio_at_the_configs1_geometry():
    """Budget 4 096, gamma 6, D = 128: codes + exponents + fp16 spec rows take 0.505 x the fp16 K + V."""
    from triforce_amd.models import cache as C

    class M1(_Model):
        class config(_Cfg):
            num_key_value_heads = num_attention_heads = 1
            hidden_size = 128
            num_hidden_layers = 1

    f8 = C.RetrievalCache(M1(), 4096, 4096, gamma=6, kv_dtype="fp8").nbytes()
    f16 = C.RetrievalCache(M1(), 4096, 4096, gamma=6, kv_dtype="fp16").nbytes()
    assert f16 == 2 * 4103 * 128 * 2 and f8 == 2 * 4096 * 128 + 2 * 4096 + 2 * 7 * 128 * 2
    assert f8 <= 0.52 * f16 and 0.504 < f8 / f16 < 0.506


def test_head_dim_other_than_128_is_refused():
    from triforce_amd.models import cache as C

    class M64(_Model):
        class config(_Cfg):
            hidden_size = 256                                       # 4 heads x 64

    with pytest.raises(NotImplementedError, match=ENV):
        C.RetrievalCache(M64(), 64, 128, kv_dtype="fp8")
    assert C.RetrievalCache(M64(), 64, 128, kv_dtype="fp16").k.shape[-1] == 64


def test_distributed_retrieval_caches_refuse(monkeypatch):
    from triforce_amd.models import cache as C
    monkeypatch.setenv(ENV, "fp8")
    with pytest.raises(NotImplementedError, match=ENV):
        C.DistributedRetrievalCache(_Cfg(), 64, device="cpu", prefill=128)
    with pytest.raises(NotImplementedError, match=ENV):
        C.DistributedRetrievalCache_Seqouia(_Cfg(), 64, device="cpu", prefill=128, tree_size=16)
    monkeypatch.delenv(ENV)
    assert C.DistributedRetrievalCache(_Cfg(), 64, device="cpu", prefill=128).k.shape == (2, 4, 71, 128)


def test_tensor_parallel_engine_refuses(monkeypatch):
    from triforce_amd.models.TP_llama import DistributedLlama
    monkeypatch.setenv(ENV, "fp8")
    with pytest.raises(NotImplementedError, match=ENV):
        DistributedLlama("random:0", device="cpu")


def test_spec_branch_appends_to_the_fp16_spec_rows():
    """What the spec branch gets from _kv_view: the fp16 spec rows at slot 0 under FP8, the parent's views and slot otherwise."""
    from triforce_amd.models import cache as C
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    c = C.RetrievalCache(_Model(), 64, 128, gamma=6, kv_dtype="fp8")
    kl, vl, slot, sk, codes = LlamaForCausalLM._kv_view(0, 7, True, None, c, None)
    assert (slot, sk, codes) == (0, 71, None) and kl.data_ptr() == c.spec_k[0].data_ptr()
    d = C.RetrievalCache(_Model(), 64, 128, gamma=6, kv_dtype="fp16")
    assert LlamaForCausalLM._kv_view(0, 7, True, None, d, None)[2:] == (64, 71, None)


# ---- the gather's host restatement ---------------------------------------------------------------------------------------
def test_gather_restatement_is_the_row_quantizer_on_the_gathered_rows():
    from triforce_amd import ops
    H, chunk, C, D = 2, 4, 6, 128
    g = torch.Generator().manual_seed(1)
    k = torch.randn(H, C * chunk, D, generator=g).half()
    v = torch.randn(H, C * chunk, D, generator=g).half()
    # hand-made rows in chunk 3 of head 0: all zero; saturating; a rounding tie under a 448 lead (272 -> 256, 304 -> 320)
    k[0, 12] = 0
    k[0, 13] = 0
    k[0, 13, 5] = 65504.0
    k[0, 13, 6] = -60000.0
    k[0, 14] = 0
    k[0, 14, :4] = torch.tensor([448.0, 272.0, 304.0, -272.0])
    idx = torch.tensor([[0, 3, 1], [0, 5, 2]], dtype=torch.int32)     # chunk 0 in slot 0, non-monotone
    kc, vc, ke, ve = ops.retrieval_gather_fp8_ref(k, v, idx, chunk)
    assert kc.shape == vc.shape == (H, 12, D) and ke.shape == ve.shape == (H, 12) and kc.dtype == torch.float8_e4m3fn
    for h in range(H):
        for s, c in enumerate(idx[h].tolist()):
            for src, codes, ex in ((k, kc, ke), (v, vc, ve)):
                rc, re_, _ = ops.kv_quantize_ref(src[h, c * chunk:(c + 1) * chunk])
                assert torch.equal(codes[h, s * chunk:(s + 1) * chunk].view(torch.uint8), rc.view(torch.uint8))
                assert torch.equal(ex[h, s * chunk:(s + 1) * chunk], re_)
    # the hand-made rows sit in slot 1 of head 0: rows 4, 5, 6 of the gathered layer
    assert int(ke[0, 4]) == 127 - 15 and int(kc[0, 4].view(torch.uint8).max()) == 0
    assert int(ke[0, 5]) == 127 + 7 and kc[0, 5].view(torch.uint8)[5] == 0x7E and kc[0, 5].view(torch.uint8)[6] == 0xFE
    assert int(ke[0, 6]) == 127 and kc[0, 6, :4].float().tolist() == [448.0, 256.0, 320.0, -256.0]


# ---- C ABI gates ---------------------------------------------------------------------------------------------------------
EINVAL, ENOSPC = -22, -28


def test_c_abi_gates_of_the_attention():
    from triforce_amd import hip
    lib = hip.lib()
    p, null = ctypes.c_void_p(16), ctypes.c_void_p(0)

    def attn(q=p, kc=p, ke=p, kt=p, vt=p, out=p, ws=p, D=128, sq=7, st=128, sh=128 * 4096, esh=4096, tst=128, tsh=7 * 128,
             skc=4096, nt=7, sk_dev=null, wsf=1 << 30, osm=4096, nsplit=8):
        return lib.tf_attn_decode_fp8_tail_act(q, kc, p, ke, p, kt, vt, out, osm, 8, st, sh, esh, tst, tsh, sq, skc, nt, sk_dev,
                                               32, D, 0.1, nsplit, ws, wsf, null, null)
    for name in ("q", "kc", "ke", "kt", "vt", "out", "ws"):
        assert attn(**{name: null}) == EINVAL, name
    assert attn(D=64) == EINVAL
    assert attn(sq=33) == EINVAL and attn(sq=0) == EINVAL
    assert attn(nt=33) == EINVAL and attn(nt=0) == EINVAL
    assert attn(skc=0) == EINVAL
    assert attn(esh=4095) == EINVAL                                  # exp_stride_h < sk_codes
    assert attn(st=136) == EINVAL and attn(st=64) == EINVAL and attn(sh=128 * 4096 + 8) == EINVAL
    assert attn(tst=132) == EINVAL and attn(tst=64) == EINVAL and attn(tsh=7 * 128 + 4) == EINVAL
    assert attn(osm=6) == EINVAL and attn(nsplit=0) == EINVAL and attn(nsplit=129) == EINVAL
    assert attn(sk_dev=p) == EINVAL                                  # the device key count is not supported in this form
    assert attn(wsf=10) == ENOSPC


def test_c_abi_gates_of_the_gather():
    from triforce_amd import hip
    lib = hip.lib()
    p, null = ctypes.c_void_p(16), ctypes.c_void_p(0)

    def gather(ks=p, vs=p, kse=null, vse=null, idx=p, kc=p, vc=p, ke=p, ve=p, sst=128, ssh=128 * 1024, sesh=1024, cst=128,
               csh=128 * 64, esh=64, sets=8, chunk=8, H=4, D=128):
        return lib.tf_retrieval_gather_fp8(ks, vs, sst, ssh, kse, vse, sesh, idx, kc, vc, ke, ve, cst, csh, esh, sets, chunk, H,
                                           D, null)
    for name in ("ks", "vs", "idx", "kc", "vc", "ke", "ve"):
        assert gather(**{name: null}) == EINVAL, name
    assert gather(kse=p) == EINVAL and gather(vse=p) == EINVAL       # source exponents: both or neither
    assert gather(D=64) == EINVAL and gather(sets=0) == EINVAL and gather(chunk=0) == EINVAL and gather(H=0) == EINVAL
    assert gather(esh=63) == EINVAL                                  # exp_stride_h < sets * chunk
    assert gather(sst=127) == EINVAL and gather(sst=64) == EINVAL and gather(ssh=128 * 1024 + 1) == EINVAL
    assert gather(cst=136) == EINVAL and gather(cst=64) == EINVAL and gather(csh=128 * 64 + 8) == EINVAL
    # a code source: 16-byte strides, an exponent stride
    assert gather(kse=p, vse=p, sst=136) == EINVAL and gather(kse=p, vse=p, ssh=128 * 1024 + 8) == EINVAL
    assert gather(kse=p, vse=p, sesh=0) == EINVAL


def test_c_abi_gates_of_the_tail_refresh():
    from triforce_amd import hip
    lib = hip.lib()
    p, null = ctypes.c_void_p(16), ctypes.c_void_p(0)

    def refresh(sk=p, sv=p, sek=null, sev=null, kc=p, vc=p, ke=p, ve=p, ssl=1 << 24, sst=128, ssh=1 << 19, sesl=1 << 17,
                sesh=4096, csl=1 << 20, cst=128, csh=1 << 13, esl=1 << 8, esh=64, s0=0, d0=0, n=0, L=2, H=4, D=128):
        return lib.tf_kv_quant_rows_pair(sk, sv, ssl, sst, ssh, sek, sev, sesl, sesh, kc, vc, csl, cst, csh, ke, ve, esl, esh, s0,
                                         d0, n, L, H, D, null)
    assert refresh() == 0                                            # n == 0: a no-op once the arguments are valid
    assert refresh(sek=p, sev=p) == 0
    for name in ("sk", "sv", "kc", "vc", "ke", "ve"):
        assert refresh(**{name: null}) == EINVAL, name
    assert refresh(sek=p) == EINVAL and refresh(sev=p) == EINVAL
    assert refresh(D=64) == EINVAL and refresh(n=-1) == EINVAL and refresh(L=0) == EINVAL and refresh(H=0) == EINVAL
    assert refresh(s0=-1) == EINVAL and refresh(d0=-1) == EINVAL
    assert refresh(sst=127) == EINVAL and refresh(sst=64) == EINVAL and refresh(ssl=(1 << 24) + 1) == EINVAL
    assert refresh(cst=136) == EINVAL and refresh(csl=(1 << 20) + 8) == EINVAL and refresh(esh=0) == EINVAL
    assert refresh(sek=p, sev=p, sst=136) == EINVAL and refresh(sek=p, sev=p, sesh=0) == EINVAL


def test_wrappers_refuse_host_tensors():
    """No CPU path: the three wrappers raise on host tensors instead of computing."""
    from triforce_amd import hip, ops
    f8 = torch.float8_e4m3fn
    kc, ke = torch.zeros(2, 16, 128, dtype=f8), torch.zeros(2, 16, dtype=torch.uint8)
    rows = torch.zeros(2, 16, 128, dtype=torch.float16)
    q = torch.zeros(3, 2, 128, dtype=torch.float16)
    with pytest.raises(hip.TriforceHipError):
        ops.attn_decode_fp8_tail(q, kc, kc, ke, ke, rows[:, :3], rows[:, :3], 16, 0.1)
    with pytest.raises(hip.TriforceHipError):
        ops.retrieval_gather_fp8(rows, rows, torch.zeros(2, 2, dtype=torch.int32), kc, kc, ke, ke, 8)
    with pytest.raises(hip.TriforceHipError):
        ops.kv_quant_rows_pair(rows.unsqueeze(0), rows.unsqueeze(0), kc.unsqueeze(0), kc.unsqueeze(0), ke.unsqueeze(0),
                               ke.unsqueeze(0), 0, 0, 4)


# ---- the tail refresh's launches -----------------------------------------------------------------------------------------
def test_tail_refresh_launches_for_the_four_tier_pairs(monkeypatch):
    """RetrievalCache._copy_tail over (full tier, retrieval tier): which wrapper it calls, with which rows and which storage.
    Host tensors: nothing is planned, every refresh is one recorded call."""
    from triforce_amd.models import cache as C
    L, H, B, P, T = 3, 2, 32, 64, 96

    class M(_Model):
        class config(_Cfg):
            num_key_value_heads = num_attention_heads = H
            hidden_size = H * 128
            num_hidden_layers = L

    calls = []

    def copy(src_k, src_v, dst_k, dst_v, src_t0, dst_t0, n):
        calls.append(("copy", (src_k, src_v), None, (dst_k, dst_v), src_t0, dst_t0, n))

    def dequant(src_k, src_v, exp_k, exp_v, dst_k, dst_v, src_t0, dst_t0, n):
        calls.append(("dequant", (src_k, src_v), (exp_k, exp_v), (dst_k, dst_v), src_t0, dst_t0, n))

    def quant(src_k, src_v, dst_kc, dst_vc, dst_ke, dst_ve, src_t0, dst_t0, n, src_exp=None):
        calls.append(("quant", (src_k, src_v), src_exp, (dst_kc, dst_vc, dst_ke, dst_ve), src_t0, dst_t0, n))

    monkeypatch.setattr(C.ops, "kv_copy_rows_pair", copy)
    monkeypatch.setattr(C.ops, "kv_dequant_rows_pair", dequant)
    monkeypatch.setattr(C.ops, "kv_quant_rows_pair", quant)
    operation = {("fp16", "fp16"): "copy", ("fp8", "fp16"): "dequant", ("fp16", "fp8"): "quant", ("fp8", "fp8"): "quant"}

    def ptrs(ts):
        return [t.data_ptr() for t in ts]

    for full, tier in operation:
        kv = C.FlashSimpleCache(M(), T, kv_dtype=full)
        rc = C.RetrievalCache(M(), max_budget=B, prefill=P, chunk_size=8, gamma=6, kv_dtype=tier)
        src_all = (kv.kc, kv.vc) if full == "fp8" else (kv.k, kv.v)
        exp_all = (kv.ke, kv.ve) if full == "fp8" else None
        dst_all = (rc.kc, rc.vc, rc.ke, rc.ve) if tier == "fp8" else (rc.k, rc.v)
        for g in (5, 31):
            kv.seq_len = P + g
            for layers, refresh in ((slice(0, L), lambda: rc.update_graph_cache(kv)),
                                    (slice(1, 2), lambda: rc._copy_tail(kv, slice(1, 2)))):
                del calls[:]
                refresh()
                assert len(calls) == 1, (full, tier, g, layers)
                op, src, src_exp, dst, src_t0, dst_t0, n = calls[0]
                assert op == operation[full, tier], (full, tier)
                assert (src_t0, dst_t0, n) == (P, B - g, g), (full, tier, g)
                assert ptrs(src) == ptrs(t[layers] for t in src_all) and all(t.shape[0] == layers.stop - layers.start for t in src)
                assert ptrs(dst) == ptrs(t[layers] for t in dst_all) and all(t.shape[0] == layers.stop - layers.start for t in dst)
                assert (src_exp is None) == (exp_all is None), (full, tier)
                if exp_all is not None:
                    assert ptrs(src_exp) == ptrs(t[layers] for t in exp_all)
                    assert all(t.shape[0] == layers.stop - layers.start for t in src_exp)
        kv.seq_len = P + B + 1
        del calls[:]
        with pytest.raises(IndexError, match="retrieval budget"):
            rc.update_graph_cache(kv)
        with pytest.raises(IndexError, match="retrieval budget"):
            rc._copy_tail(kv, slice(1, 2))
        assert not calls

    # an FP8 full cache says what its rows are: codes, with their exponent bytes
    kv = C.FlashSimpleCache(M(), T, kv_dtype="fp8")
    k, v, first_row, exp = kv.tail_source(slice(1, 3), P)
    assert first_row == P and ptrs((k, v, *exp)) == ptrs((kv.kc[1:3], kv.vc[1:3], kv.ke[1:3], kv.ve[1:3]))
    assert k.dtype == torch.float8_e4m3fn and exp[0].dtype == torch.uint8 and k.shape[0] == exp[0].shape[0] == 2
    k, v, first_row, exp = C.FlashSimpleCache(M(), T, kv_dtype="fp16").tail_source(slice(1, 3), P)
    assert exp is None and first_row == P and k.dtype == torch.float16 and k.shape[0] == 2
