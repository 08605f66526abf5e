"""FP8 weights of the retrieval-verify tier on a real MI355X (TRIFORCE_RETRIEVAL_WEIGHTS=fp8).

Kernels: every FP8 entry point against a float64 torch restatement of the numerics contract (include/triforce_hip.h) —
decoded codes times the row scale, accumulated, rounded to fp16 where the 16-bit kernel rounds, the fused epilogues'
fp16 arithmetic after that; the kernel's fp32 summation order may move a result to the neighbouring fp16 value.  With all
scales 1 and exact e4m3 weights, the same results as the 16-bit kernel (already oracle-tested) on the same values.

Engine: the knob changes only the spec forward — the target verify, the appended full-cache rows and the AR step stay
bit-identical; the spec forward matches a torch forward on the dequantized weights; calibration refreshes the FP8 lm_head
in place; greedy TriForce stays lossless with the tier on, at the tiny sizes and at full 7B size."""
import pytest
import torch
import torch.nn.functional as F

from tests import helpers as Hh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ENV = "TRIFORCE_RETRIEVAL_WEIGHTS"
GAP_TOL = 8e-3        # as tests/test_gpu_e2e.py: an emitted token may trail the target's argmax by ~2 fp16 spacings


def _ops():
    from triforce_amd import ops
    return ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.float16)


def spacing_check(name, got, want, ulps=1, atol=0.0, max_frac=0.05):
    """fp16 results against the contract: none further than `ulps` fp16 spacings (at the reference's magnitude, + atol for
    cancellation near zero), and at most `max_frac` of them different at all."""
    got, want = got.float().cpu(), want.float().cpu()
    assert torch.isfinite(got).all(), f"{name}: non-finite results"
    d = (got - want).abs()
    bound = ulps * sp16(want) + atol
    frac = float((d > 0).float().mean())
    Hh.record("fp8_spacing_check", float((d / bound).max()), what=name, max_abs=float(d.max()), frac_differing=frac)
    assert (d <= bound).all(), f"{name}: {int((d > bound).sum())} results off by more than {ulps} spacing, max {float(d.max()):.3e}"
    assert frac <= max_frac, f"{name}: {frac:.2%} of the results differ"


def sp16(t):
    """fp16 spacing at |t| (elementwise, float32 CPU)."""
    return torch.pow(2.0, torch.floor(torch.log2(torch.clamp(t.abs().float().cpu(), min=2.0 ** -14))) - 10)


def flip_tol(wd, h):
    """[N] bound on what the norm prologue's fp32 summation order can move: the sum of squares decides inv, and an fp32
    neighbour of inv moves an occasional normalised input to its neighbouring fp16 value — one spacing of h times the
    row's largest weight, per flipped input (two allowed)."""
    return (2 * wd.abs().amax(dim=1) * float(sp16(h.abs().max()))).float().cpu()


def _h(v):
    return v.to(torch.float16).double()


def ref_norm(x, ln, eps):
    """h = ln * fp16(x * rsqrt(mean(x^2) + eps)), both products rounded to fp16 (the kernels' norm prologue)."""
    x64 = x.double()
    inv = torch.rsqrt((x64 * x64).mean(dim=1, keepdim=True) + eps)
    return _h(ln.double() * _h(x64 * inv))


class Case:
    """One FP8 weight (device): fp16 source, Fp8Linear, and its dequantized float64 matrix in natural row order."""

    def __init__(self, N, K, seed, split=1, rope=None):
        ops = _ops()
        self.w = rnd(N, K, seed=seed, scale=0.05).to(DEV)
        self.w[5] *= 40.0                                  # a row with a wide range: its small entries go subnormal
        self.pl = ops.PackedLinear(self.w, split=split, rope=rope)
        self.f8 = ops.Fp8Linear(self.pl)
        self.wd = self.f8.dequantized().double()


_CASES = {}


def case(N, K, split=1, rope=None):
    key = (N, K, split, rope)
    if key not in _CASES:
        _CASES.clear()                                     # (one 7B-sized weight resident at a time)
        _CASES[key] = Case(N, K, 1000 + N + K, split, rope)
    return _CASES[key]


def _act(x, packed):
    ops = _ops()
    return ops.Act.from_rows(x, R=max(x.shape[0], 17)) if packed else x


def _rows(y, packed):
    return y.rows() if packed else y


ROWS = [1, 7, 16, 17, 32]
GEMM_SHAPES = [(4096, 4096), (4096, 11008), (32000, 4096), (256, 256), (48, 512)]


@pytest.mark.parametrize("N,K", GEMM_SHAPES)
@pytest.mark.parametrize("M", ROWS)
def test_fp8_gemm_matches_the_contract(M, N, K):
    """tf_skinny_gemm_fp8_act for both activation layouts and every fusion: plain, residual epilogue + ss_out, norm
    prologue (re-reading x and from an ss_in hand-off), fp32 logits (lm_head form)."""
    ops = _ops()
    c = case(N, K)
    eps = 1e-5
    x = rnd(M, K, seed=M + 1).to(DEV)
    res = rnd(M, N, seed=M + 2).to(DEV)
    ln = (1 + 0.1 * rnd(K, seed=3).float()).half().to(DEV)
    wd = c.wd
    acc_plain = x.double() @ wd.T
    h = ref_norm(x, ln, eps)
    acc_norm = h @ wd.T
    atol = 2.0 ** -10 * float(acc_plain.abs().max()) * 2 ** -4    # cancellation: a K-term sum need not shrink with its result
    for packed in (False, True):
        xa = _act(x, packed)
        y = _rows(ops.linear(xa, c.f8), packed)
        spacing_check(f"plain M={M} packed={packed}", y, _h(acc_plain), atol=atol)
        # residual epilogue, in place, with the per-panel sums of squares
        buf = _act(res.clone(), packed)
        ss = ops.ss_buffer(N, DEV)
        ops.linear(xa, c.f8, resid=buf, out=buf, ss_out=ss)
        got = _rows(buf, packed)
        want = _h(res.double() + _h(acc_plain))
        # (a neighbouring fp16 projection is one spacing of the projection, then the add rounds once more)
        spacing_check(f"residual M={M} packed={packed}", got, want, atol=sp16(acc_plain))
        Hh.close(ss[:, :M].sum(dim=0), (got.float() ** 2).sum(dim=1), rtol=2e-6, atol=1e-3)
        # norm prologue, re-reading x
        yn = _rows(ops.linear(xa, c.f8, ln=ln, eps=eps), packed)
        ftol = atol + flip_tol(wd, h)
        spacing_check(f"norm M={M} packed={packed}", yn, _h(acc_norm), atol=ftol, max_frac=0.35)
        # norm prologue from the ss hand-off of x's producer (a 16-bit residual GEMM writing x)
        if K <= 11008:
            pre = ops.PackedLinear(rnd(K, 256, seed=7, scale=0.05).to(DEV))
            src = rnd(M, 256, seed=8).to(DEV)
            xr = _act(x.clone(), packed)
            ss_x = ops.ss_buffer(K, DEV)
            ops.linear(_act(src, packed), pre, resid=xr, out=xr, ss_out=ss_x)
            xv = _rows(xr, packed)
            yh = _rows(ops.linear(xr, c.f8, ln=ln, eps=eps, ss_in=ss_x), packed)
            hx = ref_norm(xv, ln, eps)
            spacing_check(f"norm ss_in M={M} packed={packed}", yh, _h(hx @ wd.T), atol=atol + flip_tol(wd, hx), max_frac=0.35)
        # fp32 logits: the fp16 result cast to float (row-major output)
        y32 = ops.linear(xa, c.f8, out_f32=True, ln=ln, eps=eps)
        assert y32.dtype == torch.float32 and torch.equal(y32, y32.half().float())
        spacing_check(f"fp32 logits M={M} packed={packed}", y32, _h(acc_norm), atol=ftol, max_frac=0.35)


@pytest.mark.parametrize("I,K", [(11008, 4096), (256, 256), (512, 1024)])
@pytest.mark.parametrize("M", ROWS)
def test_fp8_swiglu_matches_the_contract(M, I, K):
    ops = _ops()
    c = case(2 * I, K, split=2)
    eps = 1e-5
    x = rnd(M, K, seed=M + 11).to(DEV)
    ln = (1 + 0.1 * rnd(K, seed=12).float()).half().to(DEV)
    for norm in (False, True):
        h = ref_norm(x, ln, eps) if norm else x.double()
        acc = h @ c.wd.T
        g, u = _h(acc[:, :I]), _h(acc[:, I:])
        # epilogue in the kernel's arithmetic: fp16(silu(g)) with silu in fp32, then the fp16 product
        gf = g.float()
        act = (gf / (1.0 + torch.exp(-gf))).half().double()
        want = _h(act * u)
        for packed in (False, True):
            got = _rows(ops.mlp_act(_act(x, packed), c.f8, ln=ln if norm else None, eps=eps), packed)
            # a neighbouring fp16 gate / up value (one spacing each) moves the product by |up| * spacing(gate) (silu' <= 1.1)
            # + |silu(gate)| * spacing(up), then it is rounded once more
            fl = flip_tol(c.wd, h) if norm else torch.zeros(2 * I)
            tol = 1.1 * u.abs().float().cpu() * (sp16(g) + fl[:I]) + act.abs().float().cpu() * (sp16(u) + fl[I:]) + 2 ** -14
            spacing_check(f"swiglu M={M} norm={norm} packed={packed}", got, want, ulps=1, atol=tol,
                          max_frac=0.35 if norm else 0.08)


@pytest.mark.parametrize("H,D,K", [(32, 128, 4096), (2, 64, 256), (4, 128, 512)])
@pytest.mark.parametrize("M", ROWS)
def test_fp8_qkv_rope_matches_the_contract(M, H, D, K):
    from oracle import ref_ops as R
    from triforce_amd.models.llama_core import rope_tables_plain
    ops = _ops()
    c = case(3 * H * D, K, rope=(H, D))
    eps, T, slot0 = 1e-5, 48, 9
    x = rnd(M, K, seed=M + 21).to(DEV)
    ln = (1 + 0.1 * rnd(K, seed=22).float()).half().to(DEV)
    cos, sin = rope_tables_plain(D, 4096, 10000.0)
    pos = torch.randint(0, 4096, (M,), generator=torch.Generator().manual_seed(M))
    cd, sd, pd = cos.to(DEV), sin.to(DEV), pos.to(DEV)
    hn = ref_norm(x, ln, eps)
    acc = hn @ c.wd.T
    qkv = acc.to(torch.float16).cpu()
    fl = flip_tol(c.wd, hn)                                # (the norm prologue's summation order, see flip_tol)
    flq, flk, flv = (fl[j * H * D:(j + 1) * H * D].view(1, H, D) for j in range(3))
    wq = R.apply_rope(qkv[:, :H * D].view(M, H, D), cos, sin, pos)

    def rope_tol(t, f):        # a neighbouring fp16 value of the row or of its rotary partner, rotated: their spacings
        def part(a):
            return torch.cat([a[..., D // 2:], a[..., :D // 2]], dim=-1)
        return sp16(t) + sp16(part(t)) + f + part(f) + 2 ** -14
    wk = qkv[:, H * D:2 * H * D].view(M, H, D)
    wv = qkv[:, 2 * H * D:].view(M, H, D)
    for rotate_k in (True, False):
        for packed in (False, True):
            k = torch.zeros(H, T, D, dtype=torch.float16, device=DEV)
            v = torch.zeros(H, T, D, dtype=torch.float16, device=DEV)
            sdev = torch.tensor([slot0], dtype=torch.int32, device=DEV)
            q = ops.qkv_rope(_act(x, packed), c.f8, ln, eps, cd, sd, pd, k, v, 0, H, D, rotate_k=rotate_k, slot0_dev=sdev)
            tag = f"M={M} rotate_k={rotate_k} packed={packed}"
            # (a neighbouring fp16 projection, then two more fp16 roundings in the rotation: two spacings)
            spacing_check(f"qkv q {tag}", q, wq, ulps=1, atol=rope_tol(qkv[:, :H * D].view(M, H, D), flq), max_frac=0.35)
            wkk = R.apply_rope(wk, cos, sin, pos) if rotate_k else wk
            spacing_check(f"qkv k {tag}", k[:, slot0:slot0 + M].permute(1, 0, 2), wkk, ulps=1,
                          atol=rope_tol(wk, flk) if rotate_k else flk, max_frac=0.35)
            spacing_check(f"qkv v {tag}", v[:, slot0:slot0 + M].permute(1, 0, 2), wv, atol=flv, max_frac=0.35)
            assert k[:, :slot0].abs().sum() == 0 and k[:, slot0 + M:].abs().sum() == 0
            assert v[:, :slot0].abs().sum() == 0 and v[:, slot0 + M:].abs().sum() == 0


def _exact_e4m3(pl_or_w):
    """Give an Fp8Linear the codes of its (exactly e4m3-representable) fp16 weight and unit scales."""
    ops = _ops()
    f8 = ops.Fp8Linear(pl_or_w)
    for codes, scales, blk in zip(f8.codes, f8.scales, f8._streams()):
        codes.copy_(ops.pack_weight_fp8(blk.to(torch.float8_e4m3fn).view(torch.uint8)))
        scales.fill_(1.0)
    return f8


@pytest.mark.parametrize("M", [1, 7, 17, 32])
def test_unit_scales_and_exact_e4m3_weights_agree_with_the_16_bit_kernel(M):
    """Weights that ARE e4m3 values (as fp16), all scales 1: the FP8 forms compute what the 16-bit forms compute on the
    same values, up to the fp32 summation order of the K loop."""
    from triforce_amd.models.llama_core import rope_tables_plain
    ops = _ops()
    eps = 1e-5

    def exact(N, K, seed):
        return (rnd(N, K, seed=seed, scale=0.3).float().to(torch.float8_e4m3fn).float()).half().to(DEV)

    K, N, H, D = 1024, 768, 2, 128
    x = rnd(M, K, seed=31).to(DEV)
    res = rnd(M, N, seed=32).to(DEV)
    ln = (1 + 0.1 * rnd(K, seed=33).float()).half().to(DEV)
    pl = ops.PackedLinear(exact(N, K, 34))
    f8 = _exact_e4m3(pl)
    assert torch.equal(f8.dequantized().half(), pl.w)
    for packed in (False, True):
        xa = _act(x, packed)
        spacing_check("plain", _rows(ops.linear(xa, f8), packed), _rows(ops.linear(xa, pl), packed), max_frac=0.03)
        b1, b2 = _act(res.clone(), packed), _act(res.clone(), packed)
        ops.linear(xa, f8, ln=ln, eps=eps, resid=b1, out=b1)
        ops.linear(xa, pl, ln=ln, eps=eps, resid=b2, out=b2)
        spacing_check("norm + residual", _rows(b1, packed), _rows(b2, packed), atol=sp16(_rows(ops.linear(xa, pl, ln=ln, eps=eps), packed)),
                      max_frac=0.03)
        spacing_check("fp32 logits", ops.linear(xa, f8, out_f32=True, ln=ln, eps=eps),
                      ops.linear(xa, pl, out_f32=True, ln=ln, eps=eps), max_frac=0.03)
        gu = ops.PackedLinear(exact(2 * N, K, 35), split=2)
        gu8 = _exact_e4m3(gu)
        sw = _rows(ops.mlp_act(xa, gu, ln=ln, eps=eps), packed)
        # (a neighbouring gate or up value propagates through the product: spacings at the largest result)
        spacing_check("swiglu", _rows(ops.mlp_act(xa, gu8, ln=ln, eps=eps), packed), sw, ulps=2,
                      atol=4 * float(sp16(sw.abs().max())), max_frac=0.05)
        qkv = ops.PackedLinear(exact(3 * H * D, K, 36), rope=(H, D))
        qkv8 = _exact_e4m3(qkv)
        cos, sin = rope_tables_plain(D, 512, 10000.0)
        pos = torch.arange(3, 3 + M, device=DEV)
        outs = []
        for w in (qkv8, qkv):
            k = torch.zeros(H, 40, D, dtype=torch.float16, device=DEV)
            v = torch.zeros(H, 40, D, dtype=torch.float16, device=DEV)
            q = ops.qkv_rope(xa, w, ln, eps, cos.to(DEV), sin.to(DEV), pos, k, v, 2, H, D)
            outs.append((q, k, v))
        for a, b, what in zip(outs[0], outs[1], "qkv"):
            spacing_check(f"qkv_rope {what}", a, b, ulps=2, atol=2 * float(sp16(b.abs().max())), max_frac=0.05)


def test_fp8_forms_refuse_unsupported_shapes_and_host_tensors():
    from triforce_amd import hip
    ops = _ops()
    with pytest.raises(hip.TriforceHipError, match="unsupported shape"):
        ops.Fp8Linear(ops.PackedLinear(rnd(64, 96).to(DEV)))             # K % 64
    f8 = ops.Fp8Linear(ops.PackedLinear(rnd(64, 128).to(DEV)))
    with pytest.raises(hip.TriforceHipError):
        ops.linear(rnd(33, 128).to(DEV), f8)                             # > 32 rows: no silent fall-back to a torch GEMM
    with pytest.raises(hip.TriforceHipError):
        ops.linear(rnd(2, 128), f8)                                      # host rows


# ---- engine ------------------------------------------------------------------------------------------------------------
def _engine(g, monkeypatch, fp8, tsd=None, dsd=None, graphs=False):
    if fp8:
        monkeypatch.setenv(ENV, "fp8")
    else:
        monkeypatch.delenv(ENV, raising=False)
    ge = Hh.build_product(g, DEV, tsd, dsd, graphs=graphs)
    W = ge.engine.model.weights
    assert W.fp8_active() == fp8 and (W.lm_head.fp8 is not None) == fp8
    return ge


def test_knob_changes_only_the_spec_forward(monkeypatch):
    """Knob on vs off from the same weights: prefill logits, the target verify's logits and appended full-cache K/V, and
    the AR step's logits are bit-identical; the spec forward matches a torch forward on the dequantized weights (the
    tolerance of the fp16 tier's retrieval-forward check) and differs from the fp16 tier's."""
    from oracle import ref_ops as R
    from tests.test_gpu_e2e import _logit_check
    g = Hh.load_golden("small_gamma6")
    oeng, tsd, dsd = Hh.build_oracle(g)
    ge0 = _engine(g, monkeypatch, False, tsd, dsd)
    ge1 = _engine(g, monkeypatch, True, tsd, dsd)
    prompt = Hh.prompt_of(g).to(DEV)
    outs = []
    for ge in (ge0, ge1):
        ge.inference(prompt[:, :-1])
        lp = ge.inference(prompt[:, -1:])
        S = ge.engine.kv_cache.seq_len
        ids = torch.randint(3, g["tcfg"]["vocab_size"], (1, g["gamma"] + 1), generator=torch.Generator().manual_seed(4)).to(DEV)
        lv = ge.inference(ids, eager=True)
        kv = (ge.engine.kv_cache.k[:, :, :S + ids.shape[1]].clone(), ge.engine.kv_cache.v[:, :, :S + ids.shape[1]].clone())
        la = ge.inference(ids[:, :1])
        outs.append((lp, lv, kv, la, S))
    (lp0, lv0, kv0, la0, S0), (lp1, lv1, kv1, la1, S1) = outs
    assert S0 == S1
    assert torch.equal(lp0, lp1) and torch.equal(lv0, lv1) and torch.equal(la0, la1)
    assert torch.equal(kv0[0], kv1[0]) and torch.equal(kv0[1], kv1[1])
    assert torch.equal(ge0.engine.graph_cache.k, ge1.engine.graph_cache.k)
    # spec forward with the oracle's retrieval cache, against the oracle run on the dequantized weights of the FP8 tier
    oeng.inference(Hh.prompt_of(g)[:, :-1])
    oeng.inference(Hh.prompt_of(g)[:, -1:])
    og, pg = oeng.graph_cache, ge1.engine.graph_cache
    pg.k.copy_(og.key_cache.permute(0, 2, 1, 3))
    pg.v.copy_(og.value_cache.permute(0, 2, 1, 3))
    gamma = g["gamma"]
    vt = torch.tensor([[11, 12, 13] + [100] * (gamma - 2)])
    So = oeng.kv_cache.seq_len
    pos = torch.arange(So, So + gamma + 1).unsqueeze(0)
    W = ge1.engine.model.weights
    m = ge1.engine.model

    def spec():
        return m(input_ids=vt.to(DEV), kv_cache=ge1.engine.kv_cache, graph_cache=pg, position_ids=pos.to(DEV), spec=True).logits.cpu()
    sp8 = spec()
    W.fp8_tier = False
    sp16 = spec()
    W.fp8_tier = True
    assert torch.equal(spec(), sp8)
    assert not torch.equal(sp8, sp16), "the FP8 tier was not exercised"
    sd = dict(oeng.model.sd)
    HD = W.H * W.D
    for i in range(W.L):
        p = f"model.layers.{i}."
        wqkv = W.wqkv[i].fp8.dequantized().float().cpu()
        sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.k_proj.weight"], sd[p + "self_attn.v_proj.weight"] = \
            wqkv[:HD], wqkv[HD:2 * HD], wqkv[2 * HD:]
        sd[p + "self_attn.o_proj.weight"] = W.wo[i].fp8.dequantized().float().cpu()
        wgu = W.wgu[i].fp8.dequantized().float().cpu()
        sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"] = wgu[:W.I_local], wgu[W.I_local:]
        sd[p + "mlp.down_proj.weight"] = W.wd[i].fp8.dequantized().float().cpu()
    sd["lm_head.weight"] = W.lm_head.fp8.dequantized().float().cpu()
    # torch forward on the dequantized weights: fp32 weights, fp32 accumulation, one fp16 rounding (the contract)
    lin = R.linear
    monkeypatch.setattr(R, "linear", lambda x, w: F.linear(x.float(), w).half() if w.dtype == torch.float32 else lin(x, w))
    monkeypatch.setattr(oeng.model, "sd", sd)
    so8 = oeng.model.forward(vt, oeng.kv_cache, og, position_ids=pos, spec=True)
    _logit_check("FP8 spec logits vs torch on the dequantized weights", sp8, so8)


def test_retrieval_verify_rows_are_the_fp8_spec_distribution(monkeypatch):
    """With the hipGraphs captured, the rows the retrieval verify hands to the accept (its probabilities) are
    norm_logits of the FP8 spec forward's logits — the distribution the draw and the accept both see."""
    from triforce_amd.utils.sampling import norm_logits
    g = Hh.load_golden("small_gamma6")
    ge = _engine(g, monkeypatch, True, graphs=True)
    prompt = Hh.prompt_of(g).to(DEV)
    ge.inference(prompt[:, :-1])
    ge.inference(prompt[:, -1:])
    S = ge.engine.kv_cache.seq_len
    gamma = g["gamma"]
    ids = torch.randint(3, g["tcfg"]["vocab_size"], (1, gamma + 1), generator=torch.Generator().manual_seed(6)).to(DEV)
    pos = torch.arange(S, S + gamma + 1, device=DEV).unsqueeze(0)
    rows = ge.graph_verify(ids, pos).clone()
    logits = ge.engine.model_verify(ids, pos, probs=False)
    want = norm_logits(logits[0], temperature=g["temperature"], top_k=-1, top_p=g["top_p"])
    assert torch.equal(rows.reshape(want.shape), want)
    W = ge.engine.model.weights
    W.fp8_tier = False
    l16 = ge.engine.model_verify(ids, pos, probs=False)
    W.fp8_tier = True
    assert not torch.equal(l16, logits)


def test_calibration_runs_on_the_fp16_tier_and_refreshes_the_fp8_lm_head_in_place(monkeypatch):
    from oracle import specs
    from triforce_amd.models import aligned
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache, StreamingLLMEvictionCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as Draft
    from triforce_amd.utils.graph_infer import GraphInferenceEngine
    ops = _ops()
    V, P, B, gamma = 4096, 2048, 256, 4
    tcfg = LlamaConfig.from_dict(specs.tiny_target_config(vocab_size=V, layers=2, hidden=256, heads=2, max_pos=8192))
    dcfg = LlamaConfig.from_dict(specs.draft_68m_config(vocab_size=V))
    spec = aligned.parse_spec("aligned:0.7:0.9:0")
    gains = {}
    for knob in ("fp16", "fp8"):
        monkeypatch.setenv(ENV, knob)
        target = LlamaForCausalLM(tcfg, DEV).init_aligned(spec, attn_keys=B)
        draft = Draft(dcfg, DEV).init_aligned(spec, attn_keys=256)
        ge = GraphInferenceEngine(target, FlashSimpleCache(target, P + 64),
                                  RetrievalCache(target, max_budget=B, prefill=P, gamma=gamma, chunk_size=8), draft,
                                  StreamingLLMEvictionCache(draft, start_size=16, recent_size=256 - 16 - gamma, gamma=gamma))
        ge.initialize_eager(gamma, probs=True, temperature=0.6, top_p=0.9)
        W = target.weights
        if knob == "fp8":
            ptr_c, ptr_s = W.lm_head.fp8.codes[0].data_ptr(), W.lm_head.fp8.scales[0].data_ptr()
            before = W.lm_head.fp8.codes[0].clone()
        prompt = specs.random_prompt(V, P, 11).to(DEV)
        ge.inference(prompt[:, :-1])
        ge.inference(prompt[:, -1:])                       # q_len == 1: the retrieval cache is built here
        out = aligned.calibrate_engine(ge, gamma, 0.6, 0.9)
        gains[knob] = out
        if knob == "fp8":
            assert W.fp8_tier and W.fp8_active()
            c, s = ops.quantize_fp8_rows(W.lm_head.w)
            assert W.lm_head.fp8.codes[0].data_ptr() == ptr_c and W.lm_head.fp8.scales[0].data_ptr() == ptr_s
            assert torch.equal(W.lm_head.fp8.codes[0], ops.pack_weight_fp8(c)) and torch.equal(W.lm_head.fp8.scales[0], s)
            assert not torch.equal(before, W.lm_head.fp8.codes[0])
        del ge, target, draft
    # the same calibration with or without the knob: it ran on the fp16 tier both times (read-out gain, probe acceptance
    # and the probe statistics, as the calibration reports them)
    assert gains["fp16"] == gains["fp8"], gains


@pytest.mark.parametrize("graphs", [False, True])
def test_greedy_triforce_with_the_fp8_tier_is_lossless_small(graphs, monkeypatch):
    from triforce_amd.utils.decoding import TriForce
    g = Hh.load_golden("small_gamma6")
    ge = _engine(g, monkeypatch, True, graphs=graphs)
    prompt = Hh.prompt_of(g).to(DEV)
    res = TriForce(Hh.FakeTokenizer(), ge, prompt, gamma=g["gamma"], max_len=g["gen_len"], top_k=-1, top_p=g["top_p"],
                   temperature=g["temperature"], return_details=True)
    gaps = Hh.teacher_forced_gaps(g, res["tokens"])
    assert max(gaps) < GAP_TOL, f"token {gaps.index(max(gaps))} trails the fp16 target's argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x == 0.0) >= len(gaps) - 3
    Hh.note(f"fp8 tier small_gamma6 graphs={graphs}: acceptance {res['acceptance_rate']:.3f}")


def test_full_scale_7b_greedy_triforce_with_the_fp8_tier_is_lossless(monkeypatch):
    """tests/test_gpu_e2e.py::test_full_scale_7b_greedy_triforce_is_lossless_on_device with the FP8 retrieval tier:
    configs[1] shape, 124 928-token prefix, budget 4096, gamma 6, hipGraphs.  Every emitted token must be the fp16
    target's teacher-forced argmax (up to GAP_TOL)."""
    import argparse
    import bench
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.sampling import UniformSource
    monkeypatch.setenv(ENV, "fp8")
    args = argparse.Namespace(target="llama-7B-128K", prefill=124928, budget=4096, chunk_size=8, gamma=6, temp=1.0,
                              top_p=1e-9, gen_cap=256, seed=0, no_graphs=False)
    dev = torch.device(DEV)
    target, draft = bench.load_models(args, dev, "random", "random:1", "random:2")
    assert target.weights.fp8_active()
    ge = bench.build_engine(args, dev, target, draft)
    tcfg, _ = bench.target_config(args.target)
    ids = torch.randint(3, tcfg.vocab_size, (1, args.prefill), generator=torch.Generator().manual_seed(0)).to(dev)
    run = TriForceRunner(bench._Tok(), ge, args.gamma, top_k=-1, top_p=args.top_p, temperature=args.temp,
                         rng=UniformSource(dev, seed=0))
    bench.do_prefill(run, ge, ids, "synthetic")
    P = ge.engine.kv_cache.seq_len
    while run.n < 20:
        run.step()
    stream = list(run.emitted)
    assert len(stream) >= 21 and ge.engine.kv_cache.seq_len == P + run.n
    eng = ge.engine
    eng.kv_cache.seq_len = P
    gaps = []
    for i in range(len(stream) - 1):                     # teacher-forced fp16 target (full-cache forward: fp16 weights)
        tok = torch.tensor([[stream[i]]], device=dev)
        logits = eng.model(input_ids=tok, kv_cache=eng.kv_cache, graph_cache=None).logits[0, -1]
        gaps.append(float(logits.max() - logits[stream[i + 1]]))
    assert max(gaps) < GAP_TOL, f"token {gaps.index(max(gaps)) + 1} trails the autoregressive argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x == 0.0) >= len(gaps) - 2
    del ge, run, eng, target, draft
    torch.cuda.empty_cache()


def test_tensor_parallel_engine_refuses_fp8(monkeypatch):
    from triforce_amd.models.TP_llama import DistributedLlama
    monkeypatch.setenv(ENV, "fp8")
    with pytest.raises(NotImplementedError, match=ENV):
        DistributedLlama("random:0", device=DEV)
