"""Attention bias on the device: tf_skinny_gemm_bias_act, tf_skinny_qkv_rope_bias_act and
tf_skinny_qkv_rope_gqa_bias_act.

Exact probes.  The material of tests/gemm_probes.py (``select`` and ``dense``: every K sum exact in fp32 in any order) plus a
bias b[n] = step * ((7 n mod 61) - 30) in the case's own step: the contract y = fp16(fp32(acc) + float(b)) is then evaluated
on the host with the same two IEEE operations (for ``dense`` the sum is an integer multiple of the step and nothing rounds
before fp16), and the value names its row — a bias from the wrong row, panel, section, head or rotary slot, one added after
the rotation or once per K share comes back as a wrong known number.  torch.equal, outputs pre-filled with the probes'
sentinel.  The cases reach every launch form csrc/sg_rule.h can pick for the three modes; the reached set is asserted.

Zero-bias identity, the TF_EINVAL gates, and the model: logits of tiny-bias / tiny-gqa-bias against an fp64 evaluation of the
same weights with the CPU restatement's own deviation as the yardstick, greedy TriForce (eager, captured, extend, FP8 KV cache,
TRIFORCE_FUSE=none) teacher-forced through the biased oracle.
"""
import pytest
import torch

from oracle import ref_model as M
from oracle import ref_ops as R
from oracle import specs
from tests import attn_bias_ref as B
from tests import gemm_probes as P
from tests import helpers as Hh
from tests.test_gpu_gemm_probes import (SS_SENTINEL, embed_act, first_diff, knobs, operand, out_buffer,  # noqa: F401
                                        sentinel_allocs)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP_TOL = 8e-3                                   # tests/test_gpu_gqa.py


def _ops():
    from triforce_amd import ops
    return ops


# ---- exact probes ---------------------------------------------------------------------------------------------------------------
def bias_of(c, kind):
    """b[n] = step * ((7 n mod 61) - 30), n the row of the natural order, fp16 (exact: |b| <= 30)."""
    n = torch.arange(P.streams_of(c) * c["N"])
    return (P.step_of(c, kind) * ((7 * n) % 61 - 30).double()).half()


def expected(c, mat, li, b):
    """tests/gemm_probes.expected with the bias in: y = fp16(fp32(acc) + fp32(b)), everything after it unchanged."""
    e = P.expected(c, mat, li)
    M_, N = c["M"], c["N"]
    acc32 = e["acc"].float()
    assert torch.equal(acc32.double(), e["acc"]), "the K sum is an fp32 value"
    y = (acc32 + b.float()[None, :]).half()
    out = dict(y=y)
    if P.mode_of(c) in (P.SG_QKV, P.SG_QKVG):
        H, Hkv, D = c["H"], c["Hkv"], c["D"]
        q, k, v = y[:, :H * D].view(M_, H, D), y[:, H * D:(H + Hkv) * D].view(M_, Hkv, D), y[:, (H + Hkv) * D:].view(M_, Hkv, D)
        out.update(q=R.apply_rope(q, mat["cos"], mat["sin"], mat["pos"]),
                   k=R.apply_rope(k, mat["cos"], mat["sin"], mat["pos"]) if c.get("rotate_k", True) else k, v=v)
    else:
        o = y
        if c.get("resid"):
            o = (mat["res"].double() + y.double()).float().half()
        out["ss"] = o.double().square().view(M_, N // 16, 16).sum(-1).t().contiguous()
        out["out"] = o
    return out


def _rope(ep, M_, H, Hkv, D, K, **kw):
    return P.case(ep, M_, (H + 2 * Hkv) * D, K, H=H, Hkv=Hkv, D=D, **kw)


def _cases():
    out = []
    # q|k|v: the three head layouts; every row count, both K, rotate_k on / off, host / device slot, every form
    for hi, (ep, H, Hkv, D) in enumerate((("qkv", 2, 2, 128), ("qkvg", 4, 2, 128), ("qkvg", 4, 2, 64))):
        ks = (2, 3, 4)[hi]
        out += [
            _rope(ep, 1, H, Hkv, D, 256, norm=True),                                        # (1, 4, 1, 1)
            _rope(ep, 7, H, Hkv, D, 4096, norm=True, rotate_k=False, slot_dev=True),        # (1, 8, 1, 1)
            _rope(ep, 16, H, Hkv, D, 4096, knobs={2: 1}, slot_dev=True),                    # (1, 4, 2, 1)
            _rope(ep, 17, H, Hkv, D, 256, slot_dev=True),                                   # (2, 4, 1, 1)
            _rope(ep, 32, H, Hkv, D, 4096, norm=True),                                      # (2, 8, 1, 1)
            _rope(ep, 17, H, Hkv, D, 4096, norm=True, knobs={2: 1}, rotate_k=False),        # (2, 4, 2, 1)
            _rope(ep, 7, H, Hkv, D, 4096, knobs={4: ks}),                                   # (1, 8, 1, ks)
            _rope(ep, 32, H, Hkv, D, 4096, norm=True, knobs={4: 6 - ks}, slot_dev=True),    # (2, 8, 1, ks')
        ]
    # more than 512 panels: 4 waves per panel at K = 4096, split by the knob (the 7B q|k|v grid is of this kind)
    out.append(_rope("qkv", 7, 22, 22, 128, 4096, norm=True, knobs={4: 2}, big=True))       # (1, 4, 1, 2)
    out.append(_rope("qkv", 17, 22, 22, 128, 4096, knobs={4: 4}, big=True))                  # (2, 4, 1, 4)
    # plain: with and without resid / ss_out, norm on / off
    for i, M_ in enumerate((1, 7, 16, 17, 32)):
        opt = dict(resid=True, ss_out=True) if i % 2 == 0 else {}
        out.append(P.case("plain", M_, 320, 256, **opt))                                    # (mt, 4, 1, 1)
        out.append(P.case("plain", M_, 320, 4096, norm=(i % 2 == 1), **({} if opt else dict(resid=True, ss_out=True))))  # (mt, 8, 1, 1)
    out.append(P.case("plain", 16, 320, 4096, knobs={2: 1}, ss_out=True))                   # (1, 4, 2, 1)
    out.append(P.case("plain", 32, 320, 4096, norm=True, knobs={2: 1}, resid=True, ss_out=True))   # (2, 4, 2, 1)
    for M_, ks in ((7, 2), (1, 3), (16, 4), (17, 2), (32, 3), (17, 4)):
        out.append(P.case("plain", M_, 320, 4096, knobs={4: ks}, resid=(ks != 3), ss_out=(ks != 3)))   # (mt, 8, 1, ks)
    out.append(P.case("plain", 7, 8208, 4096, knobs={4: 3}, resid=True, ss_out=True, big=True))       # (1, 4, 1, 3)
    out.append(P.case("plain", 17, 8208, 4096, knobs={4: 2}, big=True))                                # (2, 4, 1, 2)
    return out


def case_id(c):
    return P.case_id(c) + ("-slotdev" if c.get("slot_dev") else "")


CASES = _cases()
# every form sg_pick_form / sg_pick_ks can give the plain and the q|k|v modes: one or two row tiles x (4 | 8 waves, one panel
# per wave; 4 waves, two panels per wave; K split 2 / 3 / 4 ways at 8 waves and at 4 waves)
FORMS = sorted([("sg", mt, w, 1, 1) for mt in (1, 2) for w in (4, 8)] + [("sg", mt, 4, 2, 1) for mt in (1, 2)]
               + [("sg", mt, 8, 1, ks) for mt in (1, 2) for ks in (2, 3, 4)])
FORMS_BIG = {"plain": [("sg", 1, 4, 1, 3), ("sg", 2, 4, 1, 2)], "qkv": [("sg", 1, 4, 1, 2), ("sg", 2, 4, 1, 4)]}
REACHED = {}


def test_case_list_reaches_every_form():
    """(runs without touching the device) plain, and q|k|v over its two modes, each reach every form of FORMS; the split
    4-wave forms of the > 512-panel grids are reached by the two big cases of each."""
    for group in ("plain", "qkv"):
        got = sorted({P.form_of(c) for c in CASES if c["ep"].startswith(group) and not c.get("big")})
        assert got == FORMS, (group, sorted(set(FORMS) ^ set(got)))
        assert sorted(P.form_of(c) for c in CASES if c["ep"].startswith(group) and c.get("big")) == sorted(FORMS_BIG[group])
    assert {c["ep"] for c in CASES} == {"plain", "qkv", "qkvg"}
    assert {c["M"] for c in CASES} == {1, 7, 16, 17, 32} and {c["K"] for c in CASES} == {256, 4096}
    assert {(c["H"], c["Hkv"], c["D"]) for c in CASES if "H" in c and not c.get("big")} == {(2, 2, 128), (4, 2, 128), (4, 2, 64)}


def run_probe(ops, c, kind, layout, monkeypatch):
    M_, N, K = c["M"], c["N"], c["K"]
    mat = P.material(c, kind)
    b = bias_of(c, kind)
    x = operand(ops, mat["x"], layout, float("nan"))
    ln = mat["ln"].to(DEV) if mat["ln"] is not None else None
    eps = P.EPS if ln is not None else 0.0
    for li, w in enumerate(mat["ws"]):
        e = expected(c, mat, li, b)
        where = f"{case_id(c)} [{kind}, {layout}, launch {li}] form {P.form_of(c)}"
        with monkeypatch.context() as mp:
            mp.setattr(ops, "N8_ENABLED", False)
            rope = (c["H"], c["Hkv"], c["D"]) if c["ep"].startswith("qkv") else None
            pl = ops.PackedLinear(w.to(DEV), rope=rope, bias=b.to(DEV))
        if rope is not None:
            H, Hkv, D = rope
            T = P.SLOT0 + M_ + 5
            kc = torch.full((Hkv, T, D), P.SENTINEL, dtype=torch.float16, device=DEV)
            vc = torch.full((Hkv, T, D), P.SENTINEL, dtype=torch.float16, device=DEV)
            slot_dev = torch.tensor([P.SLOT0], dtype=torch.int32, device=DEV) if c.get("slot_dev") else None
            with sentinel_allocs(ops, monkeypatch):
                q = ops.qkv_rope(x, pl, ln, eps, mat["cos"].to(DEV), mat["sin"].to(DEV), mat["pos"].to(DEV), kc, vc,
                                 0 if slot_dev is not None else P.SLOT0, H, D, rotate_k=c.get("rotate_k", True),
                                 slot0_dev=slot_dev, Hkv=Hkv, bias=pl.bias_rope).cpu()
            assert torch.equal(q, e["q"]), f"{where}: q (m, head, d) {first_diff(q, e['q'])}"
            for name, cache, rows in (("k", kc, e["k"]), ("v", vc, e["v"])):
                want = torch.full((Hkv, T, D), P.SENTINEL, dtype=torch.float16)
                want[:, P.SLOT0:P.SLOT0 + M_] = rows.permute(1, 0, 2)
                got = cache.cpu()
                idx = first_diff(got, want)
                assert idx is None, f"{where}: {name} cache (head, slot, d) {idx}: got {float(got[idx])}, expected {float(want[idx])}"
        else:
            out, rows, intact = out_buffer(ops, M_, N, layout)
            resid = None
            if c.get("resid"):
                if layout == "rows":
                    out.copy_(mat["res"].to(DEV))
                    resid = out
                else:
                    resid = embed_act(ops, mat["res"], float("nan"))
            ss = None
            if P.wants_ss_out(c, kind):
                ss = torch.full((N // 16, 32), SS_SENTINEL, dtype=torch.float32, device=DEV)
            ret = ops.linear(x, pl, ln=ln, eps=eps, resid=resid, out=out, ss_out=ss, bias=pl.bias)
            assert ret is out
            got, want = rows().cpu(), e["out"]
            idx = first_diff(got, want)
            assert idx is None, f"{where}: element {idx}: got {float(got[idx])}, expected {float(want[idx])} (bias {float(b[idx[1]])})"
            assert intact(), f"{where}: output rows past M were written"
            if ss is not None:
                got_ss = ss[:, :M_].double().cpu()
                if P.ss_exact(c, kind):
                    assert torch.equal(got_ss, e["ss"]), (where, "ss_out", first_diff(got_ss, e["ss"]))
                else:
                    torch.testing.assert_close(got_ss, e["ss"], rtol=2e-6, atol=0.0)
    REACHED.setdefault(c["ep"][:3] if c["ep"].startswith("qkv") else c["ep"], set()).add(P.form_of(c))


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_bias_probe(c, monkeypatch):
    ops = _ops()
    ops._ensure_sg_workspace(DEV)
    combos = (("dense", "rows"), ("select", "packed")) if c.get("big") else [(k, l) for k in P.KINDS for l in P.LAYOUTS]
    with knobs(P.knobs_of(c)):
        for kind, layout in combos:
            run_probe(ops, c, kind, layout, monkeypatch)
    if P.form_of(c)[4] > 1:
        torch.cuda.synchronize()
        ws = ops._SG_WS[torch.device(DEV)]
        slot = ws.numel() // 4
        assert all(int(ws[i * slot:i * slot + 4 * P.SG_TICKETS].sum()) == 0 for i in range(4)), "tickets were not left zero"


def test_zz_every_form_was_run():
    """The forms the probes above actually launched (a deselected or failed case leaves a hole here)."""
    for group in ("plain", "qkv"):
        assert sorted(REACHED.get(group, ())) == sorted(FORMS + FORMS_BIG[group]), group


# ---- zero-bias identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M_", [7, 17])
def test_zero_bias_is_the_bias_free_kernel(M_):
    ops = _ops()
    gen = torch.Generator().manual_seed(100 + M_)
    K = 512
    x = (torch.randn(M_, K, generator=gen)).half().to(DEV)
    ln = (1 + 0.1 * torch.randn(K, generator=gen)).half().to(DEV)
    cos, sin = (t.to(DEV) for t in R.rope_tables_plain(128, 64))
    pos = torch.randperm(64, generator=gen)[:M_].to(DEV)
    for H, Hkv, D in ((2, 2, 128), (4, 2, 128)):
        N = (H + 2 * Hkv) * D
        w = (torch.randn(N, K, generator=gen) * 0.05).half().to(DEV)
        free = ops.PackedLinear(w, rope=(H, Hkv, D))
        zero = ops.PackedLinear(w, rope=(H, Hkv, D), bias=torch.zeros(N, dtype=torch.float16, device=DEV))
        res = []
        for pl in (free, zero):
            kc = torch.full((Hkv, M_ + 4, D), P.SENTINEL, dtype=torch.float16, device=DEV)
            vc = kc.clone()
            kw = {} if pl.bias is None else {"bias": pl.bias_rope}
            q = ops.qkv_rope(x, pl, ln, 1e-6, cos, sin, pos, kc, vc, 2, H, D, Hkv=Hkv, **kw)
            res.append((q, kc, vc))
        for a, b_ in zip(*res):
            assert torch.equal(a, b_)
    Nn = 512
    w = (torch.randn(Nn, K, generator=gen) * 0.05).half().to(DEV)
    free, zero = ops.PackedLinear(w), ops.PackedLinear(w, bias=torch.zeros(Nn, dtype=torch.float16, device=DEV))
    r0 = torch.randn(M_, Nn, generator=gen).half().to(DEV)
    for opts in (dict(), dict(resid=True)):
        got = []
        for pl in (free, zero):
            out = r0.clone() if opts else torch.empty(M_, Nn, dtype=torch.float16, device=DEV)
            ss = ops.ss_buffer(Nn, DEV).zero_()
            kw = {} if pl.bias is None else {"bias": pl.bias}
            ops.linear(x, pl, resid=out if opts else None, out=out, ss_out=ss, **kw)
            got.append((out, ss[:, :M_].clone()))
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


# ---- gates ----------------------------------------------------------------------------------------------------------------------
def test_bias_entry_points_return_einval():
    ops = _ops()
    L = ops.hip.lib()
    buf = torch.zeros(1 << 16, dtype=torch.float16, device=DEV)
    pos = torch.zeros(8, dtype=torch.int64, device=DEV)
    p, ps, s = ops._ptr(buf), ops._ptr(pos), ops._stream()
    odd = ops._ptr(buf[1:])                                                             # 2-byte aligned
    D = 128

    def plain(bias=p, out_f32=0, M_=1, K=64, w=p):
        return L.tf_skinny_gemm_bias_act(w, p, K, 8, None, 0.0, None, None, 0, 0, None, p, 16, 8, M_, 16, K, out_f32, bias, s)

    def qkv(bias=p, H=1, M_=1, K=64, st=4096):
        return L.tf_skinny_qkv_rope_bias_act(p, p, K, 8, None, 0.0, None, p, p, ps, p, p, p, D, st, 0, None, M_, H, D, K, 1, bias, s)

    def qkvg(bias=p, H=2, Hkv=1, M_=1, K=64, Dh=D):
        return L.tf_skinny_qkv_rope_gqa_bias_act(p, p, K, 8, None, 0.0, None, p, p, ps, p, p, p, Dh, 4096, 0, None, M_, H, Hkv, Dh, K,
                                                 1, bias, s)
    assert plain() == 0 and qkv() == 0 and qkvg() == 0                                  # the calls are otherwise well formed
    for fn in (plain, qkv, qkvg):
        assert fn(bias=None) == -22 and fn(bias=odd) == -22                             # null / misaligned bias
        assert fn(M_=33) == -22 and fn(M_=0) == -22 and fn(K=48) == -22                 # the neighbour's shape gates
    assert plain(out_f32=1) == -22 and plain(w=None) == -22
    assert qkv(H=0) == -22 and qkv(st=4098) == -22
    assert qkvg(H=3, Hkv=2) == -22 and qkvg(Dh=96) == -22
    torch.cuda.synchronize()


# ---- model ------------------------------------------------------------------------------------------------------------------------
_W = {}


def _weights(name):
    if name not in _W:                                       # drawn once, shared, left unchanged
        g = B.zoo_case(name, gen_len=160)             # (capacity for the stream, one chat turn and its answer)
        _W[name] = (g,) + B.zoo_state_dicts(g)
    return _W[name]


def _product(name, graphs, **kw):
    g, sd, _, dsd = _weights(name)
    return Hh.build_product(g, DEV, sd, dsd, graphs=graphs, **kw)


@pytest.mark.parametrize("name", ["tiny-bias", "tiny-gqa-bias"])
def test_model_logits_within_the_restatements_own_error(name):
    """A 128-token prefill chunk, then 7 decode rows, eager and captured.  Truth: the fp64 evaluation of the stored weights.
    Yardstick: the CPU restatement's deviation from it.  Device: within 2 x its max and 1.25 x its mean (the kernels sum in
    another order)."""
    g, sd, esd, dsd = _weights(name)
    ge = _product(name, graphs=True)
    W = ge.engine.model.weights
    assert W.attn_bias and W.wqkv[0].bias_rope is not None and (W.wo[0].bias is not None) == (name == "tiny-bias")
    prompt = specs.random_prompt(g["tcfg"]["vocab_size"], 128, g["pseed"])
    rows = torch.randint(3, g["tcfg"]["vocab_size"], (1, 7), generator=torch.Generator().manual_seed(7))
    truth = B.forward_fp64(g["tcfg"], sd, torch.cat([prompt, rows], dim=1)[0])
    t_pre, t_dec = truth[127], truth[128:]
    ot, okv = B.BiasedOracleTarget(g["ecfg"], esd), M.FullCache(g["ecfg"], 256)
    o_pre = ot.forward(prompt, okv, None)[0, -1].double()
    o_dec = ot.forward(rows, okv, None)[0].double()
    kvc = ge.engine.kv_cache
    kvc.reset()
    d_pre = ge.inference(prompt.to(DEV))[0, -1].double().cpu()
    S = kvc.seq_len
    assert S == 128
    eager = ge.inference(rows.to(DEV), eager=True)[0].double().cpu()
    kvc.seq_len = S
    captured = ge.inference(rows.to(DEV))[0].double().cpu()
    kvc.seq_len = S
    for what, dev, ora, tru in (("prefill chunk, last row", d_pre, o_pre, t_pre), ("7 decode rows, eager", eager, o_dec, t_dec),
                                ("7 decode rows, captured", captured, o_dec, t_dec)):
        y, d = (ora - tru).abs(), (dev - tru).abs()
        ymax, ymean, dmax, dmean = float(y.max()), float(y.mean()), float(d.max()), float(d.mean())
        print(f"[attn-bias] {name} {what}: restatement max {ymax:.3e} mean {ymean:.3e} | device max {dmax:.3e} mean {dmean:.3e}")
        ok_max = Hh.bound(f"attn bias {name} {what}: max |dlogit| vs fp64 (limit 2 x restatement)", dmax, 2.0 * ymax)
        ok_mean = Hh.bound(f"attn bias {name} {what}: mean |dlogit| vs fp64 (limit 1.25 x restatement)", dmean, 1.25 * ymean)
        assert ok_max and ok_mean, (name, what, dict(restatement=(ymax, ymean), device=(dmax, dmean)))


def _check_stream(what, name, prompt, stream):
    g, _, esd, _ = _weights(name)
    ot, okv = B.BiasedOracleTarget(g["ecfg"], esd), M.FullCache(g["ecfg"], prompt.shape[1] + len(stream) + 8)
    logits = ot.forward(prompt, okv, None)[0, -1]           # (as tests/test_gpu_gqa.py _gaps, through the biased oracle)
    gaps = [float(logits.max() - logits[stream[0]])]
    for i in range(len(stream) - 1):
        logits = ot.forward(torch.tensor([[stream[i]]]), okv, None)[0, -1]
        gaps.append(float(logits.max() - logits[stream[i + 1]]))
    worst = max(gaps)
    Hh.record("bound", worst / GAP_TOL, what=f"attn bias {name} {what}: worst teacher-forced gap", value=worst, limit=GAP_TOL)
    assert worst < GAP_TOL, f"{what}: token {gaps.index(worst)} trails the biased oracle's argmax by {worst:.4f} logit"
    exact = sum(1 for x in gaps if x == 0.0)
    assert exact >= len(gaps) - 3, f"{what}: only {exact}/{len(gaps)} tokens are the biased oracle's exact argmax"


def _run_triforce(ge, g, prompt, n):
    from triforce_amd.utils.decoding import TriForceRunner
    tok = Hh.FakeTokenizer()
    tok.eos_token_id = -1
    run = TriForceRunner(tok, ge, g["gamma"], top_k=-1, top_p=g["top_p"], temperature=g["temperature"])
    run.prefill(prompt.to(DEV))
    while run.n < n:
        run.step()
    return run


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("name", ["tiny-bias", "tiny-gqa-bias"])
def test_greedy_triforce_and_extend_follow_the_biased_oracle(name, graphs):
    g = _weights(name)[0]
    ge = _product(name, graphs=graphs)
    prompt = Hh.prompt_of(g)
    run = _run_triforce(ge, g, prompt, 32)
    stream = list(run.emitted)
    assert len(stream) >= 33
    _check_stream(f"triforce graphs={graphs}", name, prompt, stream)
    if graphs:
        turn = torch.randint(3, g["tcfg"]["vocab_size"], (1, 64), generator=torch.Generator().manual_seed(77))
        run.extend(turn.to(DEV))
        history = torch.cat([prompt, torch.tensor([stream]), turn], dim=1)
        assert torch.equal(run.history.cpu(), history) and run.n == 0
        while run.n < 12:
            run.step()
        _check_stream("extend", name, history, list(run.emitted))


def test_unfused_layer_follows_the_biased_oracle(monkeypatch):
    """TRIFORCE_FUSE=none: q|k|v through tf_skinny_gemm_bias_act + tf_rope_append, o_proj through the same entry."""
    ops = _ops()
    monkeypatch.setattr(ops, "FUSE_MODE", "none")
    calls = []
    real = ops.hip.lib().tf_skinny_gemm_bias_act
    monkeypatch.setattr(ops.hip.lib(), "tf_skinny_gemm_bias_act", lambda *a: calls.append(1) or real(*a))
    for name in ("tiny-bias", "tiny-gqa-bias"):
        g = _weights(name)[0]
        ge = _product(name, graphs=False)
        prompt = Hh.prompt_of(g)
        n0 = len(calls)
        run = _run_triforce(ge, g, prompt, 24)
        assert len(calls) > n0, "the un-fused decode rows did not take the bias GEMM"
        _check_stream("TRIFORCE_FUSE=none", name, prompt, list(run.emitted))


def test_fp8_kv_cache_stays_lossless_against_its_own_target(monkeypatch):
    """TRIFORCE_KV_CACHE=fp8 (multi-head): the cache is not lossless against the fp16 model, so greedy TriForce is checked
    against the FP8-KV target's own Autoregressive steps, as tests/test_gpu_fp8_kv.py does."""
    from tests.test_gpu_fp8_kv import _ar_gaps
    monkeypatch.setenv("TRIFORCE_KV_CACHE", "fp8")
    g = _weights("tiny-bias")[0]
    ge = _product("tiny-bias", graphs=True)
    assert ge.engine.kv_cache.fp8 and ge.engine.model.weights.attn_bias
    prompt = Hh.prompt_of(g)
    run = _run_triforce(ge, g, prompt, 32)
    stream = list(run.emitted)
    gaps = _ar_gaps(ge.engine.model, prompt.to(DEV), stream, g["prefill"] + len(stream) + 16)
    assert max(gaps) < GAP_TOL, f"token {gaps.index(max(gaps))} trails the FP8-KV target's argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x == 0.0) >= len(gaps) - 3
