"""fp16(fp32 product) pinned to two roundings on the device (tests/rounding_probes.py; include/triforce_hip.h, "ROUNDING OF
fp16(a * b)"): tf_rmsnorm, the norm prologue of every 16-bit and FP8 decode-GEMM form, the FP8 row-scale epilogue, the one-pass
retrieval scorer, tf_chunk_mean and the indexed scorer, on material whose expectation is known bit for bit and on which ONE
rounding of the exact product gives another fp16 value at the recorded witness elements.  ``==`` only.

A failure is reported by name: the site, the element, got / want / the one-rounding value.  "Equals the one-rounding value" reads
as "the compiler folded the product and the cast into one instruction (v_fma_mixlo_f16)".  The control family of tf_rmsnorm (an
exact inv) separates a divide / square-root rounding difference from the product rounding.
"""
import pytest
import torch

from tests import gemm_probes as P
from tests import rounding_probes as Q
from tests import test_gpu_gemm_probes as G

pytestmark = pytest.mark.gpu
DEV = G.DEV
SENTINEL = P.SENTINEL


def _ops():
    from triforce_amd import ops
    return ops


def report(site, name, got, want, one):
    """None when got == want everywhere; else the first differing element by name."""
    got, want, one = (torch.as_tensor(t).cpu() for t in (got, want, one))
    assert got.shape == want.shape and got.dtype == want.dtype, (site, name, got.shape, want.shape, got.dtype, want.dtype)
    diff = got != want
    if not bool(diff.any()):
        return None
    idx = tuple(int(v) for v in diff.nonzero()[0])
    g, w, o = float(got[idx]), float(want[idx]), float(one[idx])
    folded = int((diff & (got == one)).sum())
    verdict = "equals the one-rounding value: the product was folded into the cast" if (g == o and o != w) else \
        "is NOT the one-rounding value either: look past the product rounding"
    return (f"{name} [{site}]: element {idx}: got {g!r}, want {w!r}, one-rounding {o!r} — {verdict}; {int(diff.sum())} elements "
            f"differ, {folded} of them equal the one-rounding value")


def check(site, name, got, want, one):
    msg = report(site, name, got, want, one)
    assert msg is None, msg


# ---- tf_rmsnorm -------------------------------------------------------------------------------------------------------------------
def _rmsnorm(ops, m, variant):
    """-> (y, the fp16 sum the kernel wrote | None) on the CPU."""
    x = torch.from_numpy(m["x"]).to(DEV)
    w = torch.from_numpy(m["w"]).to(DEV)
    res = torch.from_numpy(m["res"]).to(DEV) if m["res"] is not None else None
    so = None
    if variant == "resid_sum_out":
        so = torch.full_like(x, SENTINEL)
    elif variant == "resid_in_place":                      # the decode layer's call: the sum replaces the residual stream
        so = res
    y = ops.rmsnorm(x, w, m["eps"], residual=None if variant == "plain" else res, sum_out=so)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), torch.from_numpy(m["x"])), "the input rows were written"
    if res is not None and so is not res:
        assert torch.equal(res.cpu(), torch.from_numpy(m["res"])), "the residual rows were written"
    return y.cpu(), (so.cpu() if so is not None else None)


@pytest.mark.parametrize("variant", Q.RMS_VARIANTS)
@pytest.mark.parametrize("rows", Q.RMS_ROWS)
@pytest.mark.parametrize("hidden", Q.RMS_HIDDEN)
def test_rmsnorm(hidden, rows, variant):
    ops = _ops()
    for family in Q.FAMILIES:
        c = (hidden, rows, variant, family)
        m = Q.rms_material(c)
        y, so = _rmsnorm(ops, m, variant)
        check("rmsnorm_kernel: fp16(x * inv)", Q.rms_id(c), y, m["y"], m["y1"])
        if so is not None:
            assert torch.equal(so, torch.from_numpy(m["sum"])), f"{Q.rms_id(c)}: sum_out rows"


@pytest.mark.parametrize("hidden", Q.RMS_HIDDEN)
def test_rmsnorm_with_an_exact_inverse(hidden):
    """eps = 0 and a mean square of 4^k: inv is a power of two whatever rounds the divide and the square root, and no witness
    exists.  If test_rmsnorm fails where this passes, look at the product rounding first; if this fails too, not there."""
    ops = _ops()
    for rows in Q.RMS_ROWS:
        m = Q.rms_control(hidden, rows)
        y, _ = _rmsnorm(ops, m, "plain")
        check("rmsnorm_kernel, control", f"rmsnorm-control-h{hidden}-r{rows}", y, m["y"], m["y1"])


# ---- the decode GEMMs ---------------------------------------------------------------------------------------------------------------
def _handoff(ops, c, mat, layout, monkeypatch):
    """x and its per-panel sums of squares as a preceding GEMM leaves them: x = x . I^T through the 16-bit kernel with ss_out."""
    M, K = c["M"], c["K"]
    wt = G.build_weight(ops, P.case("plain", M, K, K), torch.eye(K, dtype=torch.float16), None, monkeypatch)
    out, rows, intact = G.out_buffer(ops, M, K, layout)
    ss = torch.full((K // 16, 32), float("nan"), dtype=torch.float32, device=DEV)
    ops.linear(G.operand(ops, mat["x"], layout, float("nan")), wt, out=out, ss_out=ss)
    torch.cuda.synchronize()
    assert torch.equal(rows().cpu(), mat["x"]) and intact(), f"{P.case_id(c)}: the producer of x did not hand x over"
    assert torch.equal(ss[:, :M].double().cpu(), mat["ss_x"]), f"{P.case_id(c)}: ss_out of the producer (exact sums)"
    return out, ss


def launch(ops, c, mat, layout, monkeypatch, norm):
    """One launch of case ``c`` on ``mat`` -> the outputs by name, on the CPU (the rope forms' caches as (M, Hkv, D) rows)."""
    M, N, K = c["M"], c["N"], c["K"]
    mode = P.mode_of(c)
    ln = mat["ln"].to(DEV) if norm else None
    eps = P.EPS if norm else 0.0
    ss_in = None
    if c.get("ss_in"):
        x, ss_in = _handoff(ops, c, mat, layout, monkeypatch)
    else:
        x = G.operand(ops, mat["x"], layout, float("nan"))
    wt = G.build_weight(ops, c, mat["ws"][0], mat["scale"], monkeypatch)
    with G.knobs(P.knobs_of(c)):
        if mode == P.SG_GATEUP:
            with G.sentinel_allocs(ops, monkeypatch):
                act = ops.mlp_act(x, wt, ln=ln, eps=eps, ss_in=ss_in)
                assert isinstance(act, ops.Act) == (layout == "packed")
                got = (act.rows() if layout == "packed" else act).cpu()
            return {"out": got}
        if mode in (P.SG_QKV, P.SG_QKVG):
            H, Hkv, D = c["H"], c["Hkv"], c["D"]
            T = P.SLOT0 + M + 5
            kc, vc = (torch.full((Hkv, T, D), SENTINEL, dtype=torch.float16, device=DEV) for _ in range(2))
            with G.sentinel_allocs(ops, monkeypatch):
                q = ops.qkv_rope(x, wt, ln, eps, mat["cos"].to(DEV), mat["sin"].to(DEV), mat["pos"].to(DEV), kc, vc, P.SLOT0, H, D,
                                 rotate_k=c.get("rotate_k", True), ss_in=ss_in, Hkv=Hkv).cpu()
            out = {"q": q}
            for name, cache in (("k", kc), ("v", vc)):
                cc = cache.cpu()
                inside = torch.zeros(T, dtype=torch.bool)
                inside[P.SLOT0:P.SLOT0 + M] = True
                assert bool((cc[:, ~inside] == SENTINEL).all()), f"{P.case_id(c)}: {name} cache written outside [slot0, slot0 + M)"
                out[name] = cc[:, inside].permute(1, 0, 2).contiguous()
            return out
        f32 = mode == P.SG_F32
        if f32:
            big, out = G.embed_rows(torch.full((M, N), SENTINEL, dtype=torch.float32), SENTINEL)
            rows, intact = (lambda: out.clone()), (lambda: bool((big[M:] == SENTINEL).all()))
        else:
            out, rows, intact = G.out_buffer(ops, M, N, layout)
        resid = None
        if c.get("resid"):
            if layout == "rows":                              # in place, as the decode layer runs it
                out.copy_(mat["res"].to(DEV))
                resid = out
            else:
                resid = G.embed_act(ops, mat["res"], float("nan"))
        ret = ops.linear(x, wt, out_f32=f32, ln=ln, eps=eps, resid=resid, out=out, ss_in=ss_in)
        assert ret is out
        got = rows().cpu()
        assert intact(), f"{P.case_id(c)}: output rows past M were written"
        return {"out": got}


def _site(c, what):
    kernel = "skinny_gemm_fp8_kernel" if c["ep"].endswith("_fp8") else "skinny_gemm_n8" if c["ep"].endswith("_n8") else "skinny_gemm_kernel"
    return f"{kernel} form {P.form_of(c)}: {what}"


@pytest.mark.parametrize("ci", range(len(Q.PROLOGUE_CASES)), ids=[P.case_id(c) for c in Q.PROLOGUE_CASES])
def test_norm_prologue(ci, monkeypatch):
    ops = _ops()
    ops._ensure_sg_workspace(DEV)
    c = Q.PROLOGUE_CASES[ci]
    for family in Q.FAMILIES:
        mat = Q.prologue_material(ci, family)
        want = Q.outputs_of(c, Q.prologue_expected(ci, family))
        one = Q.outputs_of(c, Q.prologue_expected(ci, family, one_rounding=True))
        for layout in P.LAYOUTS:
            got = launch(ops, c, mat, layout, monkeypatch, norm=True)
            for key in want:
                check(_site(c, f"norm prologue fp16(x * inv), output {key}"), f"{Q.prologue_id(c, family)} [{layout}]",
                      got[key], want[key], one[key])


@pytest.mark.parametrize("ci", range(len(Q.F8_EPILOGUE_CASES)), ids=[P.case_id(c) for c in Q.F8_EPILOGUE_CASES])
def test_fp8_epilogue(ci, monkeypatch):
    ops = _ops()
    c = Q.F8_EPILOGUE_CASES[ci]
    mat = Q.f8_material(ci)
    want, one = Q.f8_expected(ci), Q.f8_expected(ci, one_rounding=True)
    for layout in P.LAYOUTS:
        got = launch(ops, c, mat, layout, monkeypatch, norm=False)
        for key in want:
            check(_site(c, f"epilogue fp16(s[n] * acc), output {key}"), f"{P.case_id(c)} [{layout}]", got[key], want[key], one[key])


# ---- retrieval ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(Q.RETRIEVAL_CASES)), ids=[Q.retrieval_id(c) for c in Q.RETRIEVAL_CASES])
def test_retrieval(ci):
    """The one-pass scorer, the chunk-mean index (built in the case's pieces) and the indexed scorer against the expectation,
    and the bit-identity of the two scorers, on the same material."""
    ops = _ops()
    name, C, H, D, chunk, _, pieces = Q.RETRIEVAL_CASES[ci]
    m = Q.retrieval_material(ci)
    k = m["k"].to(DEV)
    index = torch.full((H, C + 2, D), SENTINEL, dtype=torch.float16, device=DEV)
    for c0, c1 in pieces:
        ops.chunk_mean(k, index, c0, c1, chunk)
    torch.cuda.synchronize()
    got_index = index.cpu()
    cid = Q.retrieval_id(Q.RETRIEVAL_CASES[ci])
    failures, reported = [], set()                            # every site reports once, so one run names all that fold

    def site(what, where, got, want, one):
        kernel = what.split(":")[0]
        msg = report(what, where, got, want, one)
        if msg is not None and kernel not in reported:
            reported.add(kernel)
            failures.append(f"{cid} " + msg)

    site(f"chunk_mean_kernel<{D}>: fp16(sum * (1 / {chunk}))", "index rows (head, chunk, d)", got_index[:, :C],
         torch.from_numpy(m["mean"]), torch.from_numpy(m["mean1"]))
    assert bool((got_index[:, C:] == SENTINEL).all()), f"{name}: index rows past the last chunk were written"
    want_index = torch.from_numpy(m["mean"]).to(DEV)         # the indexed scorer is judged over the RIGHT index
    index[:, :C] = want_index
    identical = True
    for t, (q, d, val) in enumerate(Q.retrieval_queries(ci)):
        want = torch.from_numpy(Q.retrieval_scores(m["mean"], d, val))
        one = torch.from_numpy(Q.retrieval_scores(m["mean1"], d, val))
        qd = q.to(DEV)
        direct = ops.retrieval_score(k, qd, C, chunk).cpu()
        indexed = ops.retrieval_score_indexed(index, qd, C).cpu()
        where = f"query {t} (d_h = {d[:4].tolist()}..) scores (head, chunk)"
        site(f"retrieval_score_kernel<{D}>: fp16(sum * (1 / {chunk}))", where, direct, want, one)
        site(f"retrieval_score_indexed_kernel<{D}>: over the expected index", where, indexed, want, one)
        identical &= torch.equal(direct, indexed)
    assert not failures, "\n".join(failures)
    assert identical and torch.equal(got_index[:, :C], torch.from_numpy(m["mean"])), \
        f"{name}: index + indexed scorer is not bit-identical to the one-pass scorer"
