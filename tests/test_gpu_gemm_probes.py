"""The skinny decode GEMMs on exact-arithmetic inputs (tests/gemm_probes.py): every output must come back BIT FOR BIT
(torch.equal) at every entry point, activation layout, kernel form and K edge of the case list — whatever order the kernel adds
in.  Two allowances only, both from the issue that asked for these probes: SwiGLU elements whose fp16(silu(g)) sits within
DELTA of an fp16 boundary may differ by |up| x one fp16 spacing of fp16(silu(g)) (at most 1 % of a case's elements, asserted on
the CPU), and ss_out of the residual form is compared with the float64 sum at rtol 2e-6.

Poison.  Every operand is embedded: row-major x / resid are the first M rows of a 40-row buffer whose other rows are NaN, an
Act has R = M + 3 rows with NaN in rows M .., ss_in holds NaN in its columns M ..; every output — y, Act rows >= M, the
SwiGLU output and q (allocated by ops: its allocations are wrapped), the K / V cache outside [slot0, slot0 + M) — is pre-filled
with a sentinel that must come back untouched.  ss_out columns >= M: include/triforce_hip.h promises nothing about them
(the 16-bit kernel writes zeros up to its row tile, nothing past it), so nothing is asserted there.  After a launch that split K
across workgroups the ticket words of the workspace are zero; every tf_sg_tune key is back at its value afterwards.
"""
import contextlib

import pytest
import torch

from tests import gemm_probes as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD_ROWS, ACT_PAD = 40, 3
SS_SENTINEL = -7.0
STATS = {"unsafe": 0, "swiglu": 0, "moved": 0}


def _ops():
    from triforce_amd import ops
    return ops


def _lib():
    from triforce_amd import hip
    return hip.lib()


@contextlib.contextmanager
def knobs(setting):
    """Every tf_sg_tune key at the case's value; the previous values back in a ``finally``, and checked."""
    L = _lib()
    old = {}
    try:
        for k, v in setting.items():
            old[k] = L.tf_sg_tune(k, v)
        yield
    finally:
        for k in reversed(list(old)):
            L.tf_sg_tune(k, old[k])
    for k, v in old.items():
        now = L.tf_sg_tune(k, v)
        assert now == v, f"tf_sg_tune key {k}: {now} after the case, {v} before"


class _SentinelTorch:
    """Stands in for ``torch`` inside triforce_amd.ops: ``empty`` hands out the first rows of a sentinel-filled buffer."""

    def __init__(self):
        self.bufs = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, **kw):
        big = torch.full((shape[0] + ACT_PAD,) + tuple(shape[1:]), P.SENTINEL, **kw)
        self.bufs.append((big, shape[0]))
        return big[:shape[0]]


@contextlib.contextmanager
def sentinel_allocs(ops, monkeypatch):
    """Outputs that ops allocates itself (the SwiGLU output, q) come from sentinel-filled buffers with spare rows; on exit the
    spare rows must be untouched."""
    st = _SentinelTorch()
    acts = []

    def act_empty(cls, M, K, device, R=None):
        a = cls(torch.full((K // 8, M + ACT_PAD, 8), P.SENTINEL, dtype=torch.float16, device=device), M)
        acts.append(a)
        return a
    with monkeypatch.context() as mp:
        mp.setattr(ops, "torch", st)
        mp.setattr(ops.Act, "empty", classmethod(act_empty))
        yield
    torch.cuda.synchronize()
    for big, rows in st.bufs:
        assert bool((big[rows:] == P.SENTINEL).all()), "rows past M of an output ops allocated were written"
    for a in acts:
        assert bool((a.t[:, a.M:] == P.SENTINEL).all()), "Act rows past M of an output ops allocated were written"


def embed_rows(x, fill):
    """x (M, ...) as the first M rows of a PAD_ROWS-row device buffer filled with ``fill``."""
    big = torch.full((PAD_ROWS,) + tuple(x.shape[1:]), fill, dtype=x.dtype, device=DEV)
    big[:x.shape[0]] = x.to(DEV)
    return big, big[:x.shape[0]]


def embed_act(ops, x, fill):
    """x (M, K) as an Act of R = M + ACT_PAD rows, rows M .. filled with ``fill``."""
    M, K = x.shape
    t = torch.full((K // 8, M + ACT_PAD, 8), fill, dtype=torch.float16, device=DEV)
    t[:, :M] = x.to(DEV).view(M, K // 8, 8).permute(1, 0, 2)
    return ops.Act(t, M)


def operand(ops, x, layout, fill):
    return embed_act(ops, x, fill) if layout == "packed" else embed_rows(x, fill)[1]


def out_buffer(ops, M, N, layout):
    """-> (what to pass as ``out``, rows() -> (M, N) result, intact() -> the spare rows still hold the sentinel)."""
    if layout == "packed":
        a = embed_act(ops, torch.full((M, N), P.SENTINEL, dtype=torch.float16), P.SENTINEL)
        return a, a.rows, lambda: bool((a.t[:, M:] == P.SENTINEL).all())
    big, view = embed_rows(torch.full((M, N), P.SENTINEL, dtype=torch.float16), P.SENTINEL)
    return view, lambda: view.clone(), lambda: bool((big[M:] == P.SENTINEL).all())


def install_fp8(ops, pl, scale_nat):
    """The codes of an (exactly e4m3-representable) fp16 weight with the probe's row scales 2^(n % 5 - 2), n the row of the
    natural order: a scale read at another row's index shows as a wrong power of two."""
    f8 = ops.Fp8Linear(pl)
    sc = scale_nat.float().to(DEV)
    if f8.rope is not None:
        sc = sc[ops.rope_row_order(f8.rope[0], f8.rope[0], f8.rope[1], DEV)]
    for codes, scales, blk, s in zip(f8.codes, f8.scales, f8._streams(), sc.chunk(len(f8.codes))):
        codes.copy_(ops.pack_weight_fp8(blk.to(torch.float8_e4m3fn).view(torch.uint8)))
        scales.copy_(s)
    assert torch.equal(f8.dequantized().double().cpu(), pl.w.double().cpu() * scale_nat[:, None])
    return f8


def build_weight(ops, c, w, scale, monkeypatch):
    ep = c["ep"]
    with monkeypatch.context() as mp:
        if not ep.endswith("_n8"):
            mp.setattr(ops, "N8_ENABLED", False)                 # the 16-row forms, whatever the shape
        wd = w.to(DEV)
        if P.mode_of(c) == P.SG_GATEUP:
            pl = ops.PackedLinear(wd, split=2)
        elif ep.startswith("qkv"):
            pl = ops.PackedLinear(wd, rope=(c["H"], c["Hkv"], c["D"]))
        else:
            pl = ops.PackedLinear(wd)
    if ep == "gateup_n8":
        assert pl.parts_n8 is not None
    if ep == "qkv_n8":
        assert pl.wp_rope_n8 is not None
    return install_fp8(ops, pl, scale) if ep.endswith("_fp8") else pl


def first_diff(got, want):
    bad = (got != want).nonzero()
    return None if bad.numel() == 0 else tuple(int(v) for v in bad[0])


def explain(c, kind, mat, li, idx, got, want, where=None):
    """A failure by name: the element, and for the select probe the (m, n, k) it pins.  ``where``: "q" (m, head, d) | "k" | "v"
    (head, slot, d) for the rope forms — a rotated element mixes weight row n with its partner n +- D / 2."""
    s = f"{P.case_id(c)} [{kind}, launch {li}] form {P.form_of(c)}: element {idx}: got {float(got[idx])!r}, expected {float(want[idx])!r}"
    if kind != "select":
        return s
    if where is None:
        m, n = idx
    else:
        H, Hkv, D = c["H"], c["Hkv"], c["D"]
        m, n = (idx[0], idx[1] * D + idx[2]) if where == "q" else (idx[1] - P.SLOT0, (H + (Hkv if where == "v" else 0) + idx[0]) * D + idx[2])
    if not 0 <= m < c["M"]:
        return s + " — a slot outside [slot0, slot0 + M): the sentinel was overwritten"
    kk = mat["ks"][li]
    s += f" — row m = {m}, weight row n = {n} selects k = {int(kk[n])}"
    if P.streams_of(c) == 2:
        s += f" (gate), up row selects k = {int(kk[c['N'] + n])}"
    if where in ("q", "k"):
        pn = n + c["D"] // 2 if idx[2] < c["D"] // 2 else n - c["D"] // 2
        s += f" (rotary partner n = {pn} selects k = {int(kk[pn])})"
    return s


def run_case(ops, c, kind, layout, monkeypatch):
    M, N, K = c["M"], c["N"], c["K"]
    mat = P.material(c, kind)
    mode = P.mode_of(c)
    x = operand(ops, mat["x"], layout, float("nan"))
    ln = mat["ln"].to(DEV) if mat["ln"] is not None else None
    eps = P.EPS if ln is not None else 0.0
    ss_in = None
    if c.get("ss_in"):
        ss_in = torch.full((K // 16, 32), float("nan"), dtype=torch.float32, device=DEV)
        ss_in[:, :M] = mat["ss_x"].float().to(DEV)
    split = P.form_of(c)[0] == "sg" and P.form_of(c)[4] > 1
    for li, w in enumerate(mat["ws"]):
        e = P.expected(c, mat, li)
        wt = build_weight(ops, c, w, mat["scale"], monkeypatch)

        def fail(idx, got, want, where=None):
            return explain(c, kind, mat, li, idx, got, want, where)
        if mode == P.SG_GATEUP:
            with sentinel_allocs(ops, monkeypatch):
                act = ops.mlp_act(x, wt, ln=ln, eps=eps, ss_in=ss_in)
                assert isinstance(act, ops.Act) == (layout == "packed")
                got = (act.rows() if layout == "packed" else act).cpu()
            safe, want = e["safe"], e["out"]
            bad = (got != want) & safe
            assert not bool(bad.any()), fail(first_diff(torch.where(safe, got, want), want), got, want)
            d = (got.double() - want.double()).abs()
            assert bool((d <= e["tol"])[~safe].all()), (P.case_id(c), kind, float((d - e["tol"])[~safe].max()))
            STATS["unsafe"] += int((~safe).sum())
            STATS["swiglu"] += safe.numel()
            STATS["moved"] += int((got != want).sum())
        elif mode in (P.SG_QKV, P.SG_QKVG):
            H, Hkv, D = c["H"], c["Hkv"], c["D"]
            T = P.SLOT0 + M + 5
            kc = torch.full((Hkv, T, D), P.SENTINEL, dtype=torch.float16, device=DEV)
            vc = torch.full((Hkv, T, D), P.SENTINEL, dtype=torch.float16, device=DEV)
            with sentinel_allocs(ops, monkeypatch):
                q = ops.qkv_rope(x, wt, ln, eps, mat["cos"].to(DEV), mat["sin"].to(DEV), mat["pos"].to(DEV), kc, vc, P.SLOT0, H, D,
                                 rotate_k=c.get("rotate_k", True), ss_in=ss_in, Hkv=Hkv).cpu()
            assert torch.equal(q, e["q"]), fail(first_diff(q, e["q"]), q, e["q"], "q")
            for name, cache, rows in (("k", kc, e["k"]), ("v", vc, e["v"])):
                want = torch.full((Hkv, T, D), P.SENTINEL, dtype=torch.float16)
                want[:, P.SLOT0:P.SLOT0 + M] = rows.permute(1, 0, 2)
                got = cache.cpu()
                assert torch.equal(got, want), f"{name} cache (head, slot, d): " + fail(first_diff(got, want), got, want, name)
        else:
            f32 = mode == P.SG_F32
            if f32:
                big, out = embed_rows(torch.full((M, N), P.SENTINEL, dtype=torch.float32), P.SENTINEL)
                rows, intact = (lambda: out.clone()), (lambda: bool((big[M:] == P.SENTINEL).all()))
            else:
                out, rows, intact = out_buffer(ops, M, N, layout)
            resid = None
            if c.get("resid"):
                if layout == "rows":                              # in place, as the decode layer runs it
                    out.copy_(mat["res"].to(DEV))
                    resid = out
                else:
                    resid = embed_act(ops, mat["res"], float("nan"))
            ss = None
            if P.wants_ss_out(c, kind):
                ss = torch.full((N // 16, 32), SS_SENTINEL, dtype=torch.float32, device=DEV)
            ret = ops.linear(x, wt, out_f32=f32, ln=ln, eps=eps, resid=resid, out=out, ss_in=ss_in, ss_out=ss)
            assert ret is out
            got, want = rows().cpu(), e["out"]
            assert got.dtype == want.dtype and torch.equal(got, want), fail(first_diff(got, want), got, want)
            assert intact(), f"{P.case_id(c)}: output rows past M were written"
            if ss is not None:
                got_ss = ss[:, :M].double().cpu()
                if P.ss_exact(c, kind):
                    assert torch.equal(got_ss, e["ss"]), (P.case_id(c), kind, "ss_out", first_diff(got_ss, e["ss"]))
                else:
                    torch.testing.assert_close(got_ss, e["ss"], rtol=2e-6, atol=0.0)
        if split:
            torch.cuda.synchronize()
            ws = ops._SG_WS[torch.device(DEV)]
            slot = ws.numel() // 4
            assert all(int(ws[i * slot:i * slot + 4 * P.SG_TICKETS].sum()) == 0 for i in range(4)), "tickets were not left zero"


@pytest.mark.parametrize("c", P.CASES, ids=[P.case_id(c) for c in P.CASES])
def test_gemm_probe(c, monkeypatch):
    ops = _ops()
    ops._ensure_sg_workspace(DEV)
    assert torch.device(DEV) in ops._SG_WS, "split-K workspace was not registered"
    with knobs(P.knobs_of(c)):
        for kind in P.KINDS:
            for layout in P.LAYOUTS:
                run_case(ops, c, kind, layout, monkeypatch)


def test_zz_swiglu_allowance_on_record():
    """How much of the SwiGLU allowance the device used over the cases above (a figure, not a bound: the bounds are asserted
    per element in test_gemm_probe)."""
    from tests import helpers
    if STATS["swiglu"]:
        helpers.note(f"gemm probes, SwiGLU: {STATS['unsafe']} of {STATS['swiglu']} elements boundary-unsafe "
                     f"({100.0 * STATS['unsafe'] / STATS['swiglu']:.3f} %), {STATS['moved']} differ from the float64 expectation")
