"""The material of the rounding probes (tests/rounding_probes.py), proved on the CPU: every exactness condition holds over the
whole case list, the restatement's fp32 square root and reciprocal are correctly rounded (Fraction check on the cases' own
sums), the restatement equals oracle.ref_ops.rms_norm wherever torch's rsqrt gives the same inv, and — the vacuity guard — the
one-rounding counter-model differs from the expectation at exactly the recorded witness elements, which an integer model of the
two roundings (``r16`` / ``r32`` below, Fractions only) confirms independently.  The quota (>= 8 witness elements that reach an
output per case, >= 64 per site family, two rows, both halves of a 16-byte vector) is a condition, not a measurement.

Removed cases, by name (reasons in the docstring of tests/rounding_probes.py): gate-side witnesses of every gate|up case; ss_out of
the probed GEMMs; retrieval witnesses at |k| <= 8 for chunks 12 and 24 (none exist: proved below); draft_persist's dp_normalise.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import ref_ops as R
from tests import gemm_probes as P
from tests import rounding_probes as Q


# ---- an integer model of the two roundings ----------------------------------------------------------------------------------------
def _round_to(fr, bits, emin):
    """Fraction -> nearest value with ``bits`` significant bits (ties to even), gradual underflow below 2^emin.  No overflow here."""
    if fr == 0:
        return Fraction(0)
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    q = Fraction(2) ** (max(e, emin) - (bits - 1))
    n = a / q
    f = n.numerator // n.denominator
    rem = n - f
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and f % 2):
        f += 1
    return (f * q) * (1 if fr > 0 else -1)


def r32(fr):
    return _round_to(fr, 24, -126)


def r16(fr):
    return _round_to(fr, 11, -14)


def is_witness(a, b):
    p = Fraction(float(a)) * Fraction(float(b))
    return r16(r32(p)) != r16(p)


def test_numpy_rounds_float64_to_float16_once_and_the_integer_model_agrees():
    v = 1.0 + 2.0 ** -11 + 2.0 ** -30                       # through fp32 this is a tie and goes to 1.0
    assert float(np.float64(v).astype(np.float16)) == 1.0 + 2.0 ** -10
    assert float(np.float64(v).astype(np.float32).astype(np.float16)) == 1.0
    assert r16(Fraction(v)) == Fraction(1.0 + 2.0 ** -10) and r16(r32(Fraction(v))) == 1
    g = np.random.default_rng(5)
    a = g.uniform(0.25, 2.0, 4000).astype(np.float32)
    b = g.standard_normal(4000).astype(np.float16).astype(np.float32)
    two, one = Q.f16_two(a, b), Q.f16_one(a, b)
    for i in range(a.size):
        p = Fraction(float(a[i])) * Fraction(float(b[i]))
        assert Fraction(float(two[i])) == r16(r32(p)) and Fraction(float(one[i])) == r16(p)
    for s, x in Q.F8_PAIRS:                                 # the frozen pairs are witnesses, by integers
        sv, xv = Q.pair(Q.F8_PAIRS.index((s, x)))
        assert is_witness(sv, xv) and 2.0 ** -6 <= float(xv) < 4.0 and 0.25 <= float(sv) < 2.0


# ---- norm rows ----------------------------------------------------------------------------------------------------------------------
def test_row_sums_are_exact_in_fp32_in_any_order():
    for hidden in Q.all_hidden():
        jm = Q.jmax_of(hidden)
        assert hidden * jm * jm < 2 ** 24 and hidden % 8 == 0 and len(Q.ROW_SEEDS[hidden]) == Q.WITNESS_ROWS_PER_CASE
        for seed in Q.ROW_SEEDS[hidden]:
            assert int(np.abs(Q.row_j(hidden, seed)).max()) <= jm and Q.is_witness_row(hidden, seed)


def _on_grid(x, bound):
    j = x.astype(np.float64) / Q.UNIT
    return bool((j == np.round(j)).all()) and float(np.abs(j).max()) <= bound


def test_rmsnorm_material_is_on_the_grid():
    assert {c[0] for c in Q.RMS_CASES} == set(Q.RMS_HIDDEN) == {256, 2048, 2056, 4096, 5120} and {c[1] for c in Q.RMS_CASES} == {1, 3}
    for c in Q.RMS_CASES:
        m = Q.rms_material(c)
        jm = Q.jmax_of(c[0])
        assert (m["res"] is None) == (c[2] == "plain")
        if m["res"] is not None:
            assert _on_grid(m["x"], 2 * jm) and _on_grid(m["res"], jm)
            exact = m["x"].astype(np.float64) + m["res"].astype(np.float64)
            assert (m["sum"].astype(np.float64) == exact).all(), "x + res is not exact in fp16"
        assert _on_grid(m["sum"], jm)
        ss_units = m["ss"] / (Q.UNIT * Q.UNIT)
        assert (ss_units == np.round(ss_units)).all() and float(ss_units.max()) < 2 ** 24
    for hidden in Q.RMS_HIDDEN:
        for rows in Q.RMS_ROWS:
            m = Q.rms_control(hidden, rows)
            assert (np.abs(m["n"].astype(np.float64)) == 1.0).all() and (m["n"] == m["n1"]).all()      # inv = 2^-k: no witness
            lg = np.log2(m["inv"].astype(np.float64))
            assert (lg == np.round(lg)).all()


def _norm_materials():
    for c in Q.RMS_CASES:
        yield Q.rms_id(c), Q.rms_material(c)
    for ci, c in enumerate(Q.PROLOGUE_CASES):
        m = Q.prologue_material(ci, "w1")
        x = m["x"].numpy()
        yield P.case_id(c), dict(Q.norm_host(x, m["ln"].numpy(), P.EPS), eps=P.EPS, w=m["ln"].numpy())


def test_sqrt_and_reciprocal_of_the_restatement_are_correctly_rounded():
    seen = set()
    for name, m in _norm_materials():
        hidden = m["sum"].shape[1]
        for ss, inv in zip(m["ss"], m["inv"][:, 0]):
            key = (float(ss), hidden)
            if key in seen:
                continue
            seen.add(key)
            v = np.float32(ss) / np.float32(hidden) + np.float32(m["eps"])
            assert Fraction(float(v)) == r32(r32(Fraction(float(ss)) / hidden) + Fraction(float(np.float32(m["eps"])))), name
            root = np.sqrt(np.float64(v)).astype(np.float32)
            lo = (Fraction(float(root)) + Fraction(float(np.nextafter(root, np.float32(0))))) / 2
            hi = (Fraction(float(root)) + Fraction(float(np.nextafter(root, np.float32(np.inf))))) / 2
            assert lo * lo < Fraction(float(v)) < hi * hi, name
            assert Fraction(float(inv)) == r32(1 / Fraction(float(root))), name
    assert len(seen) > 100


def test_restatement_equals_the_oracle_where_torch_rsqrt_gives_the_same_inv():
    same = rows = 0
    for name, m in _norm_materials():
        x = torch.from_numpy(m["sum"])
        var = x.float().pow(2).mean(-1, keepdim=True)
        t_inv = torch.rsqrt(var + m["eps"]).numpy()
        eq = (t_inv == m["inv"])[:, 0]
        want = R.rms_norm(x, torch.from_numpy(m["w"]), m["eps"]).numpy()
        got = m["y"]
        assert (want[eq] == got[eq]).all(), name
        same += int(eq.sum())
        rows += eq.size
    print(f"torch's rsqrt gives the restatement's inv on {same} of {rows} rows; the others are not asserted")
    assert same > rows // 2


def _norm_witness_by_integers(m):
    """(M, K) bool from the integer model, evaluated once per distinct (row, |x|)."""
    x = m["sum"].astype(np.float32)
    out = np.zeros(x.shape, bool)
    for r in range(x.shape[0]):
        inv = m["inv"][r, 0]
        for v in np.unique(np.abs(x[r])):
            out[r, np.abs(x[r]) == v] = is_witness(v, inv)
    return out


def _halves(cols):
    cols = np.asarray(cols)
    return bool((cols % 8 < 4).any()) and bool((cols % 8 >= 4).any())


def test_rmsnorm_vacuity_guard_and_quota():
    total = 0
    for c in Q.RMS_CASES:
        m = Q.rms_material(c)
        wit = m["n"] != m["n1"]
        assert (wit == _norm_witness_by_integers(m)).all(), Q.rms_id(c)
        reach = m["y"] != m["y1"]
        assert not (reach & ~wit).any()
        if c[3] == "w1":
            assert (reach == wit).all() and (m["y"] == m["n"]).all()
        assert int(reach.sum()) >= 8, Q.rms_id(c)
        assert reach.any(1).all(), "a row without a witness"                       # every row (1 or 3) holds witnesses
        assert _halves(np.nonzero(reach)[1]), Q.rms_id(c)
        total += int(reach.sum())
    assert total >= 64


# ---- GEMM prologue ------------------------------------------------------------------------------------------------------------------
def test_prologue_case_list_reaches_every_form_with_a_prologue():
    forms = {P.form_of(c) for c in Q.PROLOGUE_CASES}
    assert not [f for f in Q.PROLOGUE_FORMS_REQUIRED if f not in forms]
    assert forms == {P.form_of(c) for c in P.CASES if c["norm"]}
    assert {(c["ep"], P.form_of(c)) for c in Q.PROLOGUE_CASES} == {(c["ep"], P.form_of(c)) for c in P.CASES if c["norm"]}
    eps = {c["ep"] for c in Q.PROLOGUE_CASES}
    assert eps == {c["ep"] for c in P.CASES if c["norm"]}
    for ep in ("plain", "gateup_n8", "qkv_n8", "plain_fp8", "gateup_fp8"):
        assert any(c["ep"] == ep and c.get("ss_in") for c in Q.PROLOGUE_CASES), ep
    assert all(c in P.CASES for c in Q.PROLOGUE_CASES)                              # that module's shapes, not restated ones


def _source_mask(c, src):
    """(M, S N) bool at the y level -> dict of masks shaped like the compared outputs: which outputs a y element can reach."""
    M, N = c["M"], c["N"]
    mode = P.mode_of(c)
    if mode == P.SG_GATEUP:
        return {"out": src[:, :N] | src[:, N:]}
    if mode in (P.SG_QKV, P.SG_QKVG):
        H, Hkv, D = c["H"], c["Hkv"], c["D"]
        q, k, v = src[:, :H * D].view(M, H, D), src[:, H * D:(H + Hkv) * D].view(M, Hkv, D), src[:, (H + Hkv) * D:].view(M, Hkv, D)
        mix = lambda t: t | torch.cat([t[..., D // 2:], t[..., :D // 2]], dim=-1)
        return {"q": mix(q), "k": mix(k), "v": v}
    return {"out": src}


@pytest.mark.parametrize("family", Q.FAMILIES)
def test_prologue_vacuity_guard_and_quota(family):
    total = 0
    for ci, c in enumerate(Q.PROLOGUE_CASES):
        name = Q.prologue_id(c, family)
        m = Q.prologue_material(ci, family)
        M, N, K, S = c["M"], c["N"], c["K"], P.streams_of(c)
        x = m["x"].numpy()
        assert _on_grid(x, Q.jmax_of(K)) and K * Q.jmax_of(K) ** 2 < 2 ** 24, name
        nh = Q.norm_host(x, m["ln"].numpy(), P.EPS)
        wit = nh["n"] != nh["n1"]
        assert (wit == _norm_witness_by_integers(nh)).all() and (torch.from_numpy(wit) == m["wit"]).all(), name
        kk, w = m["ks"][0], m["ws"][0].double()
        assert ((w != 0).sum(1) == 1).all() and (w[torch.arange(S * N), kk] != 0).all(), name         # one term per output row
        e, e1 = Q.prologue_expected(ci, family), Q.prologue_expected(ci, family, one_rounding=True)
        assert e["y_exact"] and e1["y_exact"], name
        src = (m["h"] != m["h1"])[:, kk]
        assert ((e["y"] != e1["y"]) == src).all(), name                                               # at the y level: exactly
        assert not (src & ~m["wit"][:, kk]).any(), name
        if family == "w1":
            assert (src == m["wit"][:, kk]).all(), name
        if S == 2:
            assert bool(e["safe"].all()) and bool(e1["safe"].all()), name                             # every gate boundary-safe
            assert not m["wit"][:, kk[:N]].any() and (e["y"][:, :N] == e1["y"][:, :N]).all(), name    # and witness-free
        masks, reach = _source_mask(c, src), 0
        outs, outs1 = Q.outputs_of(c, e), Q.outputs_of(c, e1)
        rows_hit = set()
        for key in outs:
            d = outs[key] != outs1[key]
            assert not (d & ~masks[key]).any(), (name, key)                                           # nowhere else
            reach += int(d.sum())
            rows_hit |= set(d.nonzero()[:, 0].tolist())
        up_cols = kk[(S - 1) * N:][src[:, (S - 1) * N:].any(0)]
        assert reach >= 8, (name, reach)
        assert M == 1 or len(rows_hit) >= 2, name
        assert _halves(up_cols.numpy()), name            # the halves of the INPUT vector the prologue loads: the selected columns
        total += reach
    assert total >= 64


# ---- FP8 epilogue -------------------------------------------------------------------------------------------------------------------
def test_fp8_epilogue_vacuity_guard_and_quota():
    forms = {P.form_of(c) for c in Q.F8_EPILOGUE_CASES}
    assert forms == {("f8", mt, w) for mt in (1, 2) for w in (4, 8)}
    assert {P.mode_of(c) for c in Q.F8_EPILOGUE_CASES} == {P.SG_PLAIN, P.SG_F32, P.SG_QKV, P.SG_GATEUP}
    total = 0
    for ci, c in enumerate(Q.F8_EPILOGUE_CASES):
        name = P.case_id(c)
        m = Q.f8_material(ci)
        M, N, S = c["M"], c["N"], P.streams_of(c)
        kk, w = m["ks"][0], m["ws"][0]
        assert ((w != 0).sum(1) == 1).all() and torch.equal(w.to(torch.float8_e4m3fn).half(), w), name       # exact e4m3 codes
        scale = m["scale"].numpy()
        assert (scale.astype(np.float32).astype(np.float64) == scale).all(), name
        y, y1, acc = m["y"], m["y1"], m["acc"]
        assert float(np.abs(y.astype(np.float64)).min()) >= 2.0 ** -14 and np.isfinite(y.astype(np.float64)).all(), name
        d = y != y1
        byint = np.zeros_like(d)
        for mm, n in zip(*np.nonzero(np.ones_like(d))):
            byint[mm, n] = is_witness(np.float32(scale[n]), np.float32(acc[mm, n]))
        assert (d == byint).all(), name                                                                      # exactly the witnesses
        planted = np.zeros_like(d)
        planted[np.ix_(Q.witness_row_slots(M), range((S - 1) * N, S * N))] = True
        assert d[planted].all(), name                                                                        # every planted pair
        if S == 2:
            assert (y[:, :N] == np.float16(16.0)).all() and (scale[:N] == 1.0).all() and not d[:, :N].any(), name
            g = 16.0 / (1.0 + np.exp(-16.0))
            assert abs(g / 16.0 - 1.0) < 1.2e-7 and np.float64(g).astype(np.float16) == np.float16(16.0)
        if P.mode_of(c) == P.SG_QKV:
            assert not m["pos"].any() and bool((m["cos"][0] == 1).all()) and not bool(m["sin"][0].any()), name
        e, e1 = Q.f8_expected(ci), Q.f8_expected(ci, one_rounding=True)
        reach, rows_hit, cols_hit = 0, set(), set()
        for key in e:
            dd = e[key] != e1[key]
            reach += int(dd.sum())
            nz = dd.nonzero()
            rows_hit |= set(nz[:, 0].tolist())
            cols_hit |= set(nz[:, -1].tolist())
        assert reach >= 8 and (M == 1 or len(rows_hit) >= 2) and _halves(sorted(cols_hit)), (name, reach)
        total += reach
    assert total >= 64


# ---- retrieval ----------------------------------------------------------------------------------------------------------------------
def test_mean_witness_table_by_integers():
    for chunk in (8, 16):
        assert Q.mean_witness_sums(chunk).size == 0                      # a power-of-two chunk: acc * inv is exact
    for chunk in (12, 24):
        inv = np.float32(1.0) / np.float32(chunk)
        assert Fraction(float(inv)) == r32(Fraction(1, chunk))
        ws = Q.mean_witness_sums(chunk)
        assert ws.size > 0 and int(ws.min()) > 128 * chunk                # none within reach of |k| <= 8
        for a in ws[:: max(1, ws.size // 200)]:
            assert is_witness(np.float32(a * Q.UNIT), inv)
        for a in range(1, 128 * chunk + 1, 7):
            assert not is_witness(np.float32(a * Q.UNIT), inv)


def test_retrieval_vacuity_guard_and_quota():
    names = {c[0] for c in Q.RETRIEVAL_CASES}
    assert {"smallest", "second-trip"} <= names and Q.RETRIEVAL_CASES[0][1:5] == (3, 1, 64, 8)
    total = 0
    for ci, c in enumerate(Q.RETRIEVAL_CASES):
        name, C, H, D, chunk, bound, pieces = c
        m = Q.retrieval_material(ci)
        assert int(np.abs(m["rows"]).max()) <= bound <= 1024 and chunk * bound < 2 ** 24
        assert torch.equal(m["k"].double(), torch.from_numpy(m["rows"].reshape(H, C * chunk, D) * Q.UNIT))  # exact in fp16
        assert pieces[0][0] == 0 and pieces[-1][1] == C and all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))
        units = np.round(np.abs(m["acc"]) / Q.UNIT).astype(np.int64)
        d = m["mean"] != m["mean1"]
        assert (d == np.isin(units, Q.mean_witness_sums(chunk))).all(), name                                 # exactly the table's sums
        qs = Q.retrieval_queries(ci)
        seen = np.zeros((H, D), bool)
        reach = 0
        for q, dh, val in qs:
            seen[np.arange(H), dh] = True
            s, s1 = Q.retrieval_scores(m["mean"], dh, val), Q.retrieval_scores(m["mean1"], dh, val)
            assert ((s != s1) == d[np.arange(H), :, dh]).all(), name
            reach += int((s != s1).sum())
        assert seen.all() if len(qs) > 1 else (H >= D and seen.any(0).all()), name      # every d of every head | every d over the heads
        if chunk in (8, 16):
            assert not d.any(), name
            continue
        assert reach >= 8 and len(set(np.nonzero(d)[1].tolist())) >= 2 and _halves(np.nonzero(d)[2]), name
        total += reach
    assert total >= 64
    # the grid-stride loop takes a second trip: workgroup cap 2048 / H, 2048 / D chunk groups per workgroup
    _, C, H, D, _, _, _ = next(c for c in Q.RETRIEVAL_CASES if c[0] == "second-trip")
    assert C > (2048 // H) * (2048 // D)
