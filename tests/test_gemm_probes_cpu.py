"""The material, the conditions and the case list of the decode-GEMM probes (tests/gemm_probes.py), proved on the CPU: select
and dense inputs are exact on the oracle pipeline (R.rms_norm, R.linear, R.apply_rope, R.silu_mul on boundary-safe elements),
every condition that makes fp32 sums order-free holds for every case and seed, the edge set E(K) is selected by every case, the
Python restatement of the launch rule agrees with csrc/sg_rule.h on every case and knob setting, and the list reaches every
kernel form the dispatchers build."""
import functools
import os
import shutil
import subprocess

import pytest
import torch

from oracle import ref_ops as R
from tests import gemm_probes as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [(i, kind) for i in range(len(P.CASES)) for kind in P.KINDS]


@functools.lru_cache(maxsize=None)
def built(i, kind):
    c = P.CASES[i]
    mat = P.material(c, kind)
    return c, mat, [P.expected(c, mat, li) for li in range(len(mat["ws"]))]


def test_case_list_reaches_every_entry_point_and_form():
    forms = {}
    for c in P.CASES:
        forms.setdefault(P.form_of(c), []).append(P.case_id(c))
    missing = [f for f in P.FORMS_REQUIRED if f not in forms]
    assert not missing, missing
    assert {c["ep"] for c in P.CASES} == set(P.ENTRY_POINTS)
    by_ep = {}
    for c in P.CASES:
        by_ep.setdefault(c["ep"], []).append(c)
    for ep, cs in by_ep.items():
        if ep in ("plain", "f32", "gateup", "qkv", "qkvg") or ep.endswith("_fp8"):
            assert {c["norm"] for c in cs} == {False, True}, ep                  # with and without the norm prologue
        print(f"{ep}: {len(cs)} cases, forms {sorted({P.form_of(c) for c in cs})}")
    # the knob keys the issue names, and the forced split that must shrink
    used = {k for c in P.CASES for k, _ in c["knobs"]}
    assert {0, 2, 4, 5} <= used
    shrunk = [c for c in P.CASES if dict(c["knobs"]).get(4, 0) > 1 and P.form_of(c)[0] == "sg" and P.form_of(c)[3] == 1
              and mode_is_splittable(c) and P.form_of(c)[4] < dict(c["knobs"])[4]]
    assert shrunk, "no case forces more K-splits than sg_pick_ks keeps"
    # 48 columns = 3 panels: must fall back from two panels per wave where 32 columns take it
    assert any(c["N"] == 48 and dict(c["knobs"]).get(2) == 1 and P.form_of(c)[3] == 1 for c in P.CASES)
    assert any(c["N"] == 32 and dict(c["knobs"]).get(2) == 1 and P.form_of(c)[3] == 2 for c in P.CASES)
    # both sides of every row-tile edge
    assert {1, 16, 17, 32} <= {c["M"] for c in by_ep["plain"]} and {8, 9, 16, 17, 24} <= {c["M"] for c in by_ep["gateup_n8"]}
    for K in (32, 64, 96, 160, 224, 512, 544, 11008):
        assert any(c["K"] == K for c in by_ep["plain"]), K
    for ep in ("gateup_n8", "qkv_n8"):
        assert {1024, 1088, 5120} <= {c["K"] for c in by_ep[ep]}, ep


def mode_is_splittable(c):
    return P.mode_of(c) != P.SG_F32


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_rule_restatement_agrees_with_sg_rule_h(tmp_path):
    """pick_form / pick_ks / pick_n8 of tests/gemm_probes.py against sg_pick_form / sg_pick_ks / sg_pick_n8 (csrc/sg_rule.h,
    compiled with g++) on every case at its knobs, at the default knobs, and over a grid of shapes around the rule's edges."""
    exe = tmp_path / "test_gemm_probe_rule"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "test_gemm_probe_rule.cpp"),
                    "-o", str(exe)], check=True)
    rows = []
    for c in P.CASES:
        for kn in (P.knobs_of(c), dict(P.KNOB_DEFAULTS)):
            rows.append((P.mode_of(c), c["M"], c["N"], c["K"], kn))
    settings = [dict(P.KNOB_DEFAULTS)] + [{**P.KNOB_DEFAULTS, **dict(k)} for k in sorted({c["knobs"] for c in P.CASES})]
    for mode in range(5):
        for M in (1, 8, 9, 16, 17, 24, 25, 32):
            for N in (16, 32, 48, 3200, 8192 + 32, 16 * 4097):
                for K in (32, 480, 512, 544, 1024, 1056, 2048, 5120, 8192, 11008):
                    for kn in settings:
                        rows.append((mode, M, N, K, kn))
    text = "".join(f"{mode} {M} {N} {K} {kn[0]} {kn[2]} {kn[3]} {kn[4]} {kn[5]}\n" for mode, M, N, K, kn in rows)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) == len(rows) + 1
    for (mode, M, N, K, kn), line in zip(rows, out):
        MT, W, Pw = P.pick_form(mode, M, N, K, kn)
        mine = (MT, W, Pw, P.pick_ks(N // 16, Pw, K >> 5, W, mode, kn)) + P.pick_n8(mode, M, K)
        assert mine == tuple(int(v) for v in line.split()), (mode, M, N, K, kn, mine, line)


def test_delta_covers_a_float32_evaluation_of_silu():
    """DELTA = 32 x the largest relative deviation of a float32 evaluation of gf / (1 + exp(-gf)) from float64, over the
    probes' own gate values."""
    worst = 0.0
    for i, kind in ALL:
        c, mat, exps = built(i, kind)
        if P.streams_of(c) != 2:
            continue
        for e in exps:
            gf = e["y"][:, :c["N"]].float()
            s32, s64 = gf / (1.0 + torch.exp(-gf)), P.silu64(gf)
            ok = s64.abs() > 2.0 ** -24                                      # (below the fp16 range the quotient rounds to +-0 anyway)
            if bool(ok.any()):
                worst = max(worst, float(((s32.double() - s64).abs() / s64.abs())[ok].max()))
    print(f"float32 silu: largest relative deviation {worst:.3e}; DELTA = {P.DELTA:.3e} = {P.DELTA / worst:.1f} x")
    assert 32 * worst <= P.DELTA


@pytest.mark.parametrize("kind", P.KINDS)
def test_every_case_holds_its_conditions(kind):
    worst_unsafe, worst_y, worst_ss = 0.0, 0.0, 0.0
    for i in range(len(P.CASES)):
        c, mat, exps = built(i, kind)
        cid = (P.case_id(c), kind)
        M, N, K, S = c["M"], c["N"], c["K"], P.streams_of(c)
        step = P.step_of(c, kind)
        assert bool((mat["x"] != 0).all()) and bool(torch.isfinite(mat["x"]).all()), cid
        unsafe = total = 0
        for li, e in enumerate(exps):
            w = mat["ws"][li]
            assert bool((w != 0).any(dim=1).all()), cid                       # no zero row
            assert e["y_exact"], cid                                          # fp16(scale * acc) rounds nothing
            if c["ep"].endswith("_fp8"):                                      # every weight is an e4m3 value
                assert torch.equal(w.float().to(torch.float8_e4m3fn).float(), w.float()), cid
            if kind == "select":
                assert bool(((w != 0).sum(dim=1) == 1).all()), cid
                n = torch.arange(S * N)
                want = mat["h"][:, mat["ks"][li]] * w.double()[n, mat["ks"][li]][None, :]
                assert torch.equal(e["acc"], want), cid
            else:
                units = e["acc"].abs() / step
                units[:, :N] *= 32.0 if S == 2 else 1.0                       # (the gate stream's step is 2^-5 of the up stream's)
                assert torch.equal(units, units.round()) and float(units.max()) < 2048, (cid, float(units.max()))
                worst_y = max(worst_y, float(units.max()))
                # fp32 matmuls with K randomly permuted reproduce the float64 sums bit for bit
                perm = torch.randperm(K, generator=torch.Generator().manual_seed(i))
                a32 = mat["h"].float()[:, perm] @ w.float()[:, perm].t()
                assert torch.equal(a32.double(), e["acc"]), cid
                if "ss" in e and P.ss_exact(c, kind):
                    ssu = e["ss"] / step ** 2
                    assert float(ssu.max()) < 2 ** 24, (cid, float(ssu.max()))
                    worst_ss = max(worst_ss, float(ssu.max()))
            if "safe" in e:
                unsafe += int((~e["safe"]).sum())
                total += e["safe"].numel()
        # the ss_in hand-off: every 16-wide partial of x^2 and every sum of them is an integer below 2^24 in units of c_m^2
        if c.get("ss_in"):
            cm2 = P.c_of_rows(M).square()
            assert torch.equal(mat["ss_x"], (16 * cm2)[None, :].expand(K // 16, M)) and K < 2 ** 24, cid
        if total:
            assert unsafe <= P.UNSAFE_CAP * total, (cid, unsafe, total)
            worst_unsafe = max(worst_unsafe, unsafe / total)
    print(f"{kind}: max |y| / step {worst_y:.0f}, largest panel sum of squares {worst_ss:.3g} step^2, "
          f"largest unsafe share {100 * worst_unsafe:.2f} %")


def test_every_k_chunk_of_every_case_shows_in_the_dense_output():
    """A kernel that drops (or adds twice) ANY 32-wide k-chunk of any weight stream changes at least one K sum of the dense
    probe in every one of the stream's 16-column panels: the chunk's own partial sum — exact, so nothing can absorb it — is
    non-zero there."""
    for i in range(len(P.CASES)):
        c, mat, _ = built(i, "dense")
        M, K, NT = c["M"], c["K"], P.streams_of(c) * c["N"]
        part = torch.einsum("mck,nck->cmn", mat["h"].view(M, K // 32, 32), mat["ws"][0].double().view(NT, K // 32, 32))
        seen = (part != 0).view(K // 32, M, NT // 16, 16).any(dim=3).any(dim=1)             # (chunk, panel)
        assert bool(seen.all()), (P.case_id(c), seen.logical_not().nonzero()[:4].tolist())


def test_edge_set_is_selected_by_every_case():
    for i in range(len(P.CASES)):
        c, mat, _ = built(i, "select")
        E, N = set(P.edge_set(c["K"])), c["N"]
        assert {0, c["K"] - 1, 31, 32 * (c["K"] // 32 - 1)} <= E
        for s in range(P.streams_of(c)):
            hit = set()
            for kk in mat["ks"]:
                hit |= set(kk[s * N:(s + 1) * N].tolist())
            assert E <= hit, (P.case_id(c), s, sorted(E - hit)[:8])


@pytest.mark.parametrize("kind", P.KINDS)
def test_probes_are_exact_on_the_oracle_pipeline(kind):
    """The oracle's own fp16 / fp32 pipeline returns the float64 expectation bit for bit: rms_norm gives +-ln, linear the
    exact sums, silu_mul the expected product on every boundary-safe element (rope: expected() IS R.apply_rope of the exact
    q | k | v)."""
    for i in range(len(P.CASES)):
        c, mat, exps = built(i, kind)
        cid = (P.case_id(c), kind)
        N = c["N"]
        h = mat["x"] if mat["ln"] is None else R.rms_norm(mat["x"], mat["ln"], P.EPS)
        assert torch.equal(h.double(), mat["h"]), cid
        for li, e in enumerate(exps):
            w_eff = (mat["ws"][li].double() * mat["scale"][:, None]).half()
            assert torch.equal(w_eff.double(), mat["ws"][li].double() * mat["scale"][:, None]), cid
            y = R.linear(h, w_eff)
            assert torch.equal(y, e["y"]), cid
            if "safe" in e:
                got = R.silu_mul(y[:, :N], y[:, N:])
                assert torch.equal(got[e["safe"]], e["out"][e["safe"]]), cid
                assert bool(((got.double() - e["out"].double()).abs() <= e["tol"]).all()), cid
            if "ss" in e and c.get("resid"):
                assert torch.equal(e["out"], mat["res"] + e["y"]), cid           # the fp16 add of the oracle
