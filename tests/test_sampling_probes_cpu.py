"""Proves the sampling probes (tests/sampling_probes.py) without a GPU: the material is dyadic and its sums exact, every
u * total and every accept ratio is exact in fp32, every int64 expectation equals the oracle (oracle/ref_ops.py,
oracle/ref_tree.py) and the host forms of triforce_amd.ops, and the case list reaches every entry point, every (instance,
data path) pair of block_sample and every member of the edge set.  The oracle is the reference: no kernel is run here."""
import os
import shutil
import subprocess
from fractions import Fraction

import pytest
import torch

from oracle import ref_model as M
from oracle import ref_ops as R
from oracle import ref_tree as RT
from tests import sampling_probes as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    from triforce_amd import ops
    return ops


def _dyadic(w):
    f = P.f32(w)
    assert torch.equal(f.double(), w.double() * 2.0 ** -P.UNIT_LOG2)
    return f


def _sums_exact(w, f, g):
    """fp32 sums of the row under a random permutation and under cumsum are the integer sums."""
    perm = torch.randperm(f.numel(), generator=g)
    acc = torch.zeros((), dtype=torch.float32)
    nzp = f[perm]
    nzp = nzp[nzp != 0]                                   # (adding an exact zero changes nothing: keep the loop short)
    for x in nzp:
        acc = acc + x
    assert float(acc) * 2.0 ** P.UNIT_LOG2 == float(w.sum())
    assert torch.equal(torch.cumsum(f, 0).double() * 2.0 ** P.UNIT_LOG2, torch.cumsum(w, 0).double())


# ---- the slice rule and the coverage of block_sample -----------------------------------------------------------------------
def test_seg_rule_matches_the_kernels_comment():
    """csrc/sampling.hip: thread t owns [t * seg, (t + 1) * seg), seg a multiple of 4, <= 32 for V <= 32768, 33 - 256 above
    (the rule lives inside the kernel source, not in a header a host program could include)."""
    for V in list(P.SAMPLE_VOCABS) + list(range(1, 5000, 7)) + [32767, 32769, 65536, 65537, 200000, 262143]:
        seg = P.seg_of(V)
        assert seg % 4 == 0 and seg * 1024 >= V and (seg - 4) * 1024 < V
        assert (seg <= 32) == (V <= 32768) and (V <= 32768 or 33 <= seg <= 256)
    assert [P.seg_of(V) for V in (1024, 4100, 32000, 32768, 32772, 40000, 128256, 262144)] == [4, 8, 32, 32, 36, 40, 128, 256]


SEG_LINE = "const int seg = (((V + SAMP_THREADS - 1) / SAMP_THREADS) + 3) & ~3;"
LARGE_LINE = "(V) > SAMP_THREADS * 32"


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_seg_rule_agrees_with_the_kernels_expression(tmp_path):
    """seg_of / path_of's instance rule against the kernel's own two expressions, compiled with g++ from
    tests/native/test_sampling_seg_rule.cpp (nothing from the GPU is included); csrc/sampling.hip must still hold both lines."""
    kernel = open(os.path.join(ROOT, "triforce_amd", "csrc", "sampling.hip")).read()
    native = os.path.join(ROOT, "tests", "native", "test_sampling_seg_rule.cpp")
    for line in (SEG_LINE, LARGE_LINE, "#define SAMP_THREADS 1024"):
        assert line in kernel and line in open(native).read()
    exe = tmp_path / "test_sampling_seg_rule"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", native, "-o", str(exe)], check=True)
    Vs = sorted(set(P.SAMPLE_VOCABS) | set(range(1, 6000, 13)) | {32767, 32769, 65536, 65537, 200000, 262143} |
                {c["V"] for c in P.chain_cases()} | set(P.MID_VOCABS))
    out = subprocess.run([str(exe)], input="".join(f"{V}\n" for V in Vs), capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == 2 * len(Vs)
    for i, V in enumerate(Vs):
        assert (int(out[2 * i]), bool(int(out[2 * i + 1]))) == (P.seg_of(V), P.path_of(V, True) == "stream" or P.path_of(V, True).startswith("elem_large")), V


def test_case_list_reaches_every_path_and_edge():
    paths = {P.path_of(V, a) for V in P.SAMPLE_VOCABS for a in P.alignments(V)}
    assert paths == P.ALL_PATHS
    assert P.path_of(32770, True) == "elem_large_mod4" and P.path_of(32772, False) == "elem_large_misaligned"
    assert P.path_of(32772, True) == "stream" and P.path_of(1023, True) == "elem_small" and P.path_of(32768, True) == "reg4"
    assert 47 in P.edge_set(40000) and 40 in P.edge_set(40000) and {15, 16} <= set(P.edge_set(32772))
    for V in P.SAMPLE_VOCABS:
        rows = P.sample_rows(V)
        for e in P.edge_set(V):
            mine = [r for r in rows if r["e"] == e]
            assert sorted(r["W"] for r in mine) == sorted(P.TOTALS)
            for r in mine:
                w, _ = P.dense_row(r)
                assert w[e] > 0
                for nb in (e - 1, e + 1):                              # neighbours are zero bins where there is room
                    if 0 <= nb < V and V > 3 and nb not in (0, V - 1):
                        assert w[nb] == 0 or nb in r["idx"] and (e <= 2 or e >= V - 3)
                if V > 3 and e not in (0, V - 1) and 0 not in r["idx"][:1]:
                    assert w[0] == 0
                us = dict(r["probes"])
                assert us[r["lo"]] == e                                  # the lower edge exactly
                if r["lo"] > 0:
                    assert us[r["lo"] - 1] == r["idx"][0] != e           # one step below: the previous non-zero token
                if r["hi"] < P.U_ONE:
                    assert us[r["hi"]] == r["idx"][-1] != e              # the upper edge exactly: the next non-zero token
                if r["hi"] - 1 in us:
                    assert us[r["hi"] - 1] == e
                assert us[0] == r["idx"][0] and us[P.U_ONE] == r["idx"][-1]
    for name in P.ENTRY_POINTS:
        assert hasattr(_ops(), name) and len(P.entry_cases(name)) > 0


def test_dropped_pairs_are_the_documented_ones():
    n = 0
    for V in P.SAMPLE_VOCABS:
        for r in P.sample_rows(V):
            for U, _ in r["probes"]:
                assert P.product_exact(U, r["W"])
            assert r["dropped"] in ([], [P.U_ONE - 1]) and (not r["dropped"] or r["W"] == 3 * P.ONE // 4)
            n += len(r["dropped"])
    assert n == sum(len(P.edge_set(V)) for V in P.SAMPLE_VOCABS)


# ---- sample_inverse_cdf ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", P.SAMPLE_VOCABS)
def test_sample_rows_against_oracle_and_host(V):
    ops = _ops()
    g = torch.Generator().manual_seed(V)
    for r in P.sample_rows(V):
        w, f = P.dense_row(r)
        _dyadic(w)
        _sums_exact(w, f, g)
        for U, want in r["probes"]:
            u = P.u_f32(U)
            assert P.expect_token(w, U, r["W"]) == want
            assert R.sample_inverse_cdf(f, u) == want, (V, r["e"], r["W"], U)
            assert ops._invcdf_host(f, torch.tensor(u, dtype=torch.float32)) == want, (V, r["e"], r["W"], U)


def test_massless_row_is_token_zero():
    """The rule of include/triforce_hip.h: a row with no mass gives token 0; u = 1.0 the last index with non-zero mass."""
    z = torch.zeros(37)
    assert R.sample_inverse_cdf(z, 0.0) == 0 and R.sample_inverse_cdf(z, 1.0) == 0
    assert _ops()._invcdf_host(z, torch.tensor(0.5)) == 0
    _, f = P.row(37, [3, 9], [P.ONE // 2, P.ONE // 2])
    assert R.sample_inverse_cdf(f, 1.0) == 9 and _ops()._invcdf_host(f, torch.tensor(1.0)) == 9


# ---- the accept chain ------------------------------------------------------------------------------------------------------
def test_chain_cases_against_oracle():
    g = torch.Generator().manual_seed(1)
    bases, seen = {}, set()
    for c in P.chain_cases():
        key = (c["g2"], c["V"])
        if key not in bases:
            bases[key] = P.chain_base(*key)
            p0, q0, _ = bases[key]
            for i in range(c["g2"]):                                   # the decoys: disjoint blocks, row by row
                sup = set((p0[i] + q0[i]).nonzero().flatten().tolist())
                for j in range(i + 1, c["g2"] + 1):
                    other = p0[j] + (q0[j] if j < c["g2"] else 0)
                    assert not sup & set(other.nonzero().flatten().tolist())
            assert p0[:, 0].sum() == 0 and p0[:, -1].sum() == 0
        p0, q0, tokens = bases[key]
        p, q = P.chain_apply(c, p0, q0)
        rec, U, draw = P.chain_expect(c, p, q, tokens)
        pf, qf = _dyadic(p), _dyadic(q)
        assert int(p.sum(1).max()) <= 2 * P.ONE and int(q.sum(1).max()) <= 2 * P.ONE
        for i, t in enumerate(tokens):                                 # every ratio is exact in fp32
            ratio = P._ratio(int(p[i, t]), int(q[i, t]))
            got = pf[i, t] / qf[i, t]
            if isinstance(ratio, Fraction):
                assert Fraction(float(got)) == ratio
            else:
                assert bool(torch.isnan(got)) if ratio is None else bool(torch.isinf(got))
        if draw is not None:
            w, Ud, W = draw
            assert P.product_exact(Ud, W) and (W & (W - 1) == 0 or Ud in (0, P.U_ONE))
            if key not in seen:
                _sums_exact(w, P.f32(w), g)
            if rec[2] == 0:                                            # |p - q| and p alone would give another token
                res = (p[rec[0]] - q[rec[0]]).clamp(min=0)
                if not c["draw_below"]:                               # (the draw ON the edge tells them apart)
                    assert P.expect_token((p[rec[0]] - q[rec[0]]).abs(), Ud) != rec[1] != P.expect_token(p[rec[0]], Ud)
                assert torch.equal(res, w)
                if W & (W - 1) == 0:                                   # q's excess sits in front of the positive part
                    assert (q[rec[0]] > p[rec[0]]).nonzero()[0] < w.nonzero()[0]
        seen.add(key)
        got = R.accept_and_correct(pf, qf, tokens, [P.u_f32(x) for x in U], c["inclusive"], c["eos"])
        assert tuple(got) == rec, (c["what"], key, c["inclusive"], got, rec)
    whats = {c["what"] for c in P.chain_cases()}
    for what in ("inf at 0", "nan at 0", "eos at the last position", "eos accepted before the last", "eos behind the reject",
                 "eos at the rejected position"):
        assert what in whats


def test_chain_boundary_triple_flips_with_inclusive():
    """u = r: accepted when inclusive, rejected when not; one step below: both accept; one step above: both reject."""
    bases = {}
    for c in P.chain_cases():
        if not c["what"].startswith("r="):
            continue
        key = (c["g2"], c["V"])
        if key not in bases:
            bases[key] = P.chain_base(*key)
        p0, q0, tokens = bases[key]
        p, q = P.chain_apply(c, p0, q0)
        rec, _, _ = P.chain_expect(c, p, q, tokens)
        pos = next(iter(c["u"]))
        du = int(c["what"].rsplit("du=", 1)[1])
        accepted = rec[0] > pos
        assert accepted == (du < 0 or (du == 0 and c["inclusive"])), c["what"]


# ---- Middle_Spec -----------------------------------------------------------------------------------------------------------
def _mid_setup(c):
    p = P.mid_base(c["V"])
    qs = [P.mid_q(c["V"], c["n"] + 2 * s) for s in range(c["depth"])]
    U = [P.NAN if x is None else P.u_f32(x) for x in P.mid_uniforms(c)]
    return p, qs, U


def test_mid_cases_against_oracle_and_host_forms():
    ops = _ops()
    pfs = {V: _dyadic(P.mid_base(V)) for V in P.MID_VOCABS}
    for V in P.MID_VOCABS:
        assert torch.equal(P.mid_base(V).sum(1), torch.full((P.GAMMA + 1,), P.ONE))
        assert P.product_exact(28 * P.U_ONE // 64, P.ONE) and P.product_exact(28 * P.U_ONE // 64 - 1, P.ONE)
    ran = set()
    for c in P.mid_cases():
        p, qs, U = _mid_setup(c)
        pf, qfs = pfs[c["V"]], [_dyadic(q) for q in qs]
        stages, tok_after, adv = P.mid_expect(c, p)
        ran.add((c["depth"], len(stages)))
        tok0 = P.mid_tokens(c)
        for s, (acc, b, d) in enumerate(stages):                       # the oracle, stage by stage
            pos = c["n"] + 2 * s
            assert Fraction(float(pf[pos, d] / qfs[s][d])) == P.MID_RATIO
            assert R.middle_accept(pf, qfs[s], d, pos, U[3 * s + 1:3 * s + 3]) == (acc, b)
        for at in (0, 5):
            ubuf = torch.tensor([P.NAN] * at + U + [P.NAN] * 3, dtype=torch.float32)
            tok, cur = torch.tensor(tok0), torch.tensor([at])
            out = torch.full((ops.mid_record_len(c["depth"]) + 1,), -7, dtype=torch.int64)
            ops.middle_accept_n_host(pf, qfs, tok, ubuf, cur, c["n"], P.GAMMA, out, c["depth"])
            assert out.tolist() == P.mid_record(stages, at, c["depth"]) + [-7]
            assert tok.tolist() == tok_after and int(cur) == at + adv
            if c["depth"] == 1:
                tok, cur = torch.tensor(tok0), torch.tensor([at])
                out = torch.full((5,), -7, dtype=torch.int64)
                ops.middle_accept_host(pf, qfs[0], tok, ubuf, cur, c["n"], P.GAMMA, out)
                assert out.tolist() == list(stages[0]) + [at, -7] and tok.tolist() == tok_after and int(cur) == at + 3
    assert ran == {(d, k) for d in (1, 2, 3, 4) for k in range(1, d + 1)}   # every depth stops at every stage and runs through


# ---- the tree walk ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", P.TREE_VOCABS)
def test_tree_cases_against_model_and_oracle(V):
    cases = P.tree_cases(V)
    assert {c["kind"] for c in cases} == {"A-reject", "A-accept", "B-accept", "B0-reject"}
    assert {c["tokens"][1] for c in cases} >= {0, 1, 2, 31, 32, V - 1}
    for c in cases:
        assert P.tree_model(c) == c["want"], (c["kind"], c["tokens"])
        p, draft, tokens, u = P.tree_tensors(c)
        pf = _dyadic(p)
        q = torch.softmax(draft[0] / P.TREE_T, dim=-1)
        assert torch.equal(q[c["sup"]], torch.full((P.TREE_K,), 1.0 / P.TREE_K)) and float(q.sum()) == 1.0
        gm = RT.grow_map_from_branches(c["branches"])
        rng = M.InjectedRng(u.tolist())
        acc, nxt, terminal, _ = RT.accept_walk(pf, draft, tokens, gm["Successors"], P.TREE_T, rng)
        want = c["want"]
        assert (acc, int(terminal), rng.i) == (want["acc"], want["terminal"], want["consumed"]), (c["kind"], c["tokens"])
        assert terminal or nxt == want["next"], (c["kind"], c["tokens"], nxt, want)
        edges = {32 * t - d for t in range(1, 1025) for d in (0, 1)} | {V - 1}
        assert any(t in edges for r in c["rows"] for t in r)


# ---- the race --------------------------------------------------------------------------------------------------------------
def test_race_cases():
    cases = P.race_cases()
    assert {(c["V"], c["k"]) for c in cases} == set(P.RACE_SHAPES) and {c["rows"] for c in cases} == {1, 5}
    for V, _ in P.RACE_SHAPES:
        hit = {x for c in cases if c["V"] == V for o in c["ones"] for x in o}
        assert set(P.race_edges(V)) <= hit
    assert any(c["dead"][0] is not None for c in cases) and any(len(c["ones"][0]) == c["k"] + 3 for c in cases)
    for c in cases:
        logits, rand = P.race_tensors(c)
        assert bool(torch.isfinite(logits).all()) == (c["dead"][0] is None)
        for r in range(c["rows"]):
            assert c["want"][r] == sorted(c["ones"][r])[:c["k"]] and c["dead"][r] not in c["ones"][r]
        if c["rows"] == 5:
            assert len({tuple(o) for o in c["ones"]}) > 1 or c["V"] == 16
        if c["dead"][0] is None and len(c["ones"][0]) == c["k"]:        # exactly k ones: the oracle's winners, as a set
            got = RT.sample_without_replacement(logits, rand, c["k"], P.RACE_T).view(c["rows"], c["k"])
            for r in range(c["rows"]):
                assert set(got[r].tolist()) == set(c["want"][r])
