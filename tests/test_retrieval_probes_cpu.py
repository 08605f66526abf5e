"""The material, the conditions and the case list of the retrieval and row-move probes (tests/retrieval_probes.py), proved on
the CPU: the score material is exact (every code, mean and dot an fp16 value), every expectation is what the oracle
(oracle/ref_ops.py) and tests/cpu_backend.py compute, the top-k expectation is R.retrieval_topk on every case and torch.topk
up to ties wherever IEEE order and bit-pattern order agree, the Python restatement of the launch rules agrees with
csrc/retrieval_rule.h, the documented refusals return their codes, and the case list reaches every label of REQUIRED."""
import os
import shutil
import subprocess

import pytest
import torch

from oracle import ref_ops as R
from tests import cpu_backend as B
from tests import retrieval_probes as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_case_list_reaches_every_label():
    reached = P.all_labels()
    missing = sorted(P.REQUIRED - reached)
    assert not missing, missing
    # every edge of rt_topk_pick, by the restated rule
    pick = {s: P.topk_pick(*s) for s in P.TOPK_SHAPES}
    assert pick[(12033, 257)]["lds"] == 48 * 1024 and not pick[(12033, 257)]["raised"] and pick[(12034, 257)]["raised"]
    assert pick[(30209, 8193)] == dict(form="select", lds=150 * 1024, mpow2=8192, npow2=0, raised=True)
    assert pick[(30210, 8193)]["form"] == "full" and pick[(30210, 8193)]["lds"] == 128 * 1024
    assert pick[(32768, 4097)]["form"] == "select" and pick[(32768, 4098)]["form"] == "full"
    for s in ((8200, 8195), (16385, 8194)):
        assert pick[s]["form"] == "full" and pick[s]["lds"] == 64 * 1024 and not pick[s]["raised"], s
    for s in ((16386, 8194), (20000, 10000), (32768, 32768)):
        assert pick[s]["form"] == "full" and pick[s]["lds"] == 128 * 1024 and pick[s]["raised"], s
    for s in ((2, 1), (2, 2), (9, 1), (9, 2), (9, 3), (9, 9)):
        assert pick[s]["form"] == "select" and not pick[s]["raised"], s
    # the raised attribute is per process: within each form every un-raised shape is launched before the first raised one
    for form in ("select", "full"):
        raised = [pick[s]["raised"] for s in P.TOPK_SHAPES if pick[s]["form"] == form]
        assert raised == sorted(raised) and False in raised and True in raised, (form, raised)
    # kv_copy_rows: both sides of the 64-workgroup cap at D = 128
    assert P.copy_grid_x(1024, 128) == 64 == P.copy_grid_x(1025, 128) and 1025 * 16 > 64 * 256 >= 1024 * 16
    # the stride cases: cap 8, and C = step j + {-1, 0, 1} for j in {1, 2, 4}, 4.5 steps and 1029
    for D in (64, 128):
        step = 8 * P.gpb_of(D)
        assert P.chunk_grid_x(10 ** 6, P.STRIDE_H, D) == 8
        want = {step * j + o for j in (1, 2, 4) for o in (-1, 0, 1)} | {4 * step + step // 2, 1029}
        assert {c["C"] for c in P.SCORE_CASES if c["H"] == P.STRIDE_H and c["D"] == D} == want
    assert {c["layout"] for c in P.SCORE_CASES} == {"head", "token", "pad"}
    assert {(c["chunk"], c["D"]) for c in P.GATHER_CASES} == set(P.GATHER_SHAPES)
    assert {P.rows_per_blk(D) for D in P.SHIFT_DS} == {32, 21, 16, 8, 1}
    for i in range(len(P.TOPK_SHAPES)):
        for bits in P.topk_case(i)["bits"]:
            assert not any(b > 0xFC00 for b in bits), P.topk_id(i)                 # -NaN is in no row


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_rule_restatement_agrees_with_retrieval_rule_h(tmp_path):
    """topk_pick / chunk_grid_x / copy_grid_x of tests/retrieval_probes.py against rt_topk_pick / rt_chunk_grid_x /
    rt_copy_grid_x (csrc/retrieval_rule.h, compiled with g++) on every case and over a grid around every edge of the rules."""
    exe = tmp_path / "test_retrieval_rule"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "test_retrieval_rule.cpp"),
                    "-o", str(exe)], check=True)
    queries = [("t",) + s for s in P.TOPK_SHAPES]
    for C in (2, 3, 9, 4097, 8193, 8194, 12032, 12033, 12034, 16384, 16385, 16386, 30208, 30209, 30210, 32767, 32768):
        for sets in (1, 2, 3, 4, 5, 257, 258, 4097, 4098, 8193, 8194, C - 1, C):
            if 1 <= sets <= C:
                queries.append(("t", C, sets))
    for c in P.SCORE_CASES:
        queries.append(("g", c["C"], c["H"], c["D"]))
        queries += [("g", c1 - c0, c["H"], c["D"]) for c0, c1 in P.pieces_of(c)]
    for n in (0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 1023, 1024, 1025, 15616, 10 ** 6):
        for H in (1, 2, 3, 5, 32, 40, 255, 256, 257, 2048, 2049, 4096):
            queries += [("g", n, H, 64), ("g", n, H, 128)]
    for c in P.COPY_CASES:
        queries.append(("c", c["n"], c["D"]))
    for n in (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 10 ** 5):
        for D in (8, 64, 96, 128, 256, 2048):
            queries.append(("c", n, D))
    text = "".join(" ".join(str(v) for v in q) + "\n" for q in queries)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) == len(queries) + 1
    for q, line in zip(queries, out):
        got = tuple(int(v) for v in line.split())
        if q[0] == "t":
            p = P.topk_pick(q[1], q[2])
            mine = (0 if p["form"] == "select" else 1, p["lds"], p["mpow2"], p["npow2"], int(p["raised"]))
        elif q[0] == "g":
            mine = (P.chunk_grid_x(*q[1:]),)
        else:
            mine = (P.copy_grid_x(*q[1:]),)
        assert mine == got, (q, mine, line)


# ---- scores -------------------------------------------------------------------------------------------------------------------------
def _neighbours_differ(codes, step):
    H, C = codes.shape
    ok = True
    for dc in (1, step):
        if dc < C:
            ok &= bool((codes[:, dc:] != codes[:, :-dc]).all())
    if H > 1:
        ok &= bool((codes[1:] != codes[:-1]).all())
    return ok


@pytest.mark.parametrize("kind", P.SCORE_KINDS)
def test_score_material_is_exact_and_is_what_the_oracle_computes(kind):
    seen_d = {64: set(), 128: set()}
    for c in P.SCORE_CASES:
        cid = (P.score_id(c), kind)
        H, D, C, chunk = c["H"], c["D"], c["C"], c["chunk"]
        mat = P.score_material(c, kind)
        k, q = mat["k"], mat["q"]
        assert chunk in (1, 2, 8, 16) and k.shape == (H, C * chunk, D) and bool(torch.isfinite(k).all()), cid
        assert torch.equal(mat["want"].double(), mat["want64"]) and torch.equal(mat["index"].double(), mat["index64"]), cid
        if kind == "onehot":
            codes = mat["codes"]
            assert int(codes.abs().min()) >= 1 and int(codes.abs().max()) <= 2048, cid
            assert _neighbours_differ(codes, P.score_step(c)), cid
            assert bool(((q != 0).sum(dim=1) == 1).all()) and bool((k != 0).all()), cid
            hs = torch.arange(H)
            assert bool((q[hs, mat["d"]] != 0).all()), cid
            col = k[hs[:, None], torch.arange(C * chunk)[None, :], mat["d"][:, None]].view(H, C, chunk)     # a chunk's rows share its code
            assert torch.equal(col.double(), codes.double()[:, :, None].expand(-1, -1, chunk)), cid
            lg = torch.log2(q[hs, mat["d"]].abs().double())
            assert torch.equal(lg, lg.round()), cid                             # q_val = +- 2^j
            seen_d[D] |= set(mat["d"].tolist())
        else:
            assert bool(((q == 0) | (q.abs() == 1)).all()) and int((q != 0).sum(dim=1).max()) <= 16, cid
            assert torch.equal(k, k.round()) and float(k.abs().max()) <= 8, cid
            units = mat["want64"] * chunk
            assert torch.equal(units, units.round()) and float(units.abs().max()) <= 2048, cid
            iu = mat["index64"] * chunk
            assert torch.equal(iu, iu.round()), cid
        view, _ = P.place(k, c["layout"])
        assert torch.equal(view, k), cid
        assert torch.equal(B.retrieval_score(view, q, C, chunk), mat["want"]), cid
        assert torch.equal(R.retrieval_chunk_means(view.permute(1, 0, 2), C * chunk, chunk).permute(1, 0, 2), mat["index"]), cid
    if kind == "onehot":
        assert seen_d[64] == set(range(64)) and seen_d[128] == set(range(128))   # d_h walks every position


def test_pieces_are_off_the_group_grid():
    for c in P.SCORE_CASES:
        (z, a), (a2, b), (b2, C) = P.pieces_of(c)
        assert z == 0 and a == a2 and b == b2 and C == c["C"] and 0 <= a <= b <= C
        g = P.gpb_of(c["D"])
        if C > 2 * g:
            assert a % g and b % g, P.score_id(c)


# ---- top-k ---------------------------------------------------------------------------------------------------------------------------
def test_topk_expectation_is_the_oracle_and_torch_topk_up_to_ties():
    clean = 0
    for i in range(len(P.TOPK_SHAPES)):
        t = P.topk_case(i)
        C, sets, scores = t["C"], t["sets"], t["scores"]
        want = torch.tensor(t["want"])
        assert want.shape == (P.TOPK_H, sets), P.topk_id(i)
        assert torch.equal(want, R.retrieval_topk(scores, sets)), P.topk_id(i)
        assert torch.equal(want, B.retrieval_topk(scores, sets).long()), P.topk_id(i)
        for h, row in enumerate(t["want"]):
            assert row[0] == 0 and len(set(row)) == sets and all(0 <= x < C for x in row) and 0 not in row[1:], (P.topk_id(i), h)
            if sets > 1 and P.topk_row_is_ieee_clean(t["bits"][h]):
                s = scores[h:h + 1]
                theirs = torch.cat([torch.zeros(1, 1, dtype=torch.int64), torch.topk(s[:, 1:].float(), sets - 1).indices + 1], dim=1)
                assert R.topk_matches_reference(s, want[h:h + 1], theirs), (P.topk_id(i), h, t["kinds"][h])
                clean += 1
    assert clean >= 20


def test_topk_planted_rows_put_the_mth_key_where_they_say():
    def key(bits, c):
        o = P.order_of_bits(bits[c])
        return ((o + 0x8000) << 16) | (65535 - c)                              # the kernel's key, from the order alone
    seen = set()
    for i in range(len(P.TOPK_SHAPES)):
        t = P.topk_case(i)
        m = t["sets"] - 1
        for h, kind in enumerate(t["kinds"]):
            if m < 1:
                continue
            bits, cm = t["bits"][h], t["want"][h][m]
            k = key(bits, cm)
            same = [c for c in range(1, t["C"]) if bits[c] == bits[cm]]
            if kind == "chunk255":
                assert cm % 256 == 255 and k & 255 == 0 and len(same) > 1
            elif kind == "chunk0":
                assert cm % 256 == 0 and k & 255 == 255 and len(same) > 1
            elif kind == "lo00":
                assert (k >> 16) & 255 == 0
            elif kind == "loFF":
                assert (k >> 16) & 255 == 255
            elif kind == "hi00":
                assert bits[cm] >> 8 == 0
            elif kind == "hiFF":
                assert k >> 24 == 255
            elif kind == "all_equal":
                assert len(same) == t["C"] - 1
            elif kind == "tie_inside":
                assert bits[t["want"][h][m - 1]] == bits[cm] and same.index(cm) + 1 < len(same)
            elif kind == "tie_first":
                assert same[0] == cm and (m == 1 or bits[t["want"][h][m - 1]] != bits[cm])
            elif kind == "tie_last":
                assert same[-1] == cm
            elif kind == "sweep":
                assert set(P._sweep_values()) <= set(bits[1:]) and {0x0000, 0x8000, 0x7C00, 0xFC00, 0x0001, 0x8001} <= set(bits[1:])
            elif kind == "one_nan":
                assert bits[1:].count(P.POS_NAN) == 1 and t["want"][h][1] == bits.index(P.POS_NAN)
            seen.add(kind)
    assert set(P.TOPK_KINDS) <= seen


def test_a_zero_pair_is_ordered_by_sign_not_tied():
    bits = [0x7C00, 0x8000, 0x0000, 0x8000, 0x0000, 0xBC00]                    # chunks 2 and 4 (+0) before 1 and 3 (-0)
    assert P.topk_expected(bits, 5) == [0, 2, 4, 1, 3]
    s = torch.tensor(bits, dtype=torch.int32).to(torch.int16).view(torch.float16)[None]
    assert R.retrieval_topk(s, 5).tolist() == [[0, 2, 4, 1, 3]]


# ---- gathers and row moves ----------------------------------------------------------------------------------------------------------
def test_address_codes_name_their_rows():
    x = P.coded(1, (2, 3, 2100, 128))
    assert torch.equal(x, x.round()) and float(x.abs().max()) <= 2046 and not bool((x == P.SENTINEL).any())
    assert float(torch.tensor(P.SENTINEL, dtype=torch.float16)) == P.SENTINEL and P.SENTINEL != round(P.SENTINEL)
    rows = x[0, 0]
    assert torch.unique(rows, dim=0).shape[0] == rows.shape[0]                 # no two rows of a head are equal
    assert not torch.equal(P.coded(1, (3, 40, 64)), P.coded(2, (3, 40, 64)))


def test_gather_expectation_is_the_oracle():
    from triforce_amd import ops
    idx = P.gather_idx()
    for h in range(P.GATHER_H):
        row = idx[h].tolist()
        assert 0 in row and P.GATHER_C - 1 in row and len(set(row)) < len(row)
        assert any(row[j] - 1 == row[j + 1] and row[j + 1] - 1 == row[j + 2] for j in range(len(row) - 2))     # a descending run
    for c in P.GATHER_CASES:
        mat = P.gather_material(c)
        chunk = c["chunk"]
        n = idx.shape[1] * chunk
        for src, want in ((mat["k"], mat["want_k"]), (mat["v"], mat["want_v"])):
            view, _ = P.place(src, c["src"])
            assert torch.equal(R.retrieval_gather(view.permute(1, 0, 2), idx.long(), chunk).permute(1, 0, 2), want), P.gather_id(c)
        kd = torch.full((P.GATHER_H, n + P.GATHER_GUARD, c["D"]), P.SENTINEL, dtype=torch.float16)
        vd = kd.clone()
        B.retrieval_gather(mat["k"], mat["v"], idx, kd, vd, chunk)
        assert torch.equal(kd[:, :n], mat["want_k"]) and torch.equal(vd[:, :n], mat["want_v"]) and bool((kd[:, n:] == P.SENTINEL).all())
        assert not torch.equal(mat["k"], mat["v"])
        if c["D"] == 128:
            kc, vc, ke, ve = ops.retrieval_gather_fp8_ref(mat["k"], mat["v"], idx, chunk)
            wk, wke, _ = ops.kv_quantize_ref(mat["want_k"])
            wv, wve, _ = ops.kv_quantize_ref(mat["want_v"])
            assert torch.equal(kc.view(torch.uint8), wk.view(torch.uint8)) and torch.equal(ke, wke)
            assert torch.equal(vc.view(torch.uint8), wv.view(torch.uint8)) and torch.equal(ve, wve)
            assert len(set(wke.flatten().tolist())) > 1                         # more than one row exponent in play


def test_row_move_expectations_are_the_cpu_backend():
    for c in P.COPY_CASES:
        mat = P.copy_material(c)
        for src in (mat["src_k"], mat["src_v"]):
            dst = torch.full((c["L"], c["H"], mat["Td"], c["D"]), P.SENTINEL, dtype=torch.float16)
            B.kv_copy_rows(src, dst, c["src_t0"], c["dst_t0"], c["n"])
            assert torch.equal(dst, P.copy_expected(c, src)), P.copy_id(c)
    for D in P.SHIFT_DS:
        for c in P.shift_cases(D):
            k, v, wk, wv = P.shift_material(c)
            kk, vv = k.clone(), v.clone()
            B.kv_shift_rows_pair(kk, vv, P.SHIFT_DST_T0 + c["shift"], P.SHIFT_DST_T0, c["n"])
            assert torch.equal(kk, wk) and torch.equal(vv, wv), c
            assert not torch.equal(k, wk)
    for c in P.ROWS_CASES:
        assert all(a < b for a, b in zip(c["idx"], c["idx"][1:])) and P.ROWS_OFFSET + max(c["idx"]) < c["T"], P.rows_id(c)
        k, v, wk, wv = P.rows_material(c)
        kk, vv = k.clone(), v.clone()
        B.kv_gather_rows(kk, vv, P.ROWS_OFFSET, torch.tensor(c["idx"], dtype=torch.int32))
        assert torch.equal(kk, wk) and torch.equal(vv, wv), P.rows_id(c)
        if c["name"] == "largest":
            assert P.ROWS_OFFSET + c["idx"][-1] == c["T"] - 1


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_documented_refusals_return_their_codes():
    """Every refused call returns before anything launches, so no device is needed: the pointers are never read."""
    from triforce_amd import hip
    lib = hip.lib()
    for entry, over, code in P.REFUSALS:
        assert set(over) <= set(P.REFUSAL_OK[entry]), (entry, over)
        assert P.refusal_call(lib, entry, over, 4096, 8192) == code, (entry, over)
    assert {e for e, _, _ in P.REFUSALS} == set(P.REFUSAL_ORDER)
    for entry, (name, order) in P.REFUSAL_ORDER.items():
        assert set(order) == set(P.REFUSAL_OK[entry]), entry
        assert len(hip.SIGNATURES[name][1]) == len(order) + 1, name            # + the stream
    elems = {"h": P.REFUSAL_BUFFERS["h"][1], "i": P.REFUSAL_BUFFERS["i"][1]}
    for entry, a in P.REFUSAL_OK.items():                                      # the accepted baseline stays inside the buffers
        if "sh" in a:
            assert a["H"] * a["sh"] <= elems["h"]
