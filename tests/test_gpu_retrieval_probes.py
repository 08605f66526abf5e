"""The retrieval build and the KV row moves (csrc/retrieval.hip) on the exact material of tests/retrieval_probes.py: every
score, every chunk id and every moved row must come back BIT FOR BIT (torch.equal / ==) at every kernel path the launch
rules of csrc/retrieval_rule.h can take.  No tolerance anywhere; no expectation comes from a kernel.

Every destination is pre-filled with a sentinel and has guard rows, and is compared WHOLE (its base buffer, padding and
guards included) with the expected buffer, so a store outside the rows a call owns shows.  Each test records the
(kernel, path) labels of the cases it ran; test_zz_every_form_was_run fails on a label nothing ran.

The raised-LDS attribute of the two top-k kernels is set once per process, so a launch labelled "plain" runs un-raised only
when no raised launch of the same kernel came first.  P.TOPK_SHAPES is in launch order with every un-raised shape of a form
before the first raised one (asserted in tests/test_retrieval_probes_cpu.py), and nothing but this file launches the full
sort: its 64 KiB cases run un-raised whenever the file runs in that order.  The select kernel's un-raised cases do so when
this file runs alone; in the whole suite a full-size select launch of an earlier file has raised it, and they run anyway.
"""
import pytest
import torch

from tests import retrieval_probes as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RAN = set()
CODE_SENTINEL, EXP_SENTINEL = 0x5A, 0xA5


def _ops():
    from triforce_amd import ops
    return ops


def sentinel(*shape):
    return torch.full(shape, P.SENTINEL, dtype=torch.float16)


def first_diff(got, want):
    bad = (got != want).nonzero()
    return None if bad.numel() == 0 else tuple(int(v) for v in bad[0])


def same(got, want, what):
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        at = first_diff(got, want)
        raise AssertionError(f"{what}: first difference at {at}: got {got[at].item()!r}, expected {want[at].item()!r}")


# ---- scores -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.SCORE_CASES, ids=[P.score_id(c) for c in P.SCORE_CASES])
def test_score_probe(c):
    ops = _ops()
    H, D, C, chunk = c["H"], c["D"], c["C"], c["chunk"]
    for kind in P.SCORE_KINDS:
        cid = f"{P.score_id(c)} [{kind}]"
        mat = P.score_material(c, kind)
        k, base = P.place(mat["k"], c["layout"], DEV)
        q = mat["q"].to(DEV)
        if c["layout"] == "token":
            assert k.stride(1) == H * D and k.stride(0) == D
        if c["layout"] == "pad":
            assert k.stride(1) == D and k.stride(0) == (C * chunk + 8) * D
        # 1. the one-pass scorer
        one_pass = ops.retrieval_score(k, q, C, chunk)
        # 2. the index built whole, then scored
        whole = sentinel(H, C + 3, D).to(DEV)
        ops.chunk_mean(k, whole, 0, C, chunk)
        via_index = ops.retrieval_score_indexed(whole, q, C)
        # 3. the index built in pieces; after each piece every chunk not yet written still holds the sentinel
        parts = sentinel(H, C + 3, D).to(DEV)
        want_parts = sentinel(H, C + 3, D)
        for c0, c1 in P.pieces_of(c):
            ops.chunk_mean(k, parts, c0, c1, chunk)
            want_parts[:, c0:c1] = mat["index"][:, c0:c1]
            same(parts, want_parts, f"{cid}: index after piece [{c0}, {c1})")
        via_parts = ops.retrieval_score_indexed(parts, q, C)
        # 4. all three against the integer expectation (hence against each other), 5. the index against the exact means
        for name, got in (("retrieval_score", one_pass), ("chunk_mean + retrieval_score_indexed", via_index),
                          ("chunk_mean in pieces + retrieval_score_indexed", via_parts)):
            same(got, mat["want"], f"{cid}: {name} (head, chunk)")
        same(whole, want_parts, f"{cid}: whole index (head, chunk, d)")
        same(base, P.place(mat["k"], c["layout"])[1], f"{cid}: K was written")
    RAN.update(P.score_labels(c))


# ---- top-k ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(P.TOPK_SHAPES)), ids=[P.topk_id(i) for i in range(len(P.TOPK_SHAPES))])
def test_topk_probe(i):
    ops = _ops()
    t = P.topk_case(i)
    C, sets = t["C"], t["sets"]
    got = ops.retrieval_topk(t["scores"].to(DEV), sets)
    assert got.dtype == torch.int32 and got.shape == (P.TOPK_H, sets)
    got = got.cpu().tolist()
    for h in range(P.TOPK_H):
        row, want = got[h], t["want"][h]
        what = f"{P.topk_id(i)} head {h} ({t['kinds'][h]})"
        assert row[0] == 0, what
        assert all(0 <= x < C for x in row), what
        assert len(set(row)) == sets, what
        if row != want:
            j = next(j for j in range(sets) if row[j] != want[j])
            raise AssertionError(f"{what}: place {j}: got chunk {row[j]} (bits {t['bits'][h][row[j]]:#06x}), expected chunk "
                                 f"{want[j]} (bits {t['bits'][h][want[j]]:#06x})")
    RAN.update(P.topk_labels(i))


# ---- chunk gather -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.GATHER_CASES, ids=[P.gather_id(c) for c in P.GATHER_CASES])
def test_gather_probe(c):
    ops = _ops()
    mat = P.gather_material(c)
    chunk, D, H = c["chunk"], c["D"], P.GATHER_H
    idx = mat["idx"].to(DEV)
    n = idx.shape[1] * chunk
    ks, _ = P.place(mat["k"], c["src"], DEV)
    vs, _ = P.place(mat["v"], c["src"], DEV)
    kd, kd_base = P.place(sentinel(H, n + P.GATHER_GUARD, D), c["dst"], DEV)
    vd, vd_base = P.place(sentinel(H, n + P.GATHER_GUARD, D), c["dst"], DEV)
    ops.retrieval_gather(ks, vs, idx, kd, vd, chunk)
    for name, base, want_rows in (("K", kd_base, mat["want_k"]), ("V", vd_base, mat["want_v"])):
        want = sentinel(H, n + P.GATHER_GUARD, D)
        want[:, :n] = want_rows
        same(base, P.place(want, c["dst"])[1], f"{P.gather_id(c)}: gathered {name} (base buffer of the {c['dst']} layout)")
    if D == 128:
        T = mat["k"].shape[1]
        rows = mat["rows"]

        def dst_f8():
            codes = torch.full((H, n + P.GATHER_GUARD, D), CODE_SENTINEL, dtype=torch.uint8, device=DEV)
            exps = torch.full((H, n + P.GATHER_GUARD), EXP_SENTINEL, dtype=torch.uint8, device=DEV)
            return codes, exps

        def check(name, codes, exps, want_codes, want_exps):
            wc = torch.full((H, n + P.GATHER_GUARD, D), CODE_SENTINEL, dtype=torch.uint8)
            we = torch.full((H, n + P.GATHER_GUARD), EXP_SENTINEL, dtype=torch.uint8)
            wc[:, :n], we[:, :n] = want_codes, want_exps
            same(codes, wc, f"{P.gather_id(c)}: {name} codes")
            same(exps, we, f"{P.gather_id(c)}: {name} exponent bytes")
        # from codes: bytes and exponent bytes are the gathered source bytes
        kc, vc, ke, ve = P.f8_material(c)
        assert kc.shape == (H, T, D)
        (dkc, dke), (dvc, dve) = dst_f8(), dst_f8()
        ops.retrieval_gather_fp8(kc.to(DEV).view(torch.float8_e4m3fn), vc.to(DEV).view(torch.float8_e4m3fn), idx,
                                 dkc.view(torch.float8_e4m3fn), dvc.view(torch.float8_e4m3fn), dke, dve, chunk,
                                 src_exp=(ke.to(DEV), ve.to(DEV)))
        pick = rows[:, :, None].expand(-1, -1, D)
        check("K from codes", dkc, dke, torch.gather(kc, 1, pick), torch.gather(ke, 1, rows))
        check("V from codes", dvc, dve, torch.gather(vc, 1, pick), torch.gather(ve, 1, rows))
        # from fp16 rows: kv_quantize_ref of the expected rows
        (dkc, dke), (dvc, dve) = dst_f8(), dst_f8()
        ops.retrieval_gather_fp8(ks, vs, idx, dkc.view(torch.float8_e4m3fn), dvc.view(torch.float8_e4m3fn), dke, dve, chunk)
        wk, wke, _ = ops.kv_quantize_ref(mat["want_k"])
        wv, wve, _ = ops.kv_quantize_ref(mat["want_v"])
        check("K from fp16", dkc, dke, wk.view(torch.uint8), wke)
        check("V from fp16", dvc, dve, wv.view(torch.uint8), wve)
    RAN.update(P.gather_labels(c))


# ---- kv_copy_rows / _pair ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.COPY_CASES, ids=[P.copy_id(c) for c in P.COPY_CASES])
def test_kv_copy_probe(c):
    ops = _ops()
    mat = P.copy_material(c)
    L, H, D, n = c["L"], c["H"], c["D"], c["n"]
    sk, sk_base = P.place(mat["src_k"], c["src"], DEV)
    sv, sv_base = P.place(mat["src_v"], c["src"], DEV)
    layers = [1] if c["slice"] else None
    sl = slice(1, 2) if c["slice"] else slice(None)

    def dst():
        return P.place(sentinel(L, H, mat["Td"], D), c["dst"], DEV)

    def check(name, base, src):
        same(base, P.place(P.copy_expected(c, src, layers), c["dst"])[1], f"{P.copy_id(c)}: {name} (base buffer of the {c['dst']} layout)")
    d1, d1_base = dst()
    ops.kv_copy_rows(sk[sl], d1[sl], c["src_t0"], c["dst_t0"], n)
    check("kv_copy_rows", d1_base, mat["src_k"])
    dk, dk_base = dst()
    dv, dv_base = dst()
    assert ops._lhtd(sk) == ops._lhtd(sv) and ops._lhtd(dk) == ops._lhtd(dv)          # one launch, not the two-call fallback
    ops.kv_copy_rows_pair(sk[sl], sv[sl], dk[sl], dv[sl], c["src_t0"], c["dst_t0"], n)
    check("kv_copy_rows_pair K", dk_base, mat["src_k"])
    check("kv_copy_rows_pair V", dv_base, mat["src_v"])
    same(sk_base, P.place(mat["src_k"], c["src"])[1], f"{P.copy_id(c)}: the source was written")
    same(sv_base, P.place(mat["src_v"], c["src"])[1], f"{P.copy_id(c)}: the source was written")
    RAN.update(P.copy_labels(c))


# ---- kv_shift_rows / _pair --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", P.SHIFT_DS)
def test_kv_shift_probe(D):
    ops = _ops()
    for c in P.shift_cases(D):
        what = f"D{D} n{c['n']} shift{c['shift']} {c['layout']}"
        k, v, wk, wv = P.shift_material(c)
        src_t0 = P.SHIFT_DST_T0 + c["shift"]
        one, one_base = P.place(k, c["layout"], DEV)
        ops.kv_shift_rows(one, src_t0, P.SHIFT_DST_T0, c["n"])
        same(one_base, P.place(wk, c["layout"])[1], f"kv_shift_rows {what}")
        kk, kk_base = P.place(k, c["layout"], DEV)
        vv, vv_base = P.place(v, c["layout"], DEV)
        ops.kv_shift_rows_pair(kk, vv, src_t0, P.SHIFT_DST_T0, c["n"])
        same(kk_base, P.place(wk, c["layout"])[1], f"kv_shift_rows_pair K {what}")
        same(vv_base, P.place(wv, c["layout"])[1], f"kv_shift_rows_pair V {what}")
        RAN.update(P.shift_labels(c))


# ---- kv_gather_rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (64, 128))
def test_kv_gather_rows_probe(D):
    ops = _ops()
    for c in P.ROWS_CASES:
        if c["D"] != D:
            continue
        k, v, wk, wv = P.rows_material(c)
        kk, kk_base = P.place(k, c["layout"], DEV)
        vv, vv_base = P.place(v, c["layout"], DEV)
        ops.kv_gather_rows(kk, vv, P.ROWS_OFFSET, torch.tensor(c["idx"], dtype=torch.int32, device=DEV), max_index=max(c["idx"]))
        same(kk_base, P.place(wk, c["layout"])[1], f"kv_gather_rows K {P.rows_id(c)}")
        same(vv_base, P.place(wv, c["layout"])[1], f"kv_gather_rows V {P.rows_id(c)}")
        RAN.update(P.rows_labels(c))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_return_their_code_and_write_nothing():
    from triforce_amd import hip
    ops = _ops()
    lib = hip.lib()
    buf_h = torch.full((P.REFUSAL_BUFFERS["h"][1],), P.SENTINEL, dtype=torch.float16, device=DEV)
    buf_i = torch.ones(P.REFUSAL_BUFFERS["i"][1], dtype=torch.int32, device=DEV)
    for entry, over, code in P.REFUSALS:
        assert P.refusal_call(lib, entry, over, buf_h.data_ptr(), buf_i.data_ptr(), ops._stream()) == code, (entry, over)
        RAN.add(("refusal", entry))
    # the tensor-level wrapper: a head_dim past the shift kernel's 2048 (one row per workgroup trip) is refused
    cache = sentinel(1, 1, 6, 2056).to(DEV)
    with pytest.raises(hip.TriforceHipError, match="TF_EINVAL"):
        ops.kv_shift_rows(cache, 3, 1, 2)
    with pytest.raises(hip.TriforceHipError, match="TF_ERANGE"):
        ops.retrieval_topk(sentinel(1, 32769).to(DEV), 4)
    torch.cuda.synchronize()
    assert bool((buf_h == P.SENTINEL).all()) and bool((buf_i == 1).all()) and bool((cache == P.SENTINEL).all())


def test_zz_every_form_was_run():
    """The (kernel, path) labels the probes above actually ran (a deselected or failed case leaves a hole here)."""
    missing = sorted(P.REQUIRED - RAN)
    assert not missing, missing
