"""The sampling and accept kernels (csrc/sampling.hip) on exact-arithmetic material (tests/sampling_probes.py): every token,
record, token buffer and cursor must come back EQUAL to the int64 expectation, at every entry point, instance, data path and
slice edge of the case list.  No tolerance and no skipped case: what cannot be made exact was removed from the case list on the
CPU side (tests/sampling_probes.py states which and why; tests/test_sampling_probes_cpu.py proves the list against the oracle).

Poison.  Probability rows are views into a larger buffer whose floats before the first row and behind the last one are NaN
(4 floats for a 16-byte aligned base, 1 float for the base moved by one float): a 16-byte load that straddles an end, or a group
guard that is one off, turns a sum into NaN.  Uniform buffers hold NaN wherever no decision may read.  Integer outputs sit in
front of sentinels that must come back untouched.  Readbacks are batched: many launches, one ``.tolist()``.
"""
import pytest
import torch

from tests import sampling_probes as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7


def _ops():
    from triforce_amd import ops
    return ops


def embed(t, aligned=True):
    """``t`` (fp32, CPU) as a view into a NaN-padded device buffer: 4 floats of padding (aligned) or 1 (base moved by a float)."""
    pad = 4 if aligned else 1
    buf = torch.full((t.numel() + 2 * pad,), P.NAN, dtype=torch.float32, device=DEV)
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    assert (view.data_ptr() % 16 == 0) == aligned
    return view


def ivec(vals, extra=2, dtype=torch.int64):
    """An integer device vector in front of ``extra`` sentinels: (the view the kernel gets, the whole buffer)."""
    buf = torch.tensor(list(vals) + [SENT] * extra, dtype=dtype, device=DEV)
    return buf[:len(vals)], buf


def uvec(U, at=0):
    """Uniforms (U24, None = NaN) behind ``at`` NaN entries, with NaN behind them."""
    return torch.tensor([P.NAN] * at + [P.NAN if x is None else P.u_f32(x) for x in U] + [P.NAN] * 3, dtype=torch.float32, device=DEV)


# ---- sample_inverse_cdf, sample_inverse_cdf_cur ---------------------------------------------------------------------------
def _run_sample(V, cur):
    ops = _ops()
    rows = P.sample_rows(V)
    cursors = {c: torch.tensor([c], dtype=torch.int64, device=DEV) for c in (0, 5)}
    for aligned in P.alignments(V):
        row_buf = embed(torch.zeros(V), aligned)
        want, us = [], []
        for r in rows:
            for U, tok in r["probes"]:
                want.append(tok)
                us.append(U)
        n = len(want)
        out = torch.full((n + 1,), SENT, dtype=torch.int64, device=DEV)
        combos = [P.CUR_COMBOS[i % 4] for i in range(n)]
        ub = torch.full((n, P.UBUF_LEN), P.NAN, dtype=torch.float32)
        for i, U in enumerate(us):
            ub[i, (combos[i][0] + combos[i][1]) if cur else 0] = P.u_f32(U)
        ub = ub.to(DEV)
        k = 0
        for r in rows:
            idx = torch.tensor(r["idx"], dtype=torch.int64, device=DEV)
            if r["idx"]:
                row_buf[idx] = P.f32(r["wts"]).to(DEV)
            for _ in r["probes"]:
                if cur:
                    ops.sample_inverse_cdf_cur(row_buf, ub[k], cursors[combos[k][0]], combos[k][1], out[k:k + 1])
                else:
                    ops.sample_inverse_cdf(row_buf, ub[k, :1], out[k:k + 1])
                k += 1
            if r["idx"]:
                row_buf[idx] = 0.0
        got = out.tolist()
        bad = [(i, us[i], got[i], want[i]) for i in range(n) if got[i] != want[i]]
        assert not bad, (V, P.path_of(V, aligned), bad[:8])
        assert got[n] == SENT and int(cursors[0]) == 0 and int(cursors[5]) == 5


@pytest.mark.parametrize("V", P.SAMPLE_VOCABS)
def test_sample_inverse_cdf(V):
    _run_sample(V, cur=False)


@pytest.mark.parametrize("V", P.SAMPLE_VOCABS)
def test_sample_inverse_cdf_cur(V):
    _run_sample(V, cur=True)


# ---- accept_chain, accept_chain_cur, accept_chain_step --------------------------------------------------------------------
CHAIN_GROUPS = sorted({(c["g2"], c["V"]) for c in P.chain_cases()})


def _run_chain(entry, g2, V):
    ops = _ops()
    cases = [c for c in P.entry_cases(entry) if (c["g2"], c["V"]) == (g2, V)]
    assert cases
    p0, q0, tokens = P.chain_base(g2, V)
    pd, qd = embed(P.f32(p0).view(g2 + 1, V)), embed(P.f32(q0).view(g2, V))
    pf0, qf0 = P.f32(p0).view(g2 + 1, V), P.f32(q0).view(g2, V)
    tok_dev = torch.tensor(tokens, dtype=torch.int64, device=DEV)
    recs = torch.full((len(cases), 5), SENT, dtype=torch.int64, device=DEV)
    keep, wants = [], []
    for k, c in enumerate(cases):
        p, q = P.chain_apply(c, p0, q0)
        rec, U, _ = P.chain_expect(c, p, q, tokens)
        for which, i, t, x in c["patches"]:
            (pd if which == "p" else qd)[i, t] = float(P.f32([x])[0])
        at = 0 if entry == "accept_chain" else (0, 5)[k % 2]
        ub = uvec(U, at)
        out = recs[k, :4]
        if entry == "accept_chain":
            ops.accept_chain(pd, qd, tok_dev, ub, g2, c["inclusive"], c["eos"], out)
            keep.append(None)
        else:
            cursor = torch.tensor([at], dtype=torch.int64, device=DEV)
            if entry == "accept_chain_cur":
                ops.accept_chain_cur(pd, qd, tok_dev, ub, cursor, g2, c["inclusive"], c["eos"], out)
                keep.append((cursor,))
            else:
                nsets, na, nb = P.STEP_COMBOS[k % len(P.STEP_COMBOS)]
                tok_view, tok_buf = ivec([5] + tokens + [SENT - 1])
                s_src = torch.tensor([P.STEP_S_SRC], dtype=torch.int32, device=DEV)
                sets, bufs = [], []
                for n_pos, qlen in list(zip((na, nb), P.STEP_QLEN))[:nsets]:
                    pos_v, pos_b = ivec([SENT] * n_pos)
                    sl_v, sl_b = ivec([SENT], dtype=torch.int32)
                    sk_v, sk_b = ivec([SENT], dtype=torch.int32)
                    sets.append((pos_v, sl_v, sk_v, qlen))
                    bufs.append((n_pos, qlen, pos_b, sl_b, sk_b))
                ops.accept_chain_step(pd, qd, tok_view, ub, cursor, g2, c["inclusive"], c["eos"], P.PAD_TOKEN, s_src, sets, out)
                keep.append((cursor, tok_buf, bufs))
        for which, i, t, x in c["patches"]:
            (pd if which == "p" else qd)[i, t] = float((pf0 if which == "p" else qf0)[i, t])
        wants.append((rec, at))
    got = recs.tolist()
    for k, c in enumerate(cases):
        rec, at = wants[k]
        assert tuple(got[k][:4]) == rec and got[k][4] == SENT, (entry, c["what"], c["inclusive"], got[k], rec)
        if keep[k] is None:
            continue
        assert int(keep[k][0]) == at + rec[3], (entry, c["what"], "cursor")
        if entry == "accept_chain_step":
            _, tok_buf, bufs = keep[k]
            assert tok_buf.tolist() == P.step_expect(rec, tokens, g2) + [SENT, SENT], (c["what"], "tok_buf")
            s_new = P.STEP_S_SRC + rec[0] + 1
            for n_pos, qlen, pos_b, sl_b, sk_b in bufs:
                assert pos_b.tolist() == [s_new + i for i in range(n_pos)] + [SENT, SENT]
                assert sl_b.tolist() == [s_new, SENT, SENT] and sk_b.tolist() == [s_new + qlen, SENT, SENT]
    assert torch.equal(pd.cpu(), pf0) and torch.equal(qd.cpu(), qf0)


@pytest.mark.parametrize("g2,V", CHAIN_GROUPS)
def test_accept_chain(g2, V):
    _run_chain("accept_chain", g2, V)


@pytest.mark.parametrize("g2,V", CHAIN_GROUPS)
def test_accept_chain_cur(g2, V):
    _run_chain("accept_chain_cur", g2, V)


@pytest.mark.parametrize("g2,V", [g for g in CHAIN_GROUPS if g[0] <= 62])
def test_accept_chain_step(g2, V):
    _run_chain("accept_chain_step", g2, V)


# ---- middle_accept, middle_accept_cur, middle_accept2_cur, middle_accept_n_cur --------------------------------------------
def _run_mid(entry, V):
    ops = _ops()
    cases = [c for c in P.entry_cases(entry) if c["V"] == V]
    assert cases
    p = P.mid_base(V)
    pd = embed(P.f32(p).view(P.GAMMA + 1, V))
    qds = {pos: embed(P.f32(P.mid_q(V, pos))) for pos in range(P.GAMMA)}
    keep = []
    for k, c in enumerate(cases):
        cursored = entry != "middle_accept"
        at = (0, 5)[k % 2] if cursored else 0
        U = P.mid_uniforms(c)
        stages, tok_after, adv = P.mid_expect(c, p, None if cursored else P.GAMMA)
        tok_view, tok_buf = ivec(P.mid_tokens(c))
        cursor = torch.tensor([at], dtype=torch.int64, device=DEV)
        qs = [qds[c["n"] + 2 * s] for s in range(c["depth"])]
        if entry == "middle_accept":
            out = torch.full((5,), SENT, dtype=torch.int64, device=DEV)
            ops.middle_accept(pd, qs[0], tok_view, uvec(U[1:]), c["n"], P.GAMMA, out)
            want = list(stages[0]) + [SENT, SENT]
            adv = 0
        elif entry == "middle_accept_cur":
            out = torch.full((5,), SENT, dtype=torch.int64, device=DEV)
            ops.middle_accept_cur(pd, qs[0], tok_view, uvec(U, at), cursor, c["n"], P.GAMMA, out)
            want = list(stages[0]) + [at, SENT]
        else:
            out = torch.full((ops.mid_record_len(c["depth"]) + 1,), SENT, dtype=torch.int64, device=DEV)
            if entry == "middle_accept2_cur":
                ops.middle_accept2_cur(pd, qs[0], qs[-1], tok_view, uvec(U, at), cursor, c["n"], P.GAMMA, out[:-1], depth=c["depth"])
            else:
                ops.middle_accept_n_cur(pd, qs, tok_view, uvec(U, at), cursor, c["n"], P.GAMMA, out[:-1], depth=c["depth"])
            want = P.mid_record(stages, at, c["depth"]) + [SENT]
        keep.append((c, out, want, tok_buf, tok_after + [SENT, SENT], cursor, at + adv))
    for c, out, want, tok_buf, tok_want, cursor, cur_want in keep:
        assert out.tolist() == want, (entry, c, out.tolist(), want)
        assert tok_buf.tolist() == tok_want, (entry, c, "tokens")
        assert int(cursor) == cur_want, (entry, c, "cursor")


@pytest.mark.parametrize("V", P.MID_VOCABS)
def test_middle_accept(V):
    _run_mid("middle_accept", V)


@pytest.mark.parametrize("V", P.MID_VOCABS)
def test_middle_accept_cur(V):
    _run_mid("middle_accept_cur", V)


@pytest.mark.parametrize("V", P.MID_VOCABS)
def test_middle_accept2_cur(V):
    _run_mid("middle_accept2_cur", V)


@pytest.mark.parametrize("V", P.MID_VOCABS)
def test_middle_accept_n_cur(V):
    _run_mid("middle_accept_n_cur", V)


# ---- tree_accept ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", P.TREE_VOCABS)
def test_tree_accept(V):
    from oracle import ref_tree as RT
    from triforce_amd.utils.tree import successors_csr
    ops = _ops()
    keep = []
    for c in P.tree_cases(V):
        p, draft, tokens, u = P.tree_tensors(c)
        gm = RT.grow_map_from_branches(c["branches"])
        off, flat = successors_csr(gm["Successors"], DEV)
        out = torch.full((ops.TREE_ACCEPT_OUT + 1,), SENT, dtype=torch.int64, device=DEV)
        ops.tree_accept(embed(P.f32(p).view(p.shape)), draft.to(DEV), tokens.to(DEV), off, flat, u.to(DEV), P.TREE_T, out[:-1])
        keep.append((c, out))
    for c, out in keep:
        rec, w = out.tolist(), c["want"]
        got = dict(acc=rec[4:4 + rec[0]], next=rec[1], terminal=rec[2], consumed=rec[3])
        assert got == w and rec[0] == len(w["acc"]) and rec[-1] == SENT, (c["kind"], c["tokens"], got, w)


# ---- sample_without_replacement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,k", P.RACE_SHAPES)
def test_sample_without_replacement(V, k):
    ops = _ops()
    keep = []
    for c in [c for c in P.race_cases() if (c["V"], c["k"]) == (V, k)]:
        logits, rand = P.race_tensors(c)
        keep.append((c, ops.sample_without_replacement(logits.to(DEV), rand.to(DEV), k, P.RACE_T)))
    assert keep
    for c, out in keep:
        assert out.view(c["rows"], k).tolist() == c["want"], (c["rows"], c["ones"], c["dead"])
