"""Exact-arithmetic probes for the sampling and accept kernels (csrc/sampling.hip): material on which every sum the kernels
form is exact in fp32 IN ANY ORDER, so the expected token, record and cursor are statements about integers and are asserted
with ``==``.  Plain torch / Python integers and fractions on the CPU; tests/test_sampling_probes_cpu.py proves the material,
its conditions and the case list against the oracle (oracle/ref_ops.py, oracle/ref_tree.py) and the host forms of
triforce_amd.ops, tests/test_gpu_sampling_probes.py feeds the same cases to the kernels.  No kernel output ever produces an
expectation.

Material.  Every probability is an integer multiple of UNIT = 2^-20 with row total <= 2: every partial sum, in any order, is a
multiple of 2^-20 below 2^2 and exact in fp32 (tree-scanned wave prefixes, sequential in-slice sums, torch.cumsum alike), and
p - q is exact.  A uniform is U24 * 2^-24; a row total W (in units) is chosen so that u * total is exact, which
``product_exact`` checks for every (u, total) pair of the case list.  The expected token is then ``expect_token``: the first
index with non-zero mass whose integer cumulative count exceeds the integer target, the LAST index with non-zero mass when
no count does (u = 1.0 reaches the total exactly), and 0 for a row with no mass.  Accept tests use q[t] a power of two and
p[t] = r * q[t] with r dyadic, so the fp32 quotient is r exactly.

The rule for what cannot be made exact: it is removed from the case list, never given a tolerance.  Removed:
  * total 0.75 with u = 1 - 2^-24: the product 0.75 - 3 * 2^-26 needs 26 bits.  That pair is dropped wherever it would
    arise (the u = 1 - 2^-24 probe of a 0.75 row, and the "one step below the upper edge" probe of a 0.75 row whose edge bin
    is the last one); totals 1, 0.5 and 2 keep it.  The other probes of a 0.75 row sit at cumulative counts below 2^18
    units, where one 2^-24 step of u still gives an exact product.
  * tree walk, a second child REJECTED: the draft row behind one rejection is 1/15 on 15 tokens, which is not dyadic, so the
    residual after a second rejection is not exact.  That outcome is probed with u = 0 only (the first index of positive
    residual, whatever the rounding); every other tree probe has at most one rejection in front of an exact draw.

The slice rule of block_sample is restated here (``seg_of``, ``path_of``, ``edge_set``) to label every case with the
(instance, data path) pair it reaches.
"""
from fractions import Fraction

import torch

UNIT_LOG2 = 20
ONE = 1 << UNIT_LOG2                 # 1.0 in units of 2^-20
U_ONE = 1 << 24                      # 1.0 in steps of 2^-24
UO = 1 << 14                         # 1/64 in units: the grain of the multi-row material
SAMP_THREADS = 1024
NAN = float("nan")
TOTALS = (ONE, ONE // 2, 3 * ONE // 4, 2 * ONE)
SAMPLE_VOCABS = (1, 3, 1023, 1024, 1025, 4100, 32000, 32768, 32770, 32772, 40000, 128256, 262144)


def f32(units):
    """fp32 image of an int64 weight vector (or a list of ints) in units of 2^-20."""
    return (torch.as_tensor(units, dtype=torch.int64).double() * 2.0 ** -UNIT_LOG2).float()


def u_f32(U24):
    return float(U24) * 2.0 ** -24


def product_exact(U24, W):
    """float32(u) * float32(total) == the rational product u * total (u = U24 * 2^-24, total = W * 2^-20)."""
    got = torch.tensor(u_f32(U24), dtype=torch.float32) * torch.tensor(W * 2.0 ** -UNIT_LOG2, dtype=torch.float32)
    return Fraction(float(got)) == Fraction(U24, U_ONE) * Fraction(W, ONE)


def row(V, support, weights):
    """(int64 weight vector in units of 2^-20, its fp32 image): zero everywhere but ``support``."""
    w = torch.zeros(V, dtype=torch.int64)
    for i, x in zip(support, weights):
        assert 0 <= i < V and w[i] == 0 and x >= 0
        w[i] = x
    return w, f32(w)


def expect_token(w, U24, total=None):
    """The int64 rule: first index i with w[i] > 0 and cumsum(w)[i] * 2^24 > U24 * total; the last index with w > 0 when
    there is none; 0 for a row with no mass."""
    w = torch.as_tensor(w, dtype=torch.int64)
    total = int(w.sum()) if total is None else int(total)
    assert total == int(w.sum()) and total <= 2 * ONE
    nz = (w > 0).nonzero().flatten()
    if nz.numel() == 0:
        return 0
    c = torch.cumsum(w, 0)[nz] * U_ONE
    hit = (c > U24 * total).nonzero().flatten()
    return int(nz[hit[0]]) if hit.numel() else int(nz[-1])


# ---- block_sample's slices, restated ----------------------------------------------------------------------------------------
def seg_of(V):
    """seg = roundup4(ceil(V / 1024)): thread t owns [t * seg, (t + 1) * seg)."""
    return (((V + SAMP_THREADS - 1) // SAMP_THREADS) + 3) & ~3


def path_of(V, aligned):
    """The (instance, data path) pair of block_sample at vocabulary V with a 16-byte aligned base or not."""
    large, vec = V > SAMP_THREADS * 32, V % 4 == 0 and aligned
    if not large:
        return "reg4" if vec else "elem_small"
    if vec:
        return "stream"
    return "elem_large_mod4" if V % 4 else "elem_large_misaligned"


ALL_PATHS = {"reg4", "elem_small", "stream", "elem_large_mod4", "elem_large_misaligned"}


def edge_set(V):
    seg = seg_of(V)
    t_last = (V - 1) // seg
    E = {0, 1, seg - 1, seg, 64 * seg - 1, 64 * seg, t_last * seg, V - 2, V - 1}
    if V > SAMP_THREADS * 32:
        E |= {15, 16}
        if seg % 16:
            E.add(16 * ((seg - 1) // 16) + 15)          # last index of thread 0's last 16-element group: it straddles i1 = seg
    return sorted(e for e in E if 0 <= e < V)


def alignments(V):
    """Every V runs with a 16-byte aligned base; V % 4 == 0 also with the base moved by one float."""
    return (True, False) if V % 4 == 0 else (True,)


# ---- sample_inverse_cdf -----------------------------------------------------------------------------------------------------
def _before(e):
    return None if e == 0 else (max(1, e // 2) if e >= 3 else 0)


def _after(e, V):
    r = V - 1 - e
    return None if r == 0 else (e + max(2, r // 2) if r >= 3 else V - 1)


def sample_rows(V):
    """One row per (edge index e, total W): mass W/8 at a bin before e (when there is room), W/8 at e, the rest behind it;
    the uniforms walk both edges of e's bin, u = 0, 1 - 2^-24 and 1.0.  Each row is a dict with ``idx``/``wts`` (the support),
    ``W``, ``e`` and ``probes`` = [(U24, expected token)]; ``dropped`` lists the (U24, W) pairs whose product is inexact."""
    out = []
    for e in edge_set(V):
        for W in TOTALS:
            a, b = _before(e), _after(e, V)
            lo = W // 8 if a is not None else 0
            hi = lo + W // 8 if b is not None else W
            idx = [i for i in (a, e, b) if i is not None]
            wts = ([lo] if a is not None else []) + [hi - lo] + ([W - hi] if b is not None else [])
            w, _ = row(V, idx, wts)
            assert (lo * U_ONE) % W == 0 and (hi * U_ONE) % W == 0
            ulo, uhi = lo * U_ONE // W, hi * U_ONE // W
            cand = {ulo, ulo - 1, uhi, uhi - 1, 0, U_ONE - 1, U_ONE}
            probes, dropped = [], []
            for U in sorted(u for u in cand if 0 <= u <= U_ONE):
                (probes if product_exact(U, W) else dropped).append(U)
            out.append(dict(V=V, e=e, W=W, idx=idx, wts=wts, lo=ulo, hi=uhi, dropped=dropped,
                            probes=[(U, expect_token(w, U, W)) for U in probes]))
    # rows with no mass at all: token 0 at every u
    out.append(dict(V=V, e=None, W=0, idx=[], wts=[], lo=0, hi=0, dropped=[], probes=[(0, 0), (U_ONE // 2, 0), (U_ONE, 0)]))
    return out


def dense_row(r):
    return row(r["V"], r["idx"], r["wts"])


CUR_COMBOS = ((0, 0), (0, 2), (5, 0), (5, 2))          # (cursor, off) of the cursor form, cycled over the launches
UBUF_LEN = 8


# ---- multi-row material: disjoint blocks of 16 slots per row ----------------------------------------------------------------
def slot(i, j, V, rows):
    """Token of slot j (0 .. 15) in the block of row i: blocks are disjoint, p[0] and p[V - 1] stay zero."""
    S = max(16, (V - 4) // rows)
    return 2 + i * S + j * (S // 16)


# slot -> (p, q) in units of UO = 1/64.  Slot 0 is the drafted token (set per case).  Residual max(p - q, 0): 16 at slots 4 and
# 6 (total 1/2); q's excess sits IN FRONT of them at slot 2, so |p - q| (20, 16, 16, 16) and p alone (4, 40, 20, 16) put u = 1/2
# on slot 4 where the residual puts it on slot 6.  Slot 10 is q alone.
CHAIN_SLOTS = {2: (4, 24), 4: (40, 24), 6: (20, 4), 8: (16, 16), 10: (0, 16)}
BONUS_SLOTS = {2: 4, 4: 24, 6: 20, 8: 16}              # the plain row p[g2]: total 1, an edge at 28/64 between slots 4 and 6
RATIOS = {"3/4": Fraction(3, 4), "2^-10": Fraction(1, 1024), "1": Fraction(1), "4": Fraction(4)}
CHAIN_G2 = (1, 2, 18, 62, 63)
PAD_TOKEN = 999999


def chain_base(g2, V):
    """Integer (g2 + 1, V) p and (g2, V) q: every drafted token with ratio 4 (clamped to 1: accepted at u < 1)."""
    rows = g2 + 1
    assert slot(g2, 15, V, rows) < V - 1
    p = torch.zeros(rows, V, dtype=torch.int64)
    q = torch.zeros(g2, V, dtype=torch.int64)
    tokens = []
    for i in range(g2):
        for j, (pv, qv) in CHAIN_SLOTS.items():
            p[i, slot(i, j, V, rows)] = pv * UO
            q[i, slot(i, j, V, rows)] = qv * UO
        t = slot(i, 0, V, rows)
        p[i, t], q[i, t] = 4 * UO, UO
        tokens.append(t)
    for j, pv in BONUS_SLOTS.items():
        p[g2, slot(g2, j, V, rows)] = pv * UO
    return p, q, tokens


def _ratio(pv, qv):
    if qv == 0:
        return None if pv == 0 else "inf"                # None: 0 / 0 = NaN, every comparison False
    return Fraction(pv, qv)


def _passes(U24, ratio, inclusive):
    if ratio is None:
        return False
    m, u = (Fraction(1) if ratio == "inf" else min(Fraction(1), ratio)), Fraction(U24, U_ONE)
    return u <= m if inclusive else u < m


def chain_apply(c, p, q):
    """The case's patches [(which, row, token, units)] on clones of the base."""
    p, q = p.clone(), q.clone()
    for which, i, t, x in c["patches"]:
        (p if which == "p" else q)[i, t] = x
    return p, q


def chain_expect(c, p, q, tokens):
    """(count, next, reason, consumed), the uniforms (U24 per entry, None = never read) and the (w, U24) of the draw."""
    g2 = c["g2"]
    U = [U_ONE // 2] * (g2 + 1)
    for i, x in c["u"].items():
        U[i] = x
    flags = [_passes(U[i], _ratio(int(p[i, tokens[i]]), int(q[i, tokens[i]])), c["inclusive"]) for i in range(g2)]
    count = flags.index(False) if False in flags else g2
    reason = 1 if count == g2 else 0
    for i in range(count):
        if tokens[i] == c["eos"] and i + 1 < g2:
            count, reason = i + 1, 2
            break
    examined = count + 1 if reason == 0 else count
    if reason == 2:
        return (count, c["eos"], 2, examined), U, None
    w = (p[count] - q[count]).clamp(min=0) if reason == 0 else p[g2]
    W = int(w.sum())
    edge = (W // 2 if reason == 0 else 28 * W // 64) * U_ONE // W       # the edge between slots 4 and 6 of the sampled row
    U[examined] = edge - c["draw_below"]
    if W & (W - 1):           # a token with p > q rejected at u = 1.0 leaves p - q in the residual: no dyadic edge; draw at an end
        U[examined] = 0 if c["draw_below"] else U_ONE
    return (count, expect_token(w, U[examined], W), reason, examined + 1), U, (w, U[examined], W)


def chain_cases():
    cases = []
    for g2 in CHAIN_G2:
        for V in ((1028, 1030, 32768, 32770, 32772) if g2 <= 2 else (1028,)):      # 1030, 32770: the element path of both instances
            _, _, tokens = chain_base(g2, V)
            k = 0
            for pos in sorted({x for x in (0, 1, g2 - 2, g2 - 1) if 0 <= x < g2}):
                t = tokens[pos]
                for name, r in RATIOS.items():
                    edge = min(U_ONE, int(r * U_ONE))
                    for du in ((-1, 0, 1) if r < 1 else (-1, 0)):
                        for inclusive in (False, True):
                            cases.append(dict(g2=g2, V=V, inclusive=inclusive, eos=-1, draw_below=k % 2, u={pos: edge + du},
                                              patches=[("p", pos, t, int(r * UO))], what=f"r={name} at {pos} du={du}"))
                            k += 1
                # q[t] = 0, p[t] > 0: inf clamps to 1, at u = 1.0 accepted iff inclusive;  q[t] = p[t] = 0: NaN, rejected, the residual row is drawn
                for inclusive in (False, True):
                    cases.append(dict(g2=g2, V=V, inclusive=inclusive, eos=-1, draw_below=0, u={pos: U_ONE},
                                      patches=[("q", pos, t, 0)], what=f"inf at {pos}"))
                    cases.append(dict(g2=g2, V=V, inclusive=inclusive, eos=-1, draw_below=1, u={pos: 0},
                                      patches=[("p", pos, t, 0), ("q", pos, t, 0)], what=f"nan at {pos}"))
            if g2 >= 2 and V == 1028:
                rej = g2 // 2
                reject = {rej: U_ONE}                                     # u = 1.0 against a ratio of 3/4: rejected
                eos = [("eos accepted before the last", {}, tokens[min(1, g2 - 2)]), ("eos at the last position", {}, tokens[g2 - 1])]
                if g2 >= 18:
                    eos += [("eos at the rejected position", reject, tokens[rej]), ("eos behind the reject", reject, tokens[rej + 2]),
                            ("eos in front of the reject", reject, tokens[rej - 1])]
                for what, u, e in eos:
                    cases.append(dict(g2=g2, V=V, inclusive=False, eos=e, draw_below=0, u=dict(u), what=what,
                                      patches=[("p", rej, tokens[rej], 3 * UO // 4)] if u else []))
    return cases


# (nsets, n_pos of set a, n_pos of set b) of accept_chain_step, cycled over its cases
STEP_COMBOS = ((0, 0, 0), (1, 1, 0), (1, 64, 0), (2, 1, 64), (2, 64, 1))
STEP_S_SRC, STEP_QLEN = 1000, (7, 19)


def step_expect(rec, tokens, g2):
    """tok_buf[0 .. g2 + 1] after the launch: [next0, accepted.., resampled | bonus | PAD, PAD..]."""
    count, nxt, reason, _ = rec
    buf = [5] + list(tokens)
    want = buf[:count + 1] + [nxt if reason != 2 else PAD_TOKEN]
    return want + [PAD_TOKEN] * (g2 + 2 - len(want))


# ---- Middle_Spec -------------------------------------------------------------------------------------------------------------
GAMMA = 8
MID_VOCABS = (1028, 32772)
MID_SLOTS = {0: 3, 2: 1, 4: 24, 6: 20, 8: 16}          # p row: total 1; slot 0 is the drafted token (q = 4/64: ratio 3/4)
MID_RATIO = Fraction(3, 4)
MID_FILL = 7                                           # token entries no stage reads


def mid_base(V):
    rows = GAMMA + 1
    p = torch.zeros(rows, V, dtype=torch.int64)
    for i in range(rows):
        for j, pv in MID_SLOTS.items():
            p[i, slot(i, j, V, rows)] = pv * UO
    return p


def mid_q(V, pos):
    """The draft row of the stage at position ``pos``: 4/64 at the drafted token, the rest of the mass on slots no p row has."""
    q = torch.zeros(V, dtype=torch.int64)
    q[slot(pos, 0, V, GAMMA + 1)] = 4 * UO
    q[slot(pos, 11, V, GAMMA + 1)] = 60 * UO
    return q


def mid_cases():
    """depth 1 .. 4; a focus stage takes the boundary triple (du) and the follow-up on the guess or one bin off it (below);
    stages around it accept one step inside and hit the guess.  n = 0 and the last legal n, token buffers of gamma + 1 and
    gamma + 2 entries."""
    cases = []
    for V in MID_VOCABS:
        for depth in (1, 2, 3, 4):
            for s in range(depth):
                for du, below in ((-1, 0), (-1, 1), (0, 0), (0, 1), (1, 0)):
                    for n in (0, GAMMA - 2 * depth + 1):
                        for tok_len in (GAMMA + 1, GAMMA + 2):
                            stages = [(-1, 0)] * depth
                            stages[s] = (du, below)
                            cases.append(dict(V=V, depth=depth, n=n, tok_len=tok_len, stages=stages))
    return cases


def mid_tokens(c):
    V, n = c["V"], c["n"]
    tok = [MID_FILL] * c["tok_len"]
    for s in range(c["depth"]):
        pos = n + 2 * s
        tok[pos + 1] = slot(pos, 0, V, GAMMA + 1)                       # the drafted token d
        if pos + 2 < len(tok) and s + 1 < c["depth"]:
            tok[pos + 2] = slot(pos + 1, 6, V, GAMMA + 1)               # the guess: the follow-up of an accept drawn ON the edge
    return tok


def mid_uniforms(c):
    """U24 of u[0 .. 3 depth): u[3 s] belongs to the draft's draw (never read here: None), u[3 s + 1] is the accept test,
    u[3 s + 2] the follow-up draw."""
    U = []
    for du, below in c["stages"]:
        U += [None, int(MID_RATIO * U_ONE) + du, 28 * U_ONE // 64 - below]
    return U


def mid_expect(c, p, limit=None):
    """(stages [(acc, b, d)], tokens after, cursor advance) from integers; every row's total is 1.  ``limit``: the last token
    index a follow-up may be written to (the cursor forms: gamma + 1 when the buffer has gamma + 2 entries, else gamma)."""
    tok, U, n = mid_tokens(c), mid_uniforms(c), c["n"]
    if limit is None:
        limit = GAMMA + 1 if c["tok_len"] >= GAMMA + 2 else GAMMA
    stages = []
    for s in range(c["depth"]):
        pos = n + 2 * s
        d = tok[pos + 1]
        q = mid_q(c["V"], pos)
        acc = int(_passes(U[3 * s + 1], _ratio(int(p[pos, d]), int(q[d])), False))
        b = expect_token(p[pos + acc], U[3 * s + 2], ONE)
        stages.append((acc, b, d))
        if not (s + 1 < c["depth"] and acc == 1 and b == tok[pos + 2]):
            break
    acc, b, _ = stages[-1]
    if pos + 1 + acc <= limit:
        tok[pos + 1 + acc] = b
    return stages, tok, 3 * len(stages)


def mid_record(stages, at, depth):
    rec = list(stages[0]) + [at, len(stages) - 1]
    for s in range(1, depth):
        rec += list(stages[s]) if s < len(stages) else [0, 0, 0]
    return rec


# ---- Sequoia tree walk ------------------------------------------------------------------------------------------------------
TREE_VOCABS = (48, 1000, 32736, 32767, 32768)
TREE_T = 0.6
TREE_K = 16                                            # the draft row's support: softmax(0 / T) = 1/16 exactly


def tree_support(V):
    """16 tokens: 0, 1, 2, both sides of the 32-entry slice edges at the front, the middle and the end, V - 2, V - 1."""
    m, L = 32 * (V // 64), 32 * ((V - 1) // 32)
    cand = [0, 1, 2, 31, 32, m - 1, m, L - 1, L, V - 2, V - 1, 63, 64, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]
    out = []
    for x in cand:
        if 0 <= x < V and x not in out:
            out.append(x)
    return sorted(out[:TREE_K])


def tree_pairs(V):
    """Adjacent tokens on both sides of a slice edge (32 t - 1, 32 t), and (V - 2, V - 1)."""
    m, L = 32 * (V // 64), 32 * ((V - 1) // 32)
    out = []
    for a in (32, m, L, V - 1):
        if a - 1 > 5 and (a - 1, a) not in out and a < V:
            out.append((a - 1, a))
    return out


def tree_cases(V):
    """Each case: successors, tokens per node, integer target rows, the uniforms (U24) and the expected record.
    kind A: root with one child x.  r = 1/2 exactly: p[x] = r q[x], rejected, draw from the residual (1/2 at y1, 1/2 at y2)
            on their edge or one step below; r one step lower: accepted, then (x in {0, 2}: terminal) the leaf's plain row.
    kind B: root with two children.  x1 rejected on the boundary; x2 = y1 has residual 1/2 against r q = 1/30: accepted
            (margin 15), draw from its leaf's plain row.  B0: x2 has residual 0: rejected, u = 0 draws the first index of
            positive mass."""
    sup = tree_support(V)
    pairs = tree_pairs(V)
    cases = []
    k = 0
    for x in [t for t in (0, 1, 2, 31, 32, V - 1) if t in sup]:
        others = [t for t in sup if t != x]
        # the two 5/16 tokens: an adjacent pair of the support where there is one without x, else the two largest others
        adj = [(a, b) for a, b in pairs if a in others and b in others]
        y1, y2 = adj[k % len(adj)] if adj else (others[-2], others[-1])
        rest = [t for t in others if t not in (y1, y2)]
        root = {x: ONE // 32, y1: 5 * ONE // 16, y2: 5 * ONE // 16, rest[5]: ONE // 32}
        root.update({t: ONE // 16 for t in rest[:5]})
        c2, c3 = pairs[k % len(pairs)]
        leaf = {5: 4 * UO, c2: 24 * UO, c3: 36 * UO} if c3 == V - 1 else {5: 4 * UO, c2: 24 * UO, c3: 20 * UO, V - 1: 16 * UO}
        half, edge = U_ONE // 2, 28 * U_ONE // 64
        for below in (0, 1):
            cases.append(dict(V=V, kind="A-reject", branches=[[1]], tokens=[0, x], rows=[root, leaf], sup=sup,
                              u=[half, half - below], want=dict(acc=[0], next=(y1 if below else y2), terminal=0, consumed=2)))
            term = int(x in (0, 2))
            cases.append(dict(V=V, kind="A-accept", branches=[[1]], tokens=[0, x], rows=[root, leaf], sup=sup,
                              u=[half - 1, edge - below],
                              want=dict(acc=[0, 1], next=0 if term else (c2 if below else c3), terminal=term, consumed=1 if term else 2)))
            cases.append(dict(V=V, kind="B-accept", branches=[[2]], tokens=[0, x, y1], rows=[root, leaf, leaf], sup=sup,
                              u=[half, half, edge - below],
                              want=dict(acc=[0, 2], next=(c2 if below else c3), terminal=0, consumed=3)))
        cases.append(dict(V=V, kind="B0-reject", branches=[[2]], tokens=[0, x, rest[0]], rows=[root, leaf, leaf], sup=sup,
                          u=[half, half, 0], want=dict(acc=[0], next=y1, terminal=0, consumed=3)))
        k += 1
    return cases


def tree_tensors(c):
    V, N = c["V"], len(c["tokens"])
    p = torch.zeros(N, V, dtype=torch.int64)
    for i, r in enumerate(c["rows"]):
        for t, x in r.items():
            p[i, t] = x
    draft = torch.full((N, V), float("-inf"))
    draft[:, c["sup"]] = 0.0
    u = torch.tensor([u_f32(x) for x in c["u"]] + [NAN] * 4, dtype=torch.float32)
    return p, draft, torch.tensor(c["tokens"], dtype=torch.int64), u


def tree_model(c):
    """The walk in exact fractions (first child) — independent of oracle/ref_tree.py; asserts the margins the case claims."""
    p = {t: Fraction(x, ONE) for t, x in c["rows"][0].items()}
    q = Fraction(1, TREE_K)
    kids = list(range(1, 1 + c["branches"][0][0]))
    U = [Fraction(x, U_ONE) for x in c["u"]]
    x1 = c["tokens"][1]
    used = 1
    if p.get(x1, Fraction(0)) > U[0] * q:
        node, res = 1, None
    else:
        res = {t: max(v - q, Fraction(0)) for t, v in p.items()}
        S = sum(res.values())
        assert S.numerator == 1 and S.denominator & (S.denominator - 1) == 0, "residual mass is a power of two"
        res = {t: v / S for t, v in res.items() if v > 0}
        node = None
        if len(kids) == 2:
            used = 2
            x2 = c["tokens"][2]
            q2 = Fraction(1, TREE_K - 1)
            lhs, rhs = res.get(x2, Fraction(0)), U[1] * q2
            assert lhs == 0 or lhs >= 2 * rhs, "second child: a factor of 2 at least"
            if lhs > rhs:
                node, res = 2, None
            else:
                res = {t: v - q2 for t, v in res.items() if v > q2}
                assert c["u"][used] == 0, "a second rejection is probed at u = 0 only"
    acc = [0] + ([node] if node else [])
    if node and c["tokens"][node] in (0, 2):
        return dict(acc=acc, next=0, terminal=1, consumed=used)
    if node:
        w = torch.zeros(c["V"], dtype=torch.int64)
        for t, x in c["rows"][node].items():
            w[t] = x
        return dict(acc=acc, next=expect_token(w, c["u"][used], ONE), terminal=0, consumed=used + 1)
    den = 1
    for v in res.values():
        den = max(den, v.denominator)
    w = torch.zeros(c["V"], dtype=torch.int64)
    for t, v in res.items():
        w[t] = int(v * den) if den <= ONE else 1
    nxt = min(res) if c["u"][used] == 0 else expect_token(w, c["u"][used], int(w.sum()))
    return dict(acc=acc, next=nxt, terminal=0, consumed=used + 1)


# ---- the race without replacement: select probes ----------------------------------------------------------------------------
RACE_T = 0.6
RACE_SHAPES = ((16, 16), (1000, 1), (1000, 7), (1000, 16), (32767, 1), (32767, 7), (32767, 16), (32768, 1), (32768, 7), (32768, 16))


def race_edges(V):
    return sorted({x for x in (0, 1023, 1024, V - 1, 31 * 1024 + 1023) if 0 <= x < V})


def race_cases():
    """rand = 1.0 (log = 0: key exactly 0, the best possible) at the ``ones``, 0.5 elsewhere.  extra = 0: exactly k ones, out
    is those ids ascending; extra = 3: k + 3 ones, out is the k lowest; ninf: one more 1.0 at a token whose logit is -inf
    (0 / 0: never drawn)."""
    cases = []
    for V, k in RACE_SHAPES:
        for rows in (1, 5):
            for extra, ninf in ((0, False), (3, False), (0, True)):
                if k + extra + int(ninf) > V:
                    continue
                E = race_edges(V)
                ones, dead = [], []
                for r in range(rows):
                    want = k + extra
                    ids = []
                    for j in range(max(1, len(E) - r % 3)):             # walk the edge set: another start and length per row
                        if len(ids) < want:
                            ids.append(E[(r + j) % len(E)])
                    j = 0
                    while len(ids) < want:
                        x = (37 * r + 1021 * j + 5) % V
                        if x not in ids:
                            ids.append(x)
                        j += 1
                    ones.append(sorted(set(ids)))
                    assert len(ones[-1]) == want
                    dead.append(next(x for x in range(V) if x not in ids) if ninf else None)   # the lowest free id: it would win every tie
                cases.append(dict(V=V, k=k, rows=rows, ones=ones, dead=dead if ninf else [None] * rows,
                                  want=[o[:k] for o in ones]))
    return cases


def race_tensors(c):
    V, rows = c["V"], c["rows"]
    i = torch.arange(V)
    logits = (((i * 7) % 13).float() - 6.0) / 4.0
    logits = logits.repeat(rows, 1).contiguous()
    rand = torch.full((rows, V), 0.5, dtype=torch.float16)
    for r in range(rows):
        rand[r, c["ones"][r]] = 1.0
        if c["dead"][r] is not None:
            rand[r, c["dead"][r]] = 1.0
            logits[r, c["dead"][r]] = float("-inf")
    return logits, rand


# ---- the case list by entry point of triforce_amd.ops -----------------------------------------------------------------------
ENTRY_POINTS = ("sample_inverse_cdf", "sample_inverse_cdf_cur", "accept_chain", "accept_chain_cur", "accept_chain_step",
                "middle_accept", "middle_accept_cur", "middle_accept2_cur", "middle_accept_n_cur", "tree_accept",
                "sample_without_replacement")


def entry_cases(name):
    """The cases an entry point is fed (tests/test_gpu_sampling_probes.py takes them from here)."""
    if name.startswith("sample_inverse_cdf"):
        return [r for V in SAMPLE_VOCABS for r in sample_rows(V)]
    if name.startswith("accept_chain"):
        return [c for c in chain_cases() if name != "accept_chain_step" or c["g2"] <= 62]
    if name.startswith("middle_accept"):
        cap = {"middle_accept": 1, "middle_accept_cur": 1, "middle_accept2_cur": 2, "middle_accept_n_cur": 4}[name]
        return [c for c in mid_cases() if c["depth"] <= cap]
    if name == "tree_accept":
        return [c for V in TREE_VOCABS for c in tree_cases(V)]
    if name == "sample_without_replacement":
        return race_cases()
    raise KeyError(name)
