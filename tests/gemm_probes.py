"""Exact-arithmetic probes for the skinny decode GEMMs (csrc/gemv.hip, csrc/gemv_fp8.hip): inputs on which every partial
sum of the K reduction is exact in fp32 IN ANY ORDER, so the expected output is known bit for bit whatever the summation
order, the weight packing or the launch form.  Plain torch on the CPU, seeded, int64 / float64; tests/test_gemm_probes_cpu.py
proves the material, its conditions and the case list, tests/test_gpu_gemm_probes.py feeds the same cases to the kernels.

Material.  ``select``: row n of W is zero except W[n, k_n] = w_n = +-2^j (j cycling over -2 .. 2), so y[m, n] = w_n * h[m, k_n]
— one non-zero term plus exact zeros.  The k_n walk the edge set E(K) (``edge_set``); a case is as many launches as E(K) needs
at its N.  ``dense``: W in {-1, 0, +1}, a quarter non-zero; every partial sum is an integer multiple of the case's step far
below 2^24.  The input rows: without a norm prologue x is randn fp16 (select) or +-1 (dense); with one, x[m, :] = +-c_m with
c_m a power of two that differs from row to row, so fp16(x * rsqrt(mean(x^2) + eps)) = +-1 exactly (the fp16 spacing below 1
is 4.9e-4, eps / c_m^2 <= 4e-5) and h = +-ln[k]: ln is randn fp16 for select (it carries the k index), one of 0.5, 1, 2, -1 for
dense.  A norm scale taken from another row shows as a wrong power of two.  ``poison``: see tests/test_gpu_gemm_probes.py.

The launch rule (csrc/sg_rule.h) is restated here (``pick_form``, ``pick_ks``, ``pick_n8``, ``fp8_form``) to label every case
with the kernel form it reaches; tests/native/test_gemm_probe_rule.cpp holds the restatement against the header.
"""
import torch

from oracle import ref_ops as R

EPS = 1e-5
SENTINEL = -1234.0                     # what outputs are pre-filled with (an fp16 value, not zero: a kernel that stores zeros past row M shows)
SLOT0, POS_MAX = 3, 64
# SwiGLU: the kernel evaluates gf / (1 + expf(-gf)) in fp32.  A float32 torch evaluation of that expression deviates from
# float64 by at most 1.31e-7 (relative; measured over the probes' own gate values by test_gemm_probes_cpu.py, which also
# asserts 32 x the measured figure <= DELTA); 32 x that = 4.2e-6 (~ 2^-17.9) allows for the device's expf.
DELTA = 4.25e-6
UNSAFE_CAP = 0.01                      # share of a case's SwiGLU elements that may be unsafe (within DELTA of an fp16 boundary)

SG_PLAIN, SG_GATEUP, SG_F32, SG_QKV, SG_QKVG = 0, 1, 2, 3, 4
KNOB_DEFAULTS = {0: 1, 2: 420, 3: 0, 4: 0, 5: 200}                 # SgKnobs of csrc/sg_rule.h, by tf_sg_tune key
SG_WAVES, SG_WAVES_WIDE, SG_WIDE_MAX_PANELS, SG_KSPLIT_MAX, SG_TICKETS, SG_N8_WAVES = 4, 8, 512, 4, 4096, 8


# ---- the launch rule, restated ---------------------------------------------------------------------------------------------
def knobs_of(c):
    kn = dict(KNOB_DEFAULTS)
    kn.update(dict(c["knobs"]))
    return kn


def pick_form(mode, M, N, K, kn):
    """sg_pick_form: (row tiles, waves per workgroup, panels per wave)."""
    panels, nchunks, MT = N // 16, K >> 5, 1 if M <= 16 else 2
    if M >= kn[0] and panels % 2 == 0 and panels // 2 >= kn[2] and nchunks >= 16:
        return MT, SG_WAVES, 2
    if mode == SG_GATEUP:
        return MT, (SG_WAVES_WIDE if (M > 16 and panels <= kn[5] and nchunks >= 32) else SG_WAVES), 1
    wide = panels <= SG_WIDE_MAX_PANELS and nchunks >= 2 * SG_WAVES_WIDE
    return MT, (SG_WAVES_WIDE if wide else SG_WAVES), 1


def pick_ks(panels, P, nchunks, WAVES, mode, kn):
    """sg_pick_ks: workgroups per panel along K."""
    if P != 1 or mode == SG_F32 or panels > SG_TICKETS or kn[4] == 1:
        return 1
    if kn[4] > 1:
        ks = kn[4]
    elif 256 < panels <= 384 and nchunks >= 256:
        ks = 3
    else:
        if panels >= kn[3]:
            return 1
        ks = (256 + panels - 1) // panels
    ks = min(ks, SG_KSPLIT_MAX)
    while ks > 1 and nchunks // ks < 2 * WAVES:
        ks -= 1
    return max(ks, 1)


def pick_n8(mode, M, K):
    """sg_pick_n8: (8-row tiles, super-chunks in flight per wave)."""
    nsc = K >> 6
    cpw = (nsc + SG_N8_WAVES - 1) // SG_N8_WAVES
    MT = 1 if M <= 8 else 2 if M <= 16 else 3
    if (cpw > 8 and cpw % 5 == 0) or (mode != SG_GATEUP and MT == 3):
        return MT, 5
    return MT, (4 if (mode == SG_GATEUP and MT > 1) else 8)


def fp8_form(mode, M, N, K):
    """launch_f8 of csrc/gemv_fp8.hip: (row tiles, waves per workgroup)."""
    wide = mode != SG_GATEUP and N // 16 <= 512 and (K >> 6) >= 16
    return (1 if M <= 16 else 2), (8 if wide else 4)


EPS_OF = {"plain": SG_PLAIN, "f32": SG_F32, "gateup": SG_GATEUP, "qkv": SG_QKV, "qkvg": SG_QKVG, "gateup_n8": SG_GATEUP,
          "qkv_n8": SG_QKV, "plain_fp8": SG_PLAIN, "gateup_fp8": SG_GATEUP, "qkv_fp8": SG_QKV}
ENTRY_POINTS = tuple(EPS_OF)


def mode_of(c):
    if c["ep"] == "plain_fp8" and c.get("f32"):
        return SG_F32
    return EPS_OF[c["ep"]]


def form_of(c):
    """The kernel form a case reaches: ("sg", MT, WAVES, P, ks) | ("n8", MT, U) | ("f8", MT, WAVES)."""
    mode, M, N, K = mode_of(c), c["M"], c["N"], c["K"]
    if c["ep"].endswith("_n8"):
        return ("n8",) + pick_n8(mode, M, K)
    if c["ep"].endswith("_fp8"):
        return ("f8",) + fp8_form(mode, M, N, K)
    kn = knobs_of(c)
    MT, W, P = pick_form(mode, M, N, K, kn)
    return "sg", MT, W, P, pick_ks(N // 16, P, K >> 5, W, mode, kn)


# ---- cases -----------------------------------------------------------------------------------------------------------------
def case(ep, M, N, K, norm=False, knobs=(), **kw):
    """One case = one entry point at one shape, knob setting and set of fused options.  N: output columns of ONE weight stream
    (gate|up: the intermediate size; q|k|v: (H + 2 Hkv) D, from H / Hkv / D).  Options: resid, ss_out, ss_in (plain forms),
    f32 (plain_fp8), H / Hkv / D and rotate_k (rope forms), n8_off (a 16-row form at a shape the narrow-panel copy would take)."""
    c = dict(ep=ep, M=M, N=N, K=K, norm=norm, knobs=tuple(sorted(dict(knobs).items())))
    c.update(kw)
    if ep.startswith("qkv"):
        c.setdefault("Hkv", c["H"])
        assert N == (c["H"] + 2 * c["Hkv"]) * c["D"] and (ep == "qkvg") == (c["Hkv"] != c["H"])
    if ep.endswith("_n8"):
        assert norm and M <= 24 and K >= 1024 and K % 64 == 0, "the narrow-panel entries need a norm prologue, <= 24 rows, K >= 1024"
    if ep.endswith("_fp8"):
        assert K % 64 == 0
    assert not c.get("ss_in") or norm
    assert not (c.get("f32") or ep == "f32") or not (c.get("resid") or c.get("ss_out"))
    return c


def case_id(c):
    s = f"{c['ep']}-M{c['M']}-N{c['N']}-K{c['K']}" + ("-norm" if c["norm"] else "")
    for key in ("resid", "ss_out", "ss_in", "f32", "n8_off"):
        if c.get(key):
            s += f"-{key}"
    if c["ep"].startswith("qkv"):
        s += f"-H{c['H']}kv{c['Hkv']}D{c['D']}" + ("" if c.get("rotate_k", True) else "-norot")
    return s + "".join(f"-k{k}={v}" for k, v in c["knobs"])


def seed_of(c, kind):
    """One seed per case and kind, from its shape alone.  A seed that breaks a condition of test_gemm_probes_cpu is changed
    HERE (``SEED_BUMP``), never the condition."""
    s = 7919 * c["M"] + 31 * c["N"] + c["K"] + 1009 * ENTRY_POINTS.index(c["ep"]) + (500009 if kind == "dense" else 0) + (97 if c["norm"] else 0)
    return s + SEED_BUMP.get((case_id(c), kind), 0)


SEED_BUMP = {       # every entry: more than UNSAFE_CAP of the SwiGLU elements within DELTA of an fp16 boundary at seed + 0
    ("gateup_n8-M9-N16-K1024-norm-ss_in", "dense"): 1,        # 2 of 144
    ("gateup_n8-M16-N16-K1088-norm-ss_in", "dense"): 1,       # 4 of 256
    ("gateup_n8-M16-N48-K5120-norm", "dense"): 1,             # 8 of 768
    ("gateup_fp8-M17-N16-K64-norm", "dense"): 8,              # 14 of 272 (a short K: few distinct gate sums, each on many elements)
    ("gateup_fp8-M17-N16-K192-norm", "dense"): 17,            # 3 of 272
    ("gateup_fp8-M17-N16-K320-norm", "dense"): 6,             # 9 of 272
    ("gateup_fp8-M17-N16-K1088-norm", "dense"): 1,            # 3 of 272
    ("gateup_fp8-M8-N48-K192-norm-ss_in", "dense"): 7,        # 4 of 384
    ("gateup_fp8-M16-N48-K192-norm-ss_in", "dense"): 2,       # 12 of 768
    ("gateup_fp8-M32-N48-K192-norm-ss_in", "dense"): 14,      # 38 of 1536
}


def _rope(ep, M, H, Hkv, D, K, **kw):
    return case(ep, M, (H + 2 * Hkv) * D, K, H=H, Hkv=Hkv, D=D, **kw)


def _cases():
    out = []
    # -- tf_skinny_gemm_act, fp16 output: every K edge at one panel, both sides of the row-tile edge
    for K in (32, 64, 96, 160, 224, 512, 544):
        for M in (1, 17):
            out.append(case("plain", M, 16, K))
            out.append(case("plain", M, 16, K, norm=True))
    for M in (8, 9, 16, 24, 25, 32):
        out.append(case("plain", M, 48, 160, norm=(M % 2 == 0)))
        out.append(case("plain", M, 16, 544, norm=(M % 2 == 1)))
    out.append(case("plain", 32, 64, 11008))                                       # one long K
    for M in (1, 16, 17, 32):                                                      # fused options
        out.append(case("plain", M, 48, 224, resid=True, ss_out=True))
        out.append(case("plain", M, 32, 544, norm=True, resid=True, ss_out=True))
        out.append(case("plain", M, 48, 96, ss_out=True))
        out.append(case("plain", M, 16, 512, norm=True, ss_in=True, ss_out=True))
        out.append(case("plain", M, 32, 160, norm=True, ss_in=True, resid=True))
    # two panels per wave: key 2 = 1 lets the smallest even grid take it, key 0 moves the row threshold; 48 = odd: falls back
    for M in (1, 16, 17, 32):
        for N in (32, 48):
            out.append(case("plain", M, N, 512, knobs={2: 1}))
            out.append(case("plain", M, N, 544, norm=True, knobs={2: 1}, ss_out=True))
        out.append(case("plain", M, 32, 544, knobs={0: 17, 2: 1}, resid=True))
    # K split across workgroups, forced (key 4): the 8-wave form keeps 2 / 3 / 4 splits from 32 / 48 / 64 k-chunks
    for M, ksf, K in ((1, 2, 1056), (17, 2, 1024), (16, 3, 1568), (32, 3, 1536), (9, 4, 2080), (25, 4, 2048),
                      (8, 4, 1056), (17, 4, 1568), (1, 4, 544), (17, 1, 2048)):
        out.append(case("plain", M, 16, K, knobs={4: ksf}))
        out.append(case("plain", M, 48, K, norm=True, resid=True, ss_out=True, knobs={4: ksf}))
    out.append(case("plain", 17, 32, 1056, norm=True, ss_in=True, knobs={3: 200}))  # the rule's own split (key 3): 256 / 2 panels -> 4 -> 2
    # -- fp32 logits
    for M, N, K, norm in ((1, 16, 32, False), (17, 16, 96, True), (16, 48, 224, True), (32, 16, 544, False), (9, 32, 512, True)):
        out.append(case("f32", M, N, K, norm=norm))
    out.append(case("f32", 17, 32, 544, norm=True, knobs={2: 1}))
    out.append(case("f32", 16, 32, 512, knobs={2: 1, 4: 2}))                        # lm_head is never split
    # -- gate|up + SwiGLU
    for K in (32, 64, 96, 160, 224, 512, 544):
        for M in (1, 17):
            out.append(case("gateup", M, 16, K, norm=(K % 64 == 0)))
    for M in (8, 16, 24, 32):
        out.append(case("gateup", M, 48, 160, norm=True))
    for M in (16, 17, 32):
        out.append(case("gateup", M, 16, 1024, norm=True, n8_off=True))             # 8 waves at two row tiles (few-panel rule)
        out.append(case("gateup", M, 16, 1088, knobs={5: 0}))                       # key 5 = 0: back to 4 waves
        out.append(case("gateup", M, 32, 544, norm=True, knobs={2: 1}))             # two panels per wave
        out.append(case("gateup", M, 48, 512, knobs={2: 1}))
    for M, ksf, K in ((1, 2, 512), (16, 3, 800), (9, 4, 1056), (17, 4, 2080), (32, 2, 1056), (8, 4, 800), (17, 3, 1024)):
        out.append(case("gateup", M, 16, K, norm=(M % 2 == 1), knobs={4: ksf}, n8_off=True))
    # -- q|k|v + RoPE + append: the smallest head layouts at D = 64 and D = 128, one grouped-query
    for K in (32, 96, 160, 544):
        out.append(_rope("qkv", 1, 1, 1, 64, K, norm=(K != 96)))
        out.append(_rope("qkv", 17, 1, 1, 64, K, norm=(K == 96)))
    for M in (16, 32):
        out.append(_rope("qkv", M, 1, 1, 128, 224, norm=True))
        out.append(_rope("qkv", M, 2, 2, 64, 64, rotate_k=False))
    out.append(_rope("qkv", 17, 1, 1, 64, 512, knobs={2: 1}))
    out.append(_rope("qkv", 9, 1, 1, 128, 1056, norm=True, knobs={4: 2}, n8_off=True))
    out.append(_rope("qkv", 25, 1, 1, 64, 1568, knobs={4: 3}))
    for M, K, norm in ((1, 64, True), (16, 160, False), (17, 544, True), (32, 96, True)):
        out.append(_rope("qkvg", M, 2, 1, 64, K, norm=norm))
    out.append(_rope("qkvg", 8, 4, 2, 128, 224, norm=True))
    out.append(_rope("qkvg", 17, 2, 1, 64, 512, norm=True, knobs={2: 1}))
    out.append(_rope("qkvg", 24, 2, 1, 64, 2080, norm=True, knobs={4: 4}))
    # -- narrow panels: 16 / 17 super-chunks over 8 waves; K = 5120: batches of 5
    for M in (1, 8, 9, 16, 17, 24):
        K = 1024 if M % 2 else 1088
        out.append(case("gateup_n8", M, 16, K, norm=True, ss_in=(M > 8)))
        out.append(_rope("qkv_n8", M, 1, 1, 64, 2112 - K, norm=True, ss_in=(M <= 8)))
    for M in (8, 16, 24):
        out.append(case("gateup_n8", M, 48, 5120, norm=True))
        out.append(_rope("qkv_n8", M, 1, 1, 128, 5120, norm=True))
    # -- FP8 weights: 64-wide super-chunks; 8 waves from 16 of them
    for K in (64, 192, 320, 1024, 1088):
        for M in (1, 17):
            out.append(case("plain_fp8", M, 16, K, norm=(M == 1)))
            out.append(case("gateup_fp8", M, 16, K, norm=(M == 17)))
        out.append(_rope("qkv_fp8", 16 if K % 128 else 32, 1, 1, 64, K, norm=True))
    for M in (8, 16, 32):
        out.append(case("plain_fp8", M, 48, 1088, norm=True, resid=True, ss_out=True))
        out.append(case("plain_fp8", M, 32, 320, norm=True, ss_in=True, f32=True))
        out.append(case("gateup_fp8", M, 48, 192, norm=True, ss_in=True))
    out.append(_rope("qkv_fp8", 17, 1, 1, 128, 192))
    ids = [case_id(c) for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return out


CASES = _cases()
LAYOUTS = ("rows", "packed")
KINDS = ("select", "dense")

# what the case list must reach (tests/test_gemm_probes_cpu.py)
FORMS_REQUIRED = (
    [("sg", mt, w, 1, 1) for mt in (1, 2) for w in (4, 8)] + [("sg", mt, 4, 2, 1) for mt in (1, 2)]
    + [("sg", mt, 8, 1, ks) for mt in (1, 2) for ks in (2, 3, 4)] + [("sg", 1, 4, 1, ks) for ks in (2, 3, 4)]
    + [("n8", 1, 8), ("n8", 2, 8), ("n8", 2, 4), ("n8", 3, 4), ("n8", 3, 5), ("n8", 1, 5), ("n8", 2, 5)]
    + [("f8", mt, w) for mt in (1, 2) for w in (4, 8)])


# ---- material --------------------------------------------------------------------------------------------------------------
def edge_set(K):
    """E(K): 0 and K - 1; the first and last element of every 32-wide k-chunk (= of every half of a 64-wide super-chunk of the
    narrow-panel and FP8 packings); in the first and the last chunk the first and last element of every k-octet (offsets 0, 7,
    8, 15, 16, 23, 24, 31); and the first and last element of k-octets 0, 7, 8 and 31 counted from either end of the row."""
    e = {0, K - 1}
    for c in range(K // 32):
        e |= {32 * c, 32 * c + 31}
    for c0 in (0, K - 32):
        e |= {c0 + o for o in (0, 7, 8, 15, 16, 23, 24, 31)}
    for o in (0, 7, 8, 31):
        for oc in (o, K // 8 - 1 - o):
            if 0 <= oc < K // 8:
                e |= {8 * oc, 8 * oc + 7}
    return sorted(e)


def c_of_rows(M):
    """c_m of the norm-prologue probes: 2^(-1 + 7 m mod 17), 17 different powers of two from 0.5 to 32768."""
    return torch.tensor([2.0 ** (-1 + (7 * m) % 17) for m in range(M)], dtype=torch.float64)


def streams_of(c):
    return 2 if mode_of(c) == SG_GATEUP else 1


def step_of(c, kind):
    """The unit every dense partial sum is an integer multiple of (of the up / only stream; the gate stream's is 2^-5 of it)."""
    return 0.5 if (kind == "dense" and c["norm"]) else 1.0


def _randn16(n, g, floor, gate):
    """n randn fp16 values, |v| >= floor (a select weight of 2^-2 and an FP8 row scale of 2^-2 then leave every product a
    normal fp16 value).  ``gate``: values a SwiGLU gate may select — only those v for which silu(+-2^j v), j = -4 .. 4 (select
    weight x FP8 row scale), is boundary-safe: about 1.2 % of random fp16 values sit within DELTA of an fp16 boundary, more than
    UNSAFE_CAP allows, so the select probe draws around them (the dense probe's gate sums cannot be chosen: it keeps its share)."""
    out = torch.empty(0, dtype=torch.float16)
    while out.numel() < n:
        v = torch.randn(2 * n + 64, generator=g).half()
        v = torch.where(v.abs() < floor, torch.tensor(floor, dtype=torch.float16).copysign(v), v)
        if gate:
            ok = torch.ones(v.numel(), dtype=torch.bool)
            for j in range(-4, 5):
                for sgn in (1.0, -1.0):
                    ok &= silu_safe(v.double() * (sgn * 2.0 ** j))
            v = v[ok]
        out = torch.cat([out, v])
    return out[:n].clone()


def material(c, kind):
    """-> dict: x (M, K) fp16, ln (K,) fp16 | None, h (M, K) float64 (what the K loop multiplies: x, or the normalised rows),
    ws = one (streams * N, K) fp16 weight per launch (natural row order, gate rows first), ks = the selected k per launch
    ((streams * N,) int64, select only), scale (streams * N,) float64 (FP8: 2^(n % 5 - 2); else ones), res (M, N) fp16, ss_x
    (K / 16, M) float64 partial sums of x^2, cos / sin / pos of the rope forms."""
    M, N, K, S = c["M"], c["N"], c["K"], streams_of(c)
    g = torch.Generator().manual_seed(seed_of(c, kind))
    gate = S == 2
    sign = (torch.randint(0, 2, (M, K), generator=g) * 2 - 1).double()
    if c["norm"]:
        x = (sign * c_of_rows(M)[:, None]).half()
        if kind == "select":
            ln = _randn16(K, g, 2.0 ** -4, gate)
        else:
            ln = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (K,), generator=g)].half()
        h = sign * ln.double()[None, :]
    else:
        ln = None
        if kind == "select":
            x = _randn16(M * K, g, 2.0 ** -6, gate).view(M, K)
        else:
            x = sign.half()
        h = x.double()
    NT = S * N
    ws, ksel = [], []
    if kind == "select":
        E = edge_set(K)
        for lo in range(0, len(E), N):
            sl = torch.tensor(E[lo:lo + N])
            kk = torch.empty(NT, dtype=torch.int64)
            for s in range(S):                                   # every stream covers the slice, in an order of its own
                k_s = torch.randint(0, K, (N,), generator=g)
                k_s[torch.randperm(N, generator=g)[:len(sl)]] = sl
                kk[s * N:(s + 1) * N] = k_s
            wn = (torch.randint(0, 2, (NT,), generator=g) * 2 - 1).double() * 2.0 ** ((torch.arange(NT) % 5) - 2).double()
            w = torch.zeros(NT, K, dtype=torch.float64)
            w[torch.arange(NT), kk] = wn
            ws.append(w.half())
            ksel.append(kk)
    else:
        w = (torch.randint(0, 2, (NT, K), generator=g) * 2 - 1) * (torch.rand(NT, K, generator=g) < 0.25)
        w = w.double()
        if S == 2:
            w[:N] *= 2.0 ** -5                                   # gate: |g| <~ 7, silu exercised and not saturated
        ws.append(w.half())
    fp8 = c["ep"].endswith("_fp8")
    scale = 2.0 ** ((torch.arange(NT) % 5) - 2).double() if fp8 else torch.ones(NT, dtype=torch.float64)
    out = dict(x=x, ln=ln, h=h, ws=ws, ks=ksel, scale=scale, res=torch.randn(M, N, generator=g).half(),
               ss_x=x.double().square().view(M, K // 16, 16).sum(-1).t().contiguous())
    if c["ep"].startswith("qkv"):
        cos, sin = R.rope_tables_plain(c["D"], POS_MAX)
        out.update(cos=cos, sin=sin, pos=torch.randperm(POS_MAX, generator=g)[:M].contiguous())
    return out


def to_f16(v64):
    """float64 -> fp16, one rounding (through fp32 the rounding would be double; int-valued and short-significand inputs, all
    this file feeds but silu, are exact either way)."""
    h = v64.float().half()
    # repair a double rounding: where the fp32 step landed on an fp16 tie, a neighbour is strictly nearer in float64
    # (an exact float64 tie is an fp32 value: the direct cast already rounded it to even)
    for other in (_next16(h, +1), _next16(h, -1)):
        better = (v64 - other.double()).abs() < (v64 - h.double()).abs()
        h = torch.where(better, other, h)
    return h


def _next16(h, direction):
    """The fp16 neighbour of h away from / towards zero by bit pattern (finite, non-zero h; else h)."""
    bits = h.view(torch.int16).to(torch.int32) & 0xFFFF
    mag, sgn = bits & 0x7FFF, bits & 0x8000
    grow = (h.float() > 0) == (direction > 0)
    nm = torch.where(grow, mag + 1, mag - 1).clamp(0, 0x7BFF)
    flip = (mag == 0)                                            # +-0: the neighbour is the smallest subnormal of the direction's sign
    nb = torch.where(flip, torch.full_like(mag, 1 | (0x8000 if direction < 0 else 0)), nm | sgn)
    return nb.to(torch.int16).view(torch.float16)


def spacing16(h):
    """The fp16 spacing at |h| (2^-24 below the normal range)."""
    a = h.double().abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def silu64(g):
    g = g.double()
    return g / (1.0 + torch.exp(-g))


def silu_safe(g):
    """Boundary-safe gate values: fp16(silu64(g) (1 - DELTA)) == fp16(silu64(g) (1 + DELTA))."""
    s64 = silu64(g)
    return to_f16(s64 * (1 - DELTA)).view(torch.int16) == to_f16(s64 * (1 + DELTA)).view(torch.int16)


def expected(c, mat, li):
    """Expected outputs of launch ``li``, following the rounding points in the header of csrc/gemv.hip.  -> dict:
    acc (M, S N) float64 the exact K sums; y (M, S N) fp16 = fp16(scale * acc); plain forms: out (M, N) fp16 (fp32 for the
    logits), ss (N / 16, M) float64; gate|up: out, act, up, safe (bool), tol (float64); rope forms: q (M, H, D), k, v (M, Hkv, D)."""
    M, N = c["M"], c["N"]
    acc = mat["h"] @ mat["ws"][li].double().t()
    y64 = acc * mat["scale"][None, :]
    y = y64.half()
    e = dict(acc=acc, y=y, y_exact=bool(torch.equal(y.double(), y64)))
    mode = mode_of(c)
    if mode == SG_GATEUP:
        gt, up = y[:, :N], y[:, N:]
        s64 = silu64(gt)
        act = to_f16(s64)
        e.update(act=act, up=up, out=(act.float() * up.float()).half(),
                 safe=silu_safe(gt),
                 tol=up.double().abs() * spacing16(act))
    elif mode in (SG_QKV, SG_QKVG):
        H, Hkv, D = c["H"], c["Hkv"], c["D"]
        q, k, v = y[:, :H * D].view(M, H, D), y[:, H * D:(H + Hkv) * D].view(M, Hkv, D), y[:, (H + Hkv) * D:].view(M, Hkv, D)
        e.update(q=R.apply_rope(q, mat["cos"], mat["sin"], mat["pos"]),
                 k=R.apply_rope(k, mat["cos"], mat["sin"], mat["pos"]) if c.get("rotate_k", True) else k, v=v)
    else:
        out = y
        if c.get("resid"):
            out = (mat["res"].double() + y.double()).float().half()      # (an fp32 sum of two fp16 values rounds to fp16 innocuously)
        e["ss"] = out.double().square().view(M, N // 16, 16).sum(-1).t().contiguous()
        e["out"] = out.float() if (mode == SG_F32) else out
    return e


def ss_exact(c, kind):
    """Is ss_out owed bit for bit?  Only where every square and partial sum is an integer multiple of step^2 below 2^24: the
    dense probe on 16-bit weights without the residual add.  Elsewhere ss_out is asked for only with the residual (rtol 2e-6)."""
    return kind == "dense" and not c.get("resid") and not c["ep"].endswith("_fp8")


def wants_ss_out(c, kind):
    return bool(c.get("ss_out")) and (bool(c.get("resid")) or ss_exact(c, kind))
