"""One-hot and decoy probes for the attention kernels: inputs on which attention is a SELECTION.

Every (row, query head) picks one known key, so the expected output is that key's V row bit for bit; the hottest key of
all is then planted just where the row must not look.  Plain torch on the CPU, seeded; tests/test_attn_probes_cpu.py
proves the inputs on the oracle and tests/test_gpu_attn_probes.py feeds them to the kernels — both from the case lists
at the bottom of this file.

Material.  Keys are random sign vectors (+-1, exact in fp16 and in e4m3), V is randn fp16 (for the FP8 caches: the
dequantised image of randn rows).  ``needle``: q[i, h] = BETA * k[t[i, h], kvhead(h)], the target scores BETA * sqrt(D) nats
(90.5 at D = 128, 64 at D = 64), every other key about BETA * N(0, 1).  ``decoy``: one more key per decoyed row, GAIN * the
row's target key, at a position the row must not see (one past its causal edge — index sk, in the spare capacity, for the
last row —, the last row of the capacity, a non-ancestor tree column on either side of the row's own); it would score
GAIN * BETA * sqrt(D).  A planted key is visible to later rows, so a case decoys every other row counted from the last and
runs in both parities.  ``poison``: the spare rows [sk, cap) of K and V, planted decoys in K apart, hold NaN, +65504 or (FP8
caches) code 0x7F with exponent byte 0xFF.  ``sink``: randn q / k / v with key 0 raised to about half of every row's mass.
"""
import math

import torch

from oracle import ref_ops as R
from oracle import ref_tree as RT

BETA, GAIN = 8.0, 1.5
SPARE = 16                       # rows past sk at least: a whole 16-key tile and a part of a 64-key slab
LEAK_CAP = 2.0 ** -16            # condition (b)
DECOY_LEAD = 20.0                # condition (c), nats
SCORE_CAP = 256.0                # condition (d), nats
MODES = [("needle", 0, "nan"), ("decoy", 0, "inf"), ("decoy", 1, "nan")]       # kind, parity of the decoyed rows, poison
MODE_IDS = ["needle-nan", "decoy0-inf", "decoy1-nan"]


def case(ep, sq, sk, H=2, Hkv=None, D=128, nsplits=(None,), **kw):
    c = dict(ep=ep, sq=sq, sk=sk, H=H, Hkv=Hkv or H, D=D, nsplits=tuple(nsplits))
    c.update(kw)
    return c


def case_id(c):
    s = f"{c['ep']}-sq{c['sq']}-sk{c['sk']}-H{c['H']}" + (f"kv{c['Hkv']}" if c["Hkv"] != c["H"] else "") + f"-D{c['D']}"
    for key in ("n_tail", "T", "row0"):
        if key in c:
            s += f"-{key}{c[key]}"
    return s + ("-skdev" if c.get("skdev") else "")


def seed_of(c):
    """One seed per case, from its shape alone.  A seed that breaks a condition of test_attn_probes_cpu is changed HERE
    (``SEED_BUMP``), never the condition."""
    s = 7919 * c["sq"] + 31 * c["sk"] + 1009 * c["H"] + 97 * c["Hkv"] + c["D"] + 13 * c.get("n_tail", 0) + 17 * c.get("row0", 0)
    return s + SEED_BUMP.get(case_id(c), 0)


SEED_BUMP = {"prefill-sq300-sk4103-H2-D64": 1}      # seed + 0: a 13-nat runner-up moved one output by half an ulp


def scale_of(c):
    """The entry point's own scale: the tree path follows SDPA's 1 / sqrt(D), the chain path flash-attn's fp16-rounded one."""
    return 1.0 / math.sqrt(c["D"]) if c["ep"] == "tree" else R.softmax_scale_for(c["D"])


# ---- boundaries of a case: (label, key) pairs the targets must land on -------------------------------------------------------
def prefill_nsplit(H, sq, sk):
    """tf_attn_prefill_pick_nsplit restated (the GPU file asserts the two agree)."""
    nrb, slabs = (sq + 127) // 128, (sk + 63) // 64
    n = max(1, min(1024 // (H * nrb), slabs // 16, 128))
    while (H * n) % 8:
        n += 1
    return n


def split_edges(sk, nsplit, unit):
    """First keys of splits 1.. of a range of ceil(sk / unit) units dealt ceil(units / nsplit) to a split."""
    units = (sk + unit - 1) // unit
    per = (units + nsplit - 1) // nsplit
    return [s * per * unit for s in range(1, nsplit) if s * per * unit < sk]


def specials(c):
    ep, sq, sk = c["ep"], c["sq"], c["sk"]
    out = [("key0", 0), ("t15", 15), ("t16", 16), ("s63", 63), ("s64", 64)]
    if ep == "tree":
        p = c["prefix"]
        out += [(f"col{j}", p + j) for j in (31, 32, 63, 64)] + [("prefix_last", p - 1), ("tree_first", p)]
    unit, ns = 16, [n for n in c["nsplits"] if n]
    if ep in ("block", "tree") and sq > 64:
        unit = 64                                        # the LDS kernel deals 64-key slabs
    if ep in ("prefill", "prefill_gqa"):
        unit, ns = 64, [prefill_nsplit(c["H"], sq, sk)]
    for n in ns:
        for j, e in enumerate(split_edges(sk, n, unit)):
            out += [(f"split{n}.{j + 1}.last", e - 1), (f"split{n}.{j + 1}.first", e)]
    if ep == "fp8_tail":
        skc = sk - c["n_tail"]
        out += [("codes_last", skc - 1), ("codes_first_tail", skc)]
    seen, uniq = set(), []
    for lab, t in out:
        if 0 <= t < sk and lab not in seen:
            seen.add(lab)
            uniq.append((lab, t))
    return uniq


# ---- visibility ---------------------------------------------------------------------------------------------------------------
def tree_mask(T, seed):
    """(T, T) 0 / 1: row n = the ancestors of node n and n itself; parents drawn among n - 1, n - 3, n / 2 and the root."""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(T, T, dtype=torch.int64)
    m[0, 0] = 1
    for n in range(1, T):
        p = [n - 1, max(0, n - 3), n // 2, 0][int(torch.randint(0, 4, (1,), generator=g))]
        m[n] = m[p]
        m[n, n] = 1
    return m


def visibility(c, cap):
    """(sq, cap) bool: the keys a row may see (nothing at or past sk)."""
    sq, sk = c["sq"], c["sk"]
    vis = torch.zeros(sq, cap, dtype=torch.bool)
    if c["ep"] == "tree":
        p, r0 = c["prefix"], c["row0"]
        vis[:, :p] = True
        vis[:, p:sk] = c["mask"][r0:r0 + sq] != 0
    else:
        edge = sk - sq + torch.arange(sq).view(sq, 1)
        vis[:, :sk] = torch.arange(sk).view(1, sk) <= edge
    return vis


def edge_of(c, i):
    """The last key row i sees: its causal edge, or its own tree column."""
    return c["prefix"] + c["row0"] + i if c["ep"] == "tree" else c["sk"] - c["sq"] + i


# ---- the generators -----------------------------------------------------------------------------------------------------------
def _rope_inverse(x, cos, sin, pos):
    """x rotated by MINUS the angle of position pos (fp16): what rope-on-read turns back into about x."""
    return (x * cos[pos]) - (R.rotate_half(x) * sin[pos])


def build(c, kind="needle", parity=0, poison=None, quantize=None):
    """The inputs of one case.  Returns a dict: q (sq, H, D); k, v (cap, Hkv, D) as the kernel must understand them (FP8
    caches: the dequantised image); target (sq, H) long, -1 = a row with no free target (q = 0); decoys [(row, head, key)];
    vis (sq, cap); covered (labels the targets landed on); planted (keys holding a decoy)."""
    c = dict(c)
    ep, sq, sk, H, Hkv, D = c["ep"], c["sq"], c["sk"], c["H"], c["Hkv"], c["D"]
    g = H // Hkv
    seed = seed_of(c)
    if ep == "tree":
        c.setdefault("mask", tree_mask(c["T"], seed + 5))
    cap = sk + c.get("spare", SPARE)
    gk, gv, gt = (torch.Generator().manual_seed(seed + j) for j in (1, 2, 3))
    k = (torch.randint(0, 2, (cap, Hkv, D), generator=gk) * 2 - 1).to(torch.float16)
    v = torch.randn(cap, Hkv, D, generator=gv).to(torch.float16)
    if quantize is not None:
        v = quantize(v)[2]
    vis = visibility(c, cap)
    scale = scale_of(c)

    # 1. where the decoys go (positions first: no target may sit on one)
    decoyed = [i for i in range(sq) if kind == "decoy" and (sq - 1 - i) % 2 == parity]
    planted, spots = set(), {}                        # spots[row] = keys that will hold GAIN * the row's target
    for i in decoyed:
        if ep == "tree":                              # a free non-ancestor column below and one above the row's own: the
            own, lo, hi = edge_of(c, i), None, None   # first found, unless a mask-word edge (31 | 32, 63 | 64) is still free
            for t in range(c["prefix"], sk):
                if not vis[i, t] and t not in planted:
                    if t < own and (lo is None or t in (c["prefix"] + 31, c["prefix"] + 32)):
                        lo = t
                    if t > own and (hi is None or t in (c["prefix"] + 63, c["prefix"] + 64)):
                        hi = t
            spots[i] = [t for t in (lo, hi) if t is not None]
        else:
            spots[i] = [edge_of(c, i) + 1]
        planted.update(spots[i])
    if decoyed and ep != "tree":
        spots[decoyed[0]].append(cap - 1)             # a second decoy deep in the capacity
        planted.add(cap - 1)

    # 2. targets: uncovered boundaries first, then the row's own edge or the next boundary in turn, then any free key
    spec = specials(c)
    copied = [set() for _ in range(Hkv)]              # targets that a decoy repeats, per KV head

    def carrier(i, kv):
        return kv * g + decoyed.index(i) % g          # the one query head of a KV group whose target row i's decoys repeat

    covered, used, target = set(), [set() for _ in range(H)], torch.full((sq, H), -1, dtype=torch.long)
    for i in range(sq):
        in_row = set()
        for h in range(H):
            def free(t):
                return bool(vis[i, t]) and t not in used[h] and t not in in_row and t not in planted and t not in copied[h // g]
            turn = (i * H + h + seed) % len(spec)
            cands = [(lab, t) for lab, t in spec if lab not in covered]
            if (i + h) % 2 == 0 or "edge" not in covered:
                cands.append(("edge", edge_of(c, i)))
            cands += spec[turn:] + spec[:turn] + [("edge", edge_of(c, i))]
            pick = next(((lab, t) for lab, t in cands if free(t)), None)
            if pick is None:
                seen = vis[i].nonzero().flatten()
                for j in torch.randperm(len(seen), generator=gt)[:256].tolist():
                    if free(int(seen[j])):
                        pick = ("any", int(seen[j]))
                        break
            if pick is None:
                continue
            covered.add(pick[0])
            used[h].add(pick[1])
            if i in spots and h == carrier(i, h // g):
                copied[h // g].add(pick[1])          # its decoy is seen by the later rows of every query head of the group
            in_row.add(pick[1])
            target[i, h] = pick[1]

    # 3. decoys (one query head of a KV group per row, in turn), queries, poison
    decoys = []
    for i in decoyed:
        for kv in range(Hkv):
            h = carrier(i, kv)
            if target[i, h] >= 0:
                for f in spots[i]:
                    k[f, kv] = GAIN * k[target[i, h], kv]
                    decoys.append((i, h, f))
    kr = k
    if ep == "rope":
        cos, sin = R.rope_tables_plain(D, 2048)
        c["cos"], c["sin"] = cos, sin
        kr = R.apply_rope(k, cos, sin, torch.arange(cap))
        for i, h, f in decoys:                        # the cache holds UN-rotated keys: plant what rotates into the decoy
            k[f, h] = _rope_inverse(GAIN * kr[target[i, h], h], cos, sin, f)
        kr = R.apply_rope(k, cos, sin, torch.arange(cap))
    q = torch.zeros(sq, H, D, dtype=torch.float16)
    for i in range(sq):
        for h in range(H):
            if target[i, h] >= 0:
                q[i, h] = BETA * kr[target[i, h], h // g]
    keep = torch.zeros(cap, dtype=torch.bool)
    keep[:sk] = True
    bad = {None: None, "nan": float("nan"), "inf": 65504.0}[poison]
    if bad is not None:
        v[sk:] = bad
        for t in range(sk, cap):
            if t not in planted:
                k[t] = bad
    c.update(q=q, k=k, v=v, cap=cap, scale=scale, target=target, decoys=decoys, vis=vis, covered=covered, planted=planted,
             kind=kind, poison=poison, kvmap=torch.arange(H) // g)
    return c


def build_sink(c, quantize=None):
    """randn q / k / v, key 0 raised to about half of every row's mass: k[0] = gamma u, q += delta u with u a sign vector
    and delta * gamma * sqrt(D) = ln(sk) + (1 + delta^2) / 2, the log of the other keys' summed mass."""
    c = dict(c)
    sq, sk, H, Hkv, D = c["sq"], c["sk"], c["H"], c["Hkv"], c["D"]
    seed = seed_of(c) + 100
    if c["ep"] == "tree":
        c.setdefault("mask", tree_mask(c["T"], seed_of(c) + 5))
    cap = sk + SPARE
    gs = [torch.Generator().manual_seed(seed + j) for j in range(4)]
    q, k, v = torch.randn(sq, H, D, generator=gs[0]), torch.randn(cap, Hkv, D, generator=gs[1]), torch.randn(cap, Hkv, D, generator=gs[2])
    u = (torch.randint(0, 2, (Hkv, D), generator=gs[3]) * 2 - 1).float()
    delta = 2.0                                                  # (small gamma: key 0's share varies little from row to row)
    gamma = (math.log(sk) + (1 + delta * delta) / 2) / (delta * math.sqrt(D))
    k[0] = gamma * u
    q = q + delta * u[torch.arange(H) // (H // Hkv)]
    if quantize is not None:                                     # FP8 caches: the dequantised image is what the kernel reads
        k, v = quantize(k.half())[2], quantize(v.half())[2]
    c.update(q=q.half(), k=k.half(), v=v.half(), cap=cap, scale=scale_of(c), vis=visibility(c, cap), kind="sink", poison=None,
             target=torch.full((sq, H), -1, dtype=torch.long), decoys=[], planted=set(), kvmap=torch.arange(H) // (H // Hkv))
    if c["ep"] == "rope":
        c["cos"], c["sin"] = R.rope_tables_plain(D, 2048)
    return c


# ---- the oracle, and a plain masked attention the mutants are made from --------------------------------------------------------
def oracle(inp):
    """(sq, H * D) fp16 from the project's oracle of the entry point, on the keys below sk alone."""
    sk, g = inp["sk"], inp["H"] // inp["Hkv"]
    q, k, v = inp["q"], inp["k"][:sk], inp["v"][:sk]
    if g > 1:
        k, v = k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1)
    if inp["ep"] == "tree":
        add = RT.additive_tree_mask(inp["vis"][:, :sk].to(torch.int64)).float()
        return RT.attn_sdpa(q, k, v, add).reshape(inp["sq"], -1)
    if inp["ep"] == "rope":
        k = R.apply_rope(k, inp["cos"], inp["sin"], torch.arange(sk))
    return R.attn_kvcache(q, k, v, inp["scale"]).reshape(inp["sq"], -1)


def masked_attn(inp, vis=None, kvmap=None, n=None, twice=None):
    """fp32 softmax attention over keys [0, n) under a visibility matrix and a query-head -> KV-head map: the oracle when
    called with the defaults, a mutant otherwise.  ``twice``: a (first, last) key range counted twice."""
    vis = inp["vis"] if vis is None else vis
    kvmap = inp["kvmap"] if kvmap is None else kvmap
    n = inp["sk"] if n is None else n
    k, v = inp["k"][:n], inp["v"][:n]
    if inp["ep"] == "rope":
        k = R.apply_rope(k, inp["cos"], inp["sin"], torch.arange(n))
    s = torch.einsum("ihd,thd->hit", inp["q"].float(), k.float()[:, kvmap]) * float(inp["scale"])
    s = s.masked_fill(~vis[None, :, :n], float("-inf"))
    m = s.amax(dim=-1, keepdim=True)
    p = torch.exp(s - m)
    if twice is not None:
        p[:, :, twice[0]:twice[1]] *= 2
    o = torch.einsum("hit,thd->ihd", p / p.sum(dim=-1, keepdim=True), v.float()[:, kvmap])
    return o.to(torch.float16).reshape(inp["sq"], -1)


def conditions(inp):
    """The figures of conditions (b) to (d): the largest summed leak exp(s - s_target) over a row's other visible keys, the
    smallest lead of a decoy over its row's target, the largest |score| over every finite key of the capacity."""
    cap, D = inp["cap"], inp["D"]
    k = inp["k"].double().nan_to_num(0.0)
    if inp["ep"] == "rope":
        k = R.apply_rope(inp["k"].nan_to_num(0.0), inp["cos"], inp["sin"], torch.arange(cap)).double()
    s = torch.einsum("ihd,thd->iht", inp["q"].double(), k[:, inp["kvmap"]]) * float(inp["scale"])     # (sq, H, cap)
    finite = torch.isfinite(inp["k"].float()).all(dim=-1).all(dim=-1) & (inp["k"].float().abs().amax(dim=(1, 2)) < 100)
    s[:, :, ~finite] = 0.0                                       # poisoned rows of the capacity: never visible, no score
    tgt = inp["target"]
    has = tgt >= 0
    st = torch.gather(s, 2, tgt.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    e = torch.exp(s - st.unsqueeze(-1)) * inp["vis"].unsqueeze(1)
    leak = e.sum(dim=-1) - 1.0                                   # the target's own term is exp(0)
    lead = min([float(s[i, h, f] - st[i, h]) for i, h, f in inp["decoys"]], default=float("inf"))
    gap = st.unsqueeze(-1) - s.masked_fill(~inp["vis"].unsqueeze(1), float("-inf")).scatter(
        2, tgt.clamp(min=0).unsqueeze(-1), float("-inf"))
    return dict(leak=float(leak[has].max()) if bool(has.any()) else 0.0, lead=lead,
                max_score=float(s[:, :, finite].abs().max()),
                gap=float(gap[has].min()) if bool(has.any()) else float("inf"))


# ---- the check ----------------------------------------------------------------------------------------------------------------
def nearest_key(inp, row):
    """(key, KV head) of the V row of the whole capacity nearest to one output row (max-norm, poison rows as they are)."""
    v = inp["v"].float().nan_to_num(nan=1e9, posinf=1e9, neginf=-1e9)
    d = (v - row.float().view(1, 1, -1)).abs().amax(dim=-1)      # (cap, Hkv)
    j = int(d.argmin())
    return j // d.shape[1], j % d.shape[1]


def diagnose(inp, out):
    """The first probed (row, head) whose output is not its target's V row, as text; None when all are."""
    sq, H, D = inp["sq"], inp["H"], inp["D"]
    o = out.reshape(sq, H, D)
    for i in range(sq):
        for h in range(H):
            t = int(inp["target"][i, h])
            if t >= 0 and not torch.equal(o[i, h], inp["v"][t, int(inp["kvmap"][h])]):
                key, kv = nearest_key(inp, o[i, h])
                d = float((o[i, h].float() - inp["v"][t, int(inp["kvmap"][h])].float()).abs().max())
                return (f"row {i} head {h}: expected V row of key {t} (KV head {int(inp['kvmap'][h])}), off by {d:.3e}; "
                        f"the output is nearest to the V row of key {key} (KV head {kv}); sk {inp['sk']}, cap {inp['cap']}, "
                        f"edge {edge_of(inp, i)}")
    return None


def check(inp, out, want, atol, rtol, close, what="", exact=True):
    """The assertions of one launch, in order: 1. finite; 2. the entry point's own tolerance against the oracle on all rows
    (``close`` = tests.helpers.close, so the parity table gets its row); 3. bit equality with the target's V row on every
    probed row.  4. Whatever fails, the message names the first wrong (row, head), its key and the key it landed on."""
    out = out.detach().cpu()
    bad = ~torch.isfinite(out.float())
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} NaN / Inf outputs, first in row {int(bad.any(dim=1).nonzero()[0])} "
                                 f"(poison {inp['poison']}: a row past sk = {inp['sk']} was read)")
    try:
        close(out.float().reshape(inp["sq"], -1), want.float().reshape(inp["sq"], -1), what=what, atol=atol, rtol=rtol)
    except AssertionError as e:
        raise AssertionError(f"{what}: {diagnose(inp, out) or 'no probed row is wrong'}\n{e}") from None
    if exact:
        msg = diagnose(inp, out)
        assert msg is None, f"{what}: {msg}"


# ---- the mutants: what a subtly wrong kernel would compute -------------------------------------------------------------------
def mutants(inp):
    """name -> (sq, H * D) output of a wrong attention on these inputs; only the mutants that apply to the case."""
    vis, sk, cap, sq = inp["vis"], inp["sk"], inp["cap"], inp["sq"]
    out = {}
    wide = vis.clone()
    wide[:, 1:] |= vis[:, :-1]
    if inp["ep"] != "tree":
        out["mask_one_wider"] = lambda: masked_attn(inp, vis=wide, n=sk + 1)
        narrow = vis.clone()
        narrow[:, :-1] &= vis[:, 1:]
        if sk > sq:                                           # (sk == sq: row 0 would see nothing)
            out["mask_one_narrower"] = lambda: masked_attn(inp, vis=narrow)
        last = vis.clone()
        last[sq - 1, sk] = True
        out["key_sk_read"] = lambda: masked_attn(inp, vis=last, n=sk + 1)
    if inp["poison"] == "nan":                                # P = 0 times a V row past sk: the clamp left out
        out["pv_past_sk"] = lambda: masked_attn(inp, n=sk + 1)
    for lab, t in specials(inp):
        drop = vis.clone()
        drop[:, t] = False
        if bool(vis[:, t].any()) and bool(drop.any(dim=1).all()):                  # (never a row left with no key)
            name = lab.split(".")[-1] if lab.startswith("split") else lab           # a split's "first" / "last" key
            out[f"drop_{name}"] = lambda d=drop: masked_attn(inp, vis=d)
    if sk >= 48:
        tile = vis.clone()
        tile[:, 16:32] = False
        out["tile_dropped"] = lambda: masked_attn(inp, vis=tile)
        out["tile_twice"] = lambda: masked_attn(inp, twice=(0, 16))
    if inp["Hkv"] > 1 and inp["Hkv"] < inp["H"]:
        out["head_mod_hkv"] = lambda: masked_attn(inp, kvmap=torch.arange(inp["H"]) % inp["Hkv"])
    if inp["ep"] == "tree":
        p = inp["prefix"]
        for name, sh in (("tree_bit_plus_one", 1), ("tree_bit_minus_one", -1)):
            off = vis.clone()
            off[:, p:sk] = torch.roll(vis[:, p:sk], sh, dims=1)
            out[name] = lambda o=off: masked_attn(inp, vis=o)
    return out


# ---- the cases: one list per entry point, shared by the CPU and the GPU file ---------------------------------------------------
def _decode_cases():
    out = []
    for D in (128, 64):
        for sq in (1, 7, 16, 17, 32):
            for sk in (sq, 33, 333, 4103):
                if sk >= sq:
                    tiles = (sk + 15) // 16
                    ns = [n for n in (1, 3, 8) if n <= tiles] + [None]
                    out.append(case("decode", sq, sk, D=D, nsplits=ns, skdev=(sq in (7, 17) and sk == 333)))
    out.append(case("decode", 17, 12305, nsplits=(1, 8, None)))
    return out


CASES = {
    "decode": _decode_cases(),
    "decode_gqa": [case("decode_gqa", sq, sk, H=H, Hkv=Hkv, D=D, nsplits=(1, 3, None))
                   for (H, Hkv, sq) in ((4, 1, 7), (8, 2, 7), (8, 1, 7), (2, 1, 17)) for sk in (333, 4103) for D in (128, 64)],
    "fp8": [case("fp8", sq, sk, nsplits=(1, 3, None)) for sq in (7, 17) for sk in (333, 4103)],
    "fp8_tail": [case("fp8_tail", sq, sk, nsplits=(1, 3, None), n_tail=nt)
                 for sq in (7, 17) for sk in (333, 4103) for nt in (1, 7, 17)],
    "block": [case("block", sq, sk, D=D, nsplits=[n for n in (1, 3) if n <= (sk + 63) // 64] + [None])
              for D in (128, 64) for sq in (32, 33, 64, 65, 128) for sk in (sq, sq + 1, 640, 4103)],
    "prefill": [case("prefill", sq, sk, D=D) for D in (128, 64) for sq in (129, 300) for sk in (sq, sq + 77, 4103)],
    "prefill_gqa": [case("prefill_gqa", sq, sk, H=H, Hkv=Hkv, D=D)
                    for (H, Hkv) in ((4, 2), (8, 1)) for sq in (33, 129) for sk in (sq + 77, 4103) for D in (128, 64)],
    "tree": [case("tree", sq, 300 + T, D=D, T=T, row0=row0, prefix=300, nsplits=((None,) if sq > 128 else (1, 3, None)))
             for D in (128, 64) for (T, row0, sq) in ((40, 0, 40), (40, 5, 35), (130, 0, 130), (130, 2, 128))],
    "rope": [case("rope", sq, kv, H=H, D=64) for kv in (5, 259, 384, 400) for (sq, H) in ((1, 2), (9, 12), (64, 3)) if sq <= kv],
}
SINK_CASES = [case("decode", 7, 4103, nsplits=(1, 8, None)), case("decode", 17, 333, D=64, nsplits=(3,)),
              case("decode_gqa", 7, 4103, H=8, Hkv=2, nsplits=(3, None)),
              case("fp8", 7, 4103, nsplits=(3,)), case("fp8_tail", 17, 4103, nsplits=(3,), n_tail=17),
              case("block", 65, 4103, nsplits=(3, None)), case("block", 33, 640, D=64, nsplits=(1, 3)),
              case("prefill", 300, 4103), case("prefill_gqa", 129, 4103, H=4, Hkv=2),
              case("tree", 130, 430, T=130, row0=0, prefix=300), case("rope", 9, 259, H=12, D=64), case("rope", 5, 400, D=64)]
ALL_CASES = [c for ep in CASES for c in CASES[ep]]
