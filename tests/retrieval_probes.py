"""Exact probes for the retrieval build and the KV row moves (csrc/retrieval.hip): material on which every score is a
statement about integers, every top-k order is a plain Python sort and every moved row carries its own address, so that each
comparison is ``torch.equal`` or ``==``.  CPU only, seeded; tests/test_retrieval_probes_cpu.py proves the material, its
conditions and the case list against the oracle (oracle/ref_ops.py) and tests/cpu_backend.py, and the restated launch rules
against csrc/retrieval_rule.h; tests/test_gpu_retrieval_probes.py feeds the same cases to the kernels.  No kernel output
ever produces an expectation, and nothing here has a tolerance.

Scores.  ONE-HOT rows: q[h] is zero but for q[h, d_h] = +-2^j, K holds an address code (an integer, 1 <= |x| <= 2048, that
differs from its neighbours at c +- 1, c +- step and h +- 1) at [h, rows of chunk c, d_h] and small non-zero integer decoys
everywhere else: the expected score is q_val * code exactly, whatever the chunk (a power of two here; every row of a chunk
holds the chunk's code, so the mean is the code).  DENSE rows: q in {-1, 0, 1} with at most 16 non-zeros, K integers in
[-8, 8], chunk a power of two: every sum, mean and dot is a multiple of 1 / chunk of at most 2048 units, exact in fp32 in
any order and exact in fp16.  Chunks that are no power of two stay with tests/rounding_probes.py.

Top-k.  The expectation is ``topk_expected``: candidates 1 .. C - 1 sorted by (fp16 BIT-PATTERN order descending, chunk
ascending), chunk 0 prepended.  Bit-pattern order is sign-magnitude: -0 sits just below +0, +NaN above +inf; "tie" means
equal bit patterns, so a (+0, -0) pair is NOT a tie (it is one for torch.topk, whose order among IEEE-equal scores is
unspecified: either answer is admissible against the reference).  -NaN is left out of every row: the kernel sorts it last,
torch.topk sorts it first, and neither is claimed.
The planted rows put the m-th key (m = sets - 1, the radix select's threshold) into the end bins of the select's 8-bit
passes.  The key is sortable(score) << 16 | (65535 - chunk), so pass 0 reads the score field's high byte, pass 1 its low
byte, passes 2 and 3 the chunk field.  ``chunk255`` / ``chunk0``: the m-th key's chunk = 255 / 0 (mod 256) inside a run of
equal scores - bins 0 / 255 of pass 3.  ``lo00`` / ``loFF``: the score field's low byte 0x00 / 0xFF with neighbours that
share its high byte - bins 0 / 255 of pass 1.  ``hi00``: the SCORE's high byte 0x00 (a positive subnormal; the key field's
high byte 0x00 would need -NaN).  ``hiFF``: the key field's high byte 0xFF, which only +NaN reaches - bin 255 of pass 0.
Pass 2 (the chunk field's high byte) has bin 255 whenever the m-th chunk is below 256, and nothing below bin 0x80.

Row moves and gathers carry address codes: the value at (tensor, l, h, t, d) is an integer of at most 2047 that names its
place; destinations are pre-filled with SENTINEL (no integer) and have guard rows, and every row a call must not touch is
asserted unchanged.

The launch rules of csrc/retrieval_rule.h are restated (``topk_pick``, ``chunk_grid_x``, ``copy_grid_x``) to label every
case with the (kernel, path) pairs it reaches; REQUIRED lists the labels the case list must reach.
"""
import ctypes
import functools

import torch

HALF = torch.float16
SENTINEL = -0.62353515625            # an fp16 value that is no integer: no address code equals it
EINVAL, ERANGE = -22, -34


# ---- the launch rules, restated (csrc/retrieval_rule.h) ---------------------------------------------------------------------
def topk_pick(C, sets):
    mpow2 = 2
    while mpow2 < sets - 1:
        mpow2 *= 2
    lds_sel = (C - 1 + mpow2) * 4
    if lds_sel <= 150 * 1024 and mpow2 <= 8192:
        return dict(form="select", lds=lds_sel, mpow2=mpow2, npow2=0, raised=lds_sel > 48 * 1024)
    npow2 = 2
    while npow2 < C - 1:
        npow2 *= 2
    return dict(form="full", lds=npow2 * 4, mpow2=mpow2, npow2=npow2, raised=npow2 * 4 > 64 * 1024)


def gpb_of(D):
    return 256 // (D // 8)


def chunk_grid_x(n, H, D):
    gx = (n + gpb_of(D) - 1) // gpb_of(D)
    cap = 2048 // H if H <= 2048 else 1
    return max(1, min(gx, cap))


def copy_grid_x(n, D):
    return min(64, (n * (D // 8) + 255) // 256)


def rows_per_blk(D):
    return 256 // (D // 8)


# ---- layouts ------------------------------------------------------------------------------------------------------------------
def place(x, layout, device="cpu", fill=SENTINEL):
    """x (..., T, D) with leading dims (H,) or (L, H) as a view of the given layout on ``device``: "head" contiguous,
    "token" a permuted view of a token-major buffer, "pad" rows [3, 3 + T) of a longer sentinel-filled buffer (padded head
    stride).  -> (view, base buffer)."""
    x = x.to(device)
    if layout == "head":
        base = x.clone().contiguous()
        return base, base
    lead = x.dim() - 2
    if layout == "token":
        perm = (0, 2, 1, 3) if lead == 2 else (1, 0, 2)             # (L, T, H, D) | (T, H, D)
        base = x.permute(*perm).contiguous()
        return base.permute(*perm), base
    assert layout == "pad"
    shape = list(x.shape)
    shape[-2] += 8
    base = torch.full(shape, fill, dtype=x.dtype, device=device)
    view = base[..., 3:3 + x.shape[-2], :]
    view.copy_(x)
    return view, base


# =================================================================================================================================
# scores
# =================================================================================================================================
SCORE_KINDS = ("onehot", "dense")
STRIDE_H = 256                        # grid cap 2048 / 256 = 8 workgroups: step = 8 * GPB chunks


def _score_cases():
    cases = []
    chunks = (1, 2, 8, 16)
    i = 0
    for D in (64, 128):
        g = gpb_of(D)
        for H in (1, 3, 32):
            for C in (1, g - 1, g, g + 1):
                cases.append(dict(H=H, D=D, C=C, chunk=chunks[i % 4], layout="head"))
                i += 1
        step = 8 * g
        for j in (1, 2, 4):
            for o in (-1, 0, 1):
                cases.append(dict(H=STRIDE_H, D=D, C=step * j + o, chunk=2 if j == 1 else 1, layout="head"))
        cases.append(dict(H=STRIDE_H, D=D, C=4 * step + step // 2, chunk=2, layout="head"))
        cases.append(dict(H=STRIDE_H, D=D, C=1029, chunk=1, layout="head"))
    # one token-major K and one padded head stride, small and strided
    for c in cases:
        key = (c["H"], c["D"], c["C"])
        if key in ((3, 128, 17), (STRIDE_H, 64, 257)):
            c["layout"] = "token"
        if key in ((32, 64, 33), (STRIDE_H, 128, 255)):
            c["layout"] = "pad"
    return cases


SCORE_CASES = _score_cases()


def score_id(c):
    return f"H{c['H']}-D{c['D']}-C{c['C']}-chunk{c['chunk']}-{c['layout']}"


def score_step(c):
    """Chunks between two trips of a group: grid x GPB (the indexed scorer walks 4 of them per trip)."""
    return chunk_grid_x(c["C"], c["H"], c["D"]) * gpb_of(c["D"])


def pieces_of(c):
    """(0, a), (a, b), (b, C) with a and b off the GPB grid wherever C leaves room."""
    C, g = c["C"], gpb_of(c["D"])
    a, b = C // 3, min(C, 2 * C // 3 + 1)
    if a and a % g == 0:
        a += 1
    if b % g == 0 and b < C:
        b += 1
    a = min(a, b)
    return ((0, a), (a, b), (b, C))


def score_labels(c):
    C, H, D = c["C"], c["H"], c["D"]
    step = score_step(c)
    out = set()
    for kern in ("score", "chunk_mean"):
        out.add((kern, "stride" if C > step else "single_trip"))
    out.add(("chunk_mean", "pieces"))
    for c0, c1 in pieces_of(c):
        if c1 - c0 > chunk_grid_x(c1 - c0, H, D) * gpb_of(D):
            out.add(("chunk_mean", "piece_stride"))
        if c0 % gpb_of(D):
            out.add(("chunk_mean", "piece_off_grid"))
    trips = (C + 4 * step - 1) // (4 * step)
    rem = C - (trips - 1) * 4 * step
    out.add(("score_indexed", f"u{min(4, (rem + step - 1) // step)}"))
    if rem % step:
        out.add(("score_indexed", "partial_tail"))
    if trips > 1:
        out.add(("score_indexed", "second_trip"))
    for kern in ("score", "chunk_mean", "score_indexed"):
        out.add((kern, f"D{D}"))
    if c["layout"] != "head":
        out.add(("score", f"layout_{c['layout']}"))
    return out


def code_of(h, c, step):
    """Address code of (head, chunk): an integer, 1 <= |x| <= 2048 (int64 tensors broadcast)."""
    x = (c * 37 + (c // step) * 101 + h * 211) % 4095 - 2047
    return x + (x >= 0).to(x.dtype)


def d_of(h, D):
    return (h * 37 + 5) % D


def q_val_of(h):
    return (-1.0 if h % 2 else 1.0) * 2.0 ** (h % 7 - 2)


@functools.lru_cache(maxsize=None)
def _decoy_base(D, dense):
    gen = torch.Generator().manual_seed(4100 + D + int(dense))
    if dense:
        return torch.randint(-8, 9, (STRIDE_H, 2304, D), generator=gen, dtype=torch.int8)
    x = torch.randint(-100, 101, (STRIDE_H, 2304, D), generator=gen, dtype=torch.int8)
    return torch.where(x == 0, torch.ones_like(x), x)


def score_material(c, kind):
    """-> dict(k (H, T, D) fp16 head-major contiguous, q (H, D) fp16, want (H, C) fp16, index (H, C, D) fp16 the exact chunk
    means; one-hot: codes (H, C) int64, d (H,) int64)."""
    H, D, C, chunk = c["H"], c["D"], c["C"], c["chunk"]
    T = C * chunk
    k = _decoy_base(D, kind == "dense")[:H, :T].to(HALF)
    hs = torch.arange(H)
    mat = {}
    if kind == "onehot":
        codes = code_of(hs[:, None], torch.arange(C)[None, :], score_step(c))
        d = d_of(hs, D)
        k[hs[:, None], torch.arange(T)[None, :], d[:, None]] = codes.repeat_interleave(chunk, dim=1).to(HALF)
        q = torch.zeros(H, D, dtype=HALF)
        qv = torch.tensor([q_val_of(h) for h in range(H)], dtype=torch.float64)
        q[hs, d] = qv.to(HALF)
        want = qv[:, None] * codes.double()
        mat.update(codes=codes, d=d)
    else:
        gen = torch.Generator().manual_seed(977 * C + D + H)
        q = torch.zeros(H, D, dtype=HALF)
        for h in range(H):
            nz = torch.randperm(D, generator=gen)[:1 + (h % 16)]
            q[h, nz] = (torch.randint(0, 2, (nz.numel(),), generator=gen) * 2 - 1).to(HALF)
        means = k.double().view(H, C, chunk, D).mean(dim=2)
        want = (q.double()[:, None, :] * means).sum(dim=-1)
    index = k.double().view(H, C, chunk, D).mean(dim=2)
    mat.update(k=k, q=q, want64=want, want=want.to(HALF), index64=index, index=index.to(HALF))
    return mat


# =================================================================================================================================
# top-k
# =================================================================================================================================
# In launch order.  The raised-LDS attribute of a top-k kernel is set once per process, so within each form every shape that
# launches un-raised stands before the first one that raises it (asserted on the CPU): the 48 KiB select edge and the 64 KiB
# full sorts run un-raised when this list is walked in a fresh process.
TOPK_SHAPES = ((2, 1), (2, 2), (9, 1), (9, 2), (9, 3), (9, 9), (12033, 257), (8200, 8195), (16385, 8194), (12034, 257),
               (30209, 8193), (30210, 8193), (32768, 4097), (32768, 4098), (32768, 32768), (16386, 8194), (20000, 10000))
TOPK_KINDS = ("all_equal", "tie_inside", "tie_first", "tie_last", "sweep", "one_nan", "coarse", "chunk255", "chunk0", "hi00",
              "hiFF", "lo00", "loFF")
TOPK_H = 3
POS_NAN = 0x7E00


def order_of_bits(b):
    """Sign-magnitude order of an fp16 bit pattern as an integer: +0 -> 0, -0 -> -1, +NaN above +inf."""
    mag = b & 0x7FFF
    return -1 - mag if b & 0x8000 else mag


def topk_expected(bits, sets):
    """bits: the C fp16 bit patterns of one head (ints) -> the ``sets`` chunk ids."""
    order = sorted(range(1, len(bits)), key=lambda c: (-order_of_bits(bits[c]), c))
    return [0] + order[:sets - 1]


def _bits_of(x):
    return [v & 0xFFFF for v in x.to(HALF).view(torch.int16).tolist()]


def _coarse(C, gen):
    return _bits_of((torch.randn(C, generator=gen) * 4).round() / 4)


def _sweep_values():
    vals = [0x7C00, 0xFC00]
    for sign in (0, 0x8000):
        for e in range(31):
            for mant in (0, 1, 0x155, 0x3FF):
                vals.append(sign | (e << 10) | mant)
    return vals


def _planted(C, m, gen, star, above, below, star_chunk=None):
    """m - 1 candidates from ``above`` (bit patterns that sort above ``star``), one ``star``, the rest from ``below``."""
    n = C - 1
    perm = (torch.randperm(n, generator=gen) + 1).tolist()
    if star_chunk is not None:
        perm.remove(star_chunk)
        perm.insert(m - 1, star_chunk)
    bits = [0] * C
    for i, ch in enumerate(perm):
        src = above if i < m - 1 else below
        bits[ch] = star if i == m - 1 else src[i % len(src)]
    return bits


def _chunk_planted(C, m, gen, residue):
    """A run of equal scores around chunk c* = residue (mod 256), with the m-th place ON c*: m - p candidates outside the run
    score higher (p = c*'s place inside the run), every other one lower.  None when [1, C) has no such chunk."""
    n = C - 1
    cands = [ch for ch in range(1, C) if ch % 256 == residue]
    if not cands:
        return None
    cstar = cands[len(cands) // 2]
    before = min(3, m - 1, cstar - 1)
    after = min(3, n - m, n - cstar)
    run = set(range(cstar - before, cstar + after + 1))
    rest = [ch for ch in (torch.randperm(n, generator=gen) + 1).tolist() if ch not in run]
    hi = m - (before + 1)
    if hi > len(rest):
        return None
    bits = [0] * C
    for ch in run:
        bits[ch] = 0x3C00
    for i, ch in enumerate(rest):
        bits[ch] = (0x4000 + i % 3) if i < hi else (0x3800 - i % 3)
    return bits


def topk_row(C, sets, kind, seed):
    """-> (C fp16 bit patterns as ints, the kind actually built: shapes too small for a planted kind fall back to "coarse")."""
    gen = torch.Generator().manual_seed(seed)
    n, m = C - 1, max(1, sets - 1)
    bits = None
    if kind == "all_equal":
        bits = [0x3E00] * C
    elif kind in ("tie_inside", "tie_first", "tie_last"):
        n_hi = {"tie_inside": m // 2, "tie_first": m - 1, "tie_last": m}[kind]
        if kind == "tie_inside" and not (n_hi < m < n):                     # the m-th place must have neighbours in the run
            kind = "coarse"
        else:
            perm = (torch.randperm(n, generator=gen) + 1).tolist()
            bits = [0] * C
            for i, ch in enumerate(perm):
                bits[ch] = 0x4100 if i < n_hi else 0xB800
    elif kind == "sweep":
        vals = _sweep_values()
        order = torch.randperm(len(vals), generator=gen).tolist()
        bits = [vals[order[i % len(vals)]] for i in range(C)]
        if n < len(vals):
            kind = "sweep_part"
    elif kind == "one_nan":
        bits = _coarse(C, gen)
        bits[1 + int(torch.randint(0, n, (1,), generator=gen))] = POS_NAN
    elif kind in ("chunk255", "chunk0"):
        bits = _chunk_planted(C, m, gen, 255 if kind == "chunk255" else 0)
    elif kind == "lo00":
        bits = _planted(C, m, gen, 0x3C00, [0x3C01, 0x3C02, 0x3CFF], [0x3BFF, 0x3BFE, 0x3800])
    elif kind == "loFF":
        bits = _planted(C, m, gen, 0x3BFF, [0x3C00, 0x3C01, 0x4000], [0x3BFE, 0x3B00, 0x3BFD])
    elif kind == "hi00":
        bits = _planted(C, m, gen, 0x0080, [0x0081, 0x00FF, 0x3C00], [0x007F, 0x0000, 0x8001])
    elif kind == "hiFF":
        bits = _planted(C, m, gen, 0x7F00, [0x7FFF, 0x7F01], [0x7C00, 0x7BFF, 0x3C00])
    if bits is None:
        kind, bits = "coarse", _coarse(C, gen)
    bits[0] = 0xFC00 if seed % 2 else 0x7C00                                  # chunk 0 is no candidate: -inf or +inf there
    return bits, kind


@functools.lru_cache(maxsize=None)
def topk_case(i):
    """-> dict(C, sets, pick, kinds, bits (H lists of ints), scores (H, C) fp16, want (H lists))."""
    C, sets = TOPK_SHAPES[i]
    pick = topk_pick(C, sets)
    first = sum(TOPK_H for j in range(i) if topk_pick(*TOPK_SHAPES[j])["form"] == pick["form"])   # rows of this form so far
    rows, kinds = [], []
    for r in range(TOPK_H):
        bits, kind = topk_row(C, sets, TOPK_KINDS[(first + r + (9 if pick["form"] == "select" else 0)) % len(TOPK_KINDS)], 100 * i + r)
        rows.append(bits)
        kinds.append(kind)
    scores = ((torch.tensor(rows, dtype=torch.int32) + 32768) % 65536 - 32768).to(torch.int16).view(HALF)
    return dict(C=C, sets=sets, pick=pick, kinds=kinds, bits=rows, scores=scores, want=[topk_expected(b, sets) for b in rows])


def topk_id(i):
    C, sets = TOPK_SHAPES[i]
    p = topk_pick(C, sets)
    return f"C{C}-sets{sets}-{p['form']}-{p['lds'] // 1024}K{'-raised' if p['raised'] else ''}"


def topk_labels(i):
    t = topk_case(i)
    p = t["pick"]
    out = {("topk", f"{p['form']}_{'raised' if p['raised'] else 'plain'}")}
    if p["form"] == "select":
        m, n = t["sets"] - 1, t["C"] - 1
        out.add(("topk_select", "m0" if m == 0 else "m1" if m == 1 else "mn" if m == n else "m2" if m == 2 else "m_mid"))
        if p["lds"] == 150 * 1024:
            out.add(("topk_select", "lds_150K"))
        if p["lds"] == 48 * 1024:
            out.add(("topk_select", "lds_48K"))
    else:
        out.add(("topk_full", f"lds_{p['lds'] // 1024}K"))
        if t["sets"] == t["C"]:
            out.add(("topk_full", "mn"))
    if t["C"] == 32768:
        out.add(("topk", "C_max"))
    for kind in t["kinds"]:
        out.add((f"topk_{p['form']}", f"row_{kind}"))
    return out


def topk_row_is_ieee_clean(bits):
    """No NaN and not both zeros among the candidates: torch.topk's order is then the bit-pattern order up to ties."""
    cand = bits[1:]
    return not any((b & 0x7FFF) > 0x7C00 for b in cand) and not (0x0000 in cand and 0x8000 in cand)


# =================================================================================================================================
# address-coded rows
# =================================================================================================================================
def coded(tensor, shape):
    """fp16 tensor of ``shape`` = (..., T, D) (leading dims (H,) or (L, H)) whose element names its place: an integer of at
    most 2046 in magnitude; 4093 is prime, so two rows of one head differ unless their distance is a multiple of 4093."""
    lead = len(shape) - 2
    L, H = (shape[0], shape[1]) if lead == 2 else (1, shape[0])
    T, D = shape[-2], shape[-1]
    l = torch.arange(L).view(L, 1, 1, 1)
    h = torch.arange(H).view(1, H, 1, 1)
    t = torch.arange(T).view(1, 1, T, 1)
    d = torch.arange(D).view(1, 1, 1, D)
    x = ((tensor * 1009 + l * 701 + h * 307 + t * 13 + d * 3) % 4093 - 2046).to(HALF)
    return x if lead == 2 else x[0]


# ---- chunk gather -----------------------------------------------------------------------------------------------------------------
GATHER_SHAPES = ((1, 128), (4, 64), (8, 128), (12, 128), (16, 128), (24, 64), (40, 128))
GATHER_H, GATHER_C, GATHER_GUARD = 3, 11, 5


def _gather_cases():
    cases = []
    for i, (chunk, D) in enumerate(GATHER_SHAPES):
        cases.append(dict(chunk=chunk, D=D, src="token" if i == 2 else "pad" if i == 4 else "head",
                          dst="token" if i == 3 else "pad" if i == 5 else "head"))
    return cases


GATHER_CASES = _gather_cases()


def gather_id(c):
    return f"chunk{c['chunk']}-D{c['D']}-src_{c['src']}-dst_{c['dst']}"


def gather_idx():
    """(H, sets) chunk ids: chunk 0, chunk C - 1, a repeated chunk and a descending run, in another order for every head."""
    base = [0, GATHER_C - 1, 5, 5, 4, 3, 2, 9]
    return torch.tensor([base[h:] + base[:h] for h in range(GATHER_H)], dtype=torch.int32)


def gather_labels(c):
    vec = c["chunk"] * c["D"] // 8
    trip = "below_128" if vec < 128 else "at_128" if vec == 128 else "partial_second_trip" if vec % 128 else "whole_trips"
    out = {("gather", trip), ("gather", f"D{c['D']}")}
    for side in ("src", "dst"):
        if c[side] == "token":
            out.add(("gather", f"{side}_token_major"))
    if c["D"] == 128:
        out |= {("gather_fp8", "from_codes"), ("gather_fp8", "from_fp16")}
    return out


def gather_material(c):
    """-> k, v (H, T, D) coded sources, idx, want_k, want_v (H, sets * chunk, D)."""
    chunk, D = c["chunk"], c["D"]
    T = GATHER_C * chunk
    k, v = coded(1, (GATHER_H, T, D)), coded(2, (GATHER_H, T, D))
    idx = gather_idx()
    rows = (idx.long()[:, :, None] * chunk + torch.arange(chunk)[None, None, :]).reshape(GATHER_H, -1)
    pick = rows[:, :, None].expand(-1, -1, D)
    return dict(k=k, v=v, idx=idx, rows=rows, want_k=torch.gather(k, 1, pick), want_v=torch.gather(v, 1, pick))


def f8_material(c):
    """Codes and exponent bytes of an FP8 source layer for the gather from codes: every byte names its place."""
    chunk, D = c["chunk"], c["D"]
    T = GATHER_C * chunk
    h = torch.arange(GATHER_H).view(-1, 1, 1)
    t = torch.arange(T).view(1, -1, 1)
    d = torch.arange(D).view(1, 1, -1)
    kc = ((h * 83 + t * 7 + d * 3 + 1) % 251).to(torch.uint8)
    vc = ((h * 59 + t * 11 + d * 5 + 2) % 241).to(torch.uint8)
    ke = ((h[:, :, 0] * 31 + t[:, :, 0] * 3) % 23 + 112).to(torch.uint8)
    ve = ((h[:, :, 0] * 17 + t[:, :, 0] * 5) % 23 + 112).to(torch.uint8)
    return kc, vc, ke, ve


# ---- kv_copy_rows ---------------------------------------------------------------------------------------------------------------------
def _copy_cases():
    cases = []
    for D in (64, 128):
        for n in (1, 1023, 1024, 1025, 2049):
            cases.append(dict(L=1, H=1, D=D, n=n, src_t0=0, dst_t0=0, src="head", dst="head", slice=False))
    for D in (64, 128):
        cases.append(dict(L=2, H=3, D=D, n=37, src_t0=5, dst_t0=11, src="head", dst="head", slice=False))
        cases.append(dict(L=2, H=3, D=D, n=37, src_t0=9, dst_t0=2, src="head", dst="head", slice=True))
        cases.append(dict(L=2, H=3, D=D, n=37, src_t0=3, dst_t0=6, src="token", dst="head", slice=False))
        cases.append(dict(L=2, H=3, D=D, n=37, src_t0=6, dst_t0=3, src="head", dst="token", slice=False))
    cases.append(dict(L=2, H=3, D=128, n=1100, src_t0=1, dst_t0=4, src="pad", dst="pad", slice=False))
    return cases


COPY_CASES = _copy_cases()
COPY_GUARD = 7


def copy_id(c):
    return f"L{c['L']}xH{c['H']}-D{c['D']}-n{c['n']}-{c['src_t0']}to{c['dst_t0']}-{c['src']}-{c['dst']}{'-slice' if c['slice'] else ''}"


def copy_labels(c):
    vecs = c["n"] * c["D"] // 8
    out = {("kv_copy", "stride" if (vecs + 255) // 256 > 64 else "at_cap" if (vecs + 255) // 256 == 64 else "single_trip"),
           ("kv_copy", f"D{c['D']}"), ("kv_copy", "pair"), ("kv_copy", "single")}
    if c["src_t0"] != c["dst_t0"]:
        out.add(("kv_copy", "offset"))
    if c["slice"]:
        out.add(("kv_copy", "layer_slice"))
    for side in ("src", "dst"):
        if c[side] == "token":
            out.add(("kv_copy", f"{side}_token_major"))
    if c["L"] * c["H"] > 1:
        out.add(("kv_copy", "layers_heads"))
    return out


def copy_material(c):
    """-> src_k, src_v (L, H, Ts, D) coded sources and Td, the rows of a destination (``copy_expected`` gives its contents)."""
    Ts, Td = c["src_t0"] + c["n"] + COPY_GUARD, c["dst_t0"] + c["n"] + COPY_GUARD
    shape = (c["L"], c["H"], Ts, c["D"])
    return dict(src_k=coded(3, shape), src_v=coded(4, shape), Td=Td)


def copy_expected(c, src, layers=None):
    L = c["L"]
    want = torch.full((L, c["H"], c["dst_t0"] + c["n"] + COPY_GUARD, c["D"]), SENTINEL, dtype=HALF)
    ls = range(L) if layers is None else layers
    for l in ls:
        want[l, :, c["dst_t0"]:c["dst_t0"] + c["n"]] = src[l, :, c["src_t0"]:c["src_t0"] + c["n"]]
    return want


# ---- kv_shift_rows ------------------------------------------------------------------------------------------------------------------
SHIFT_DS = (64, 96, 128, 256, 2048)
SHIFT_DST_T0, SHIFT_GUARD = 2, 4


def shift_cases(D):
    """Every (n, shift) of the grid at D, deduplicated: n in {1, rpb - 1, rpb, rpb + 1, 2 rpb + 1}, shift in {1, rpb - 1, rpb,
    rpb + 1, n, n + 3}; one case per D on a token-major cache."""
    rpb = rows_per_blk(D)
    out, seen = [], set()
    for n in (1, rpb - 1, rpb, rpb + 1, 2 * rpb + 1):
        for shift in (1, rpb - 1, rpb, rpb + 1, n, n + 3):
            if n < 1 or shift < 1 or (n, shift) in seen:
                continue
            seen.add((n, shift))
            out.append(dict(D=D, n=n, shift=shift, layout="token" if (n, shift) == (rpb + 1, rpb) or rpb == 1 and (n, shift) == (2, 1) else "head"))
    return out


def shift_labels(c):
    rpb = rows_per_blk(c["D"])
    n, s = c["n"], c["shift"]
    out = {("kv_shift", f"rpb{rpb}"), ("kv_shift", "pair"), ("kv_shift", "single")}
    out.add(("kv_shift", "one_block" if n <= rpb else "two_blocks" if n <= 2 * rpb else "three_blocks"))
    if n % rpb:
        out.add(("kv_shift", "partial_block"))
    out.add(("kv_shift", "overlap" if s < n else "disjoint"))
    if 256 % (c["D"] // 8):
        out.add(("kv_shift", "idle_threads"))
    if c["layout"] == "token":
        out.add(("kv_shift", "token_major"))
    return out


def shift_material(c, L=2, H=2):
    """-> (k, v coded caches (L, H, T, D), want_k, want_v): rows [dst_t0 + shift, ... + n) moved down to [dst_t0, ...)."""
    T = SHIFT_DST_T0 + c["shift"] + c["n"] + SHIFT_GUARD
    out = []
    for tensor in (5, 6):
        x = coded(tensor, (L, H, T, c["D"]))
        want = x.clone()
        want[:, :, SHIFT_DST_T0:SHIFT_DST_T0 + c["n"]] = x[:, :, SHIFT_DST_T0 + c["shift"]:SHIFT_DST_T0 + c["shift"] + c["n"]]
        out.append((x, want))
    return out[0][0], out[1][0], out[0][1], out[1][1]


# ---- kv_gather_rows ---------------------------------------------------------------------------------------------------------------
ROWS_OFFSET, ROWS_GUARD = 3, 4


def rows_cases():
    out = []
    for D in (64, 128):
        rpb = rows_per_blk(D)
        for n in (1, rpb, rpb + 1, 2 * rpb + 1):
            lists = {"identity": list(range(n)), "plus_one": [j + 1 for j in range(n)],
                     "prefix_jump": list(range(n // 2)) + [j + 5 for j in range(n // 2, n)],
                     "next_batch": [j + rpb for j in range(n)]}
            for name, idx in lists.items():
                out.append(dict(D=D, n=n, name=name, idx=idx, T=ROWS_OFFSET + max(idx) + 1 + ROWS_GUARD,
                                layout="token" if (name, n) == ("next_batch", 2 * rpb + 1) else "pad" if (name, n) == ("prefix_jump", rpb + 1)
                                else "head"))
            out.append(dict(D=D, n=n, name="largest", idx=list(range(n - 1)) + [n + 8], T=ROWS_OFFSET + n + 9, layout="head"))   # offset + idx[-1] == T - 1
    return out


ROWS_CASES = rows_cases()


def rows_id(c):
    return f"D{c['D']}-n{c['n']}-{c['name']}-{c['layout']}"


def rows_labels(c):
    rpb = rows_per_blk(c["D"])
    n = c["n"]
    return {("kv_gather_rows", f"D{c['D']}"), ("kv_gather_rows", f"idx_{c['name']}"), ("kv_gather_rows", f"layout_{c['layout']}"),
            ("kv_gather_rows", "one_block" if n <= rpb else "two_blocks" if n <= 2 * rpb else "three_blocks")}


def rows_material(c, L=2, H=2):
    out = []
    for tensor in (7, 8):
        x = coded(tensor, (L, H, c["T"], c["D"]))
        want = x.clone()                                                       # the expectation reads a CLONE of the cache
        for j, i in enumerate(c["idx"]):
            want[:, :, ROWS_OFFSET + j] = x[:, :, ROWS_OFFSET + i]
        out.append((x, want))
    return out[0][0], out[1][0], out[0][1], out[1][1]


# =================================================================================================================================
# refusals: every documented condition of the entry points once, with its code (no launch: the pointers are never read)
# =================================================================================================================================
REFUSAL_OK = {
    "topk": dict(scores="h", idx="i", C=16, sets=4, H=2),
    "score": dict(k="h", st=128, sh=128 * 64, q="h", scores="h", C=4, chunk=8, H=2, D=128),
    "chunk_mean": dict(k="h", st=128, sh=128 * 64, index="h", ish=128 * 8, c0=0, c1=8, chunk=8, H=2, D=128),
    "score_indexed": dict(index="h", ish=128 * 8, q="h", scores="h", C=8, H=2, D=128),
    "gather": dict(ks="h", vs="h", sst=128, ssh=128 * 64, idx="i", kd="h", vd="h", dst=128, dsh=128 * 64, sets=2, chunk=4, H=2, D=128),
    "copy": dict(src="h", ssl=4096, sst=64, ssh=1024, dst="h", dsl=4096, dst_t=64, dsh=1024, src_t0=1, dst_t0=2, n=3, L=1, H=2, D=64),
    "shift": dict(cache="h", sl=4096, st=64, sh=1024, src_t0=5, dst_t0=2, n=3, L=1, H=2, D=64),
    "gather_rows": dict(k="h", v="h", sl=4096, st=64, sh=1024, offset=1, idx="i", n=3, L=1, H=2, D=64),
}
REFUSAL_OK["copy_pair"] = dict(REFUSAL_OK["copy"], src2="h", dst2="h")
REFUSAL_OK["shift_pair"] = dict(REFUSAL_OK["shift"], cache2="h")
REFUSAL_ORDER = {
    "topk": ("tf_retrieval_topk", ("scores", "idx", "C", "sets", "H")),
    "score": ("tf_retrieval_score", ("k", "st", "sh", "q", "scores", "C", "chunk", "H", "D")),
    "chunk_mean": ("tf_chunk_mean", ("k", "st", "sh", "index", "ish", "c0", "c1", "chunk", "H", "D")),
    "score_indexed": ("tf_retrieval_score_indexed", ("index", "ish", "q", "scores", "C", "H", "D")),
    "gather": ("tf_retrieval_gather", ("ks", "vs", "sst", "ssh", "idx", "kd", "vd", "dst", "dsh", "sets", "chunk", "H", "D")),
    "copy": ("tf_kv_copy_rows", ("src", "ssl", "sst", "ssh", "dst", "dsl", "dst_t", "dsh", "src_t0", "dst_t0", "n", "L", "H", "D")),
    "copy_pair": ("tf_kv_copy_rows_pair", ("src", "src2", "ssl", "sst", "ssh", "dst", "dst2", "dsl", "dst_t", "dsh", "src_t0", "dst_t0",
                                           "n", "L", "H", "D")),
    "shift": ("tf_kv_shift_rows", ("cache", "sl", "st", "sh", "src_t0", "dst_t0", "n", "L", "H", "D")),
    "shift_pair": ("tf_kv_shift_rows_pair", ("cache", "cache2", "sl", "st", "sh", "src_t0", "dst_t0", "n", "L", "H", "D")),
    "gather_rows": ("tf_kv_gather_rows", ("k", "v", "sl", "st", "sh", "offset", "idx", "n", "L", "H", "D")),
}
REFUSALS = [
    ("topk", dict(C=1, sets=1), EINVAL), ("topk", dict(sets=17), EINVAL), ("topk", dict(sets=0), EINVAL),
    ("topk", dict(C=32769), ERANGE), ("topk", dict(C=32769, sets=32769), ERANGE), ("topk", dict(H=0), EINVAL),
    ("topk", dict(scores=None), EINVAL), ("topk", dict(idx=None), EINVAL),
    ("score", dict(st=132), EINVAL), ("score", dict(sh=128 * 64 + 4), EINVAL), ("score", dict(D=96), EINVAL),
    ("score", dict(D=256), EINVAL), ("score", dict(C=0), EINVAL), ("score", dict(chunk=0), EINVAL),
    ("chunk_mean", dict(st=132), EINVAL), ("chunk_mean", dict(sh=128 * 64 + 4), EINVAL), ("chunk_mean", dict(ish=128 * 8 + 4), EINVAL),
    ("chunk_mean", dict(ish=128 * 8 - 8), EINVAL), ("chunk_mean", dict(c0=3, c1=2), EINVAL), ("chunk_mean", dict(c0=-1), EINVAL),
    ("chunk_mean", dict(D=96), EINVAL), ("chunk_mean", dict(D=256), EINVAL),
    ("score_indexed", dict(ish=128 * 8 - 8), EINVAL), ("score_indexed", dict(ish=128 * 8 + 2), EINVAL),
    ("score_indexed", dict(D=32), EINVAL), ("score_indexed", dict(C=0), EINVAL),
    ("gather", dict(D=100), EINVAL), ("gather", dict(sst=132), EINVAL), ("gather", dict(ssh=128 * 64 + 4), EINVAL),
    ("gather", dict(dst=132), EINVAL), ("gather", dict(dsh=128 * 64 + 4), EINVAL), ("gather", dict(sets=0), EINVAL),
    ("gather", dict(chunk=0), EINVAL),
    ("copy", dict(D=60), EINVAL), ("copy", dict(sst=68), EINVAL), ("copy", dict(ssh=1028), EINVAL), ("copy", dict(ssl=4100), EINVAL),
    ("copy", dict(dst_t=68), EINVAL), ("copy", dict(dsh=1028), EINVAL), ("copy", dict(dsl=4100), EINVAL),
    ("copy", dict(src_t0=-1), EINVAL), ("copy", dict(dst_t0=-1), EINVAL), ("copy", dict(n=-1), EINVAL),
    ("copy_pair", dict(D=60), EINVAL), ("copy_pair", dict(src2=None), EINVAL), ("copy_pair", dict(dst2=None), EINVAL),
    ("copy_pair", dict(dst_t=68), EINVAL),
    ("shift", dict(src_t0=2, dst_t0=5), EINVAL), ("shift", dict(D=2056), EINVAL), ("shift", dict(D=60), EINVAL),
    ("shift", dict(st=68), EINVAL), ("shift", dict(sh=1028), EINVAL), ("shift", dict(sl=4100), EINVAL), ("shift", dict(dst_t0=-1), EINVAL),
    ("shift_pair", dict(src_t0=2, dst_t0=5), EINVAL), ("shift_pair", dict(D=2056), EINVAL), ("shift_pair", dict(cache2=None), EINVAL),
    ("gather_rows", dict(D=2056), EINVAL), ("gather_rows", dict(D=4), EINVAL), ("gather_rows", dict(D=60), EINVAL),
    ("gather_rows", dict(n=0), EINVAL), ("gather_rows", dict(offset=-1), EINVAL), ("gather_rows", dict(idx=None), EINVAL),
]
REFUSAL_BUFFERS = {"h": ("float16", 2 * 1024 * 64), "i": ("int32", 64)}     # elements: larger than anything REFUSAL_OK addresses


def refusal_call(lib, entry, over, ptr_h, ptr_i, stream=None):
    """Call the entry point with REFUSAL_OK[entry] overridden by ``over``; ptr_h / ptr_i stand for every fp16 / int32 buffer."""
    name, order = REFUSAL_ORDER[entry]
    a = dict(REFUSAL_OK[entry], **over)
    args = []
    for key in order:
        v = a[key]
        args.append(None if v is None else ctypes.c_void_p(ptr_h) if v == "h" else ctypes.c_void_p(ptr_i) if v == "i" else v)
    return getattr(lib, name)(*args, stream)


# =================================================================================================================================
# the labels the case list must reach
# =================================================================================================================================
def _required():
    req = set()
    for kern in ("score", "chunk_mean"):
        req |= {(kern, "single_trip"), (kern, "stride"), (kern, "D64"), (kern, "D128")}
    req |= {("chunk_mean", "pieces"), ("chunk_mean", "piece_stride"), ("chunk_mean", "piece_off_grid"), ("score", "layout_token"),
            ("score", "layout_pad")}
    req |= {("score_indexed", p) for p in ("u1", "u2", "u3", "u4", "partial_tail", "second_trip", "D64", "D128")}
    req |= {("topk", p) for p in ("select_plain", "select_raised", "full_plain", "full_raised", "C_max")}
    req |= {("topk_select", p) for p in ("m0", "m1", "m2", "mn", "m_mid", "lds_150K", "lds_48K")}
    req |= {("topk_full", p) for p in ("lds_64K", "lds_128K", "mn")}
    for form in ("select", "full"):
        req |= {(f"topk_{form}", f"row_{k}") for k in TOPK_KINDS}
    req |= {("gather", p) for p in ("below_128", "at_128", "partial_second_trip", "whole_trips", "D64", "D128",
                                    "src_token_major", "dst_token_major")}
    req |= {("gather_fp8", "from_codes"), ("gather_fp8", "from_fp16")}
    req |= {("kv_copy", p) for p in ("single_trip", "at_cap", "stride", "D64", "D128", "pair", "single", "offset", "layer_slice",
                                     "src_token_major", "dst_token_major", "layers_heads")}
    req |= {("kv_shift", f"rpb{r}") for r in (32, 21, 16, 8, 1)}
    req |= {("kv_shift", p) for p in ("pair", "single", "one_block", "two_blocks", "three_blocks", "partial_block", "overlap",
                                      "disjoint", "idle_threads", "token_major")}
    req |= {("kv_gather_rows", p) for p in ("D64", "D128", "one_block", "two_blocks", "three_blocks", "idx_identity",
                                            "idx_plus_one", "idx_prefix_jump", "idx_next_batch", "idx_largest", "layout_head",
                                            "layout_token", "layout_pad")}
    req |= {("refusal", e) for e in REFUSAL_ORDER}
    return req


REQUIRED = _required()


def all_labels():
    out = set()
    for c in SCORE_CASES:
        out |= score_labels(c)
    for i in range(len(TOPK_SHAPES)):
        out |= topk_labels(i)
    for c in GATHER_CASES:
        out |= gather_labels(c)
    for c in COPY_CASES:
        out |= copy_labels(c)
    for D in SHIFT_DS:
        for c in shift_cases(D):
            out |= shift_labels(c)
    for c in ROWS_CASES:
        out |= rows_labels(c)
    out |= {("refusal", e) for e, _, _ in REFUSALS}
    return out
