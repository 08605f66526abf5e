"""Rows and float64 restatements shared by tests/test_large_vocab_cpu.py and tests/test_gpu_large_vocab.py (DESIGN section
26): the dense rows above 32 768 entries, norm_logits restated in float64, and the inverse-CDF draw restated in float64."""
import torch

DENSE_KINDS = ("sigma1", "sigma2.5", "sigma8", "dominant", "near_flat", "ties4096")


def dense_row(kind, V, seed):
    """One fp32 logits row of V entries.
    sigma*: N(0, sigma).  dominant: N(0, 2.5) with one token 30 units up.  near_flat: N(0, 0.01).
    ties4096: ten entries at 4.0, 4 096 EQUAL entries at 0.0 spread over the whole row (stride V // 4096, so they sit on both
    sides of entry 32 768 and of every slab edge), the rest at -40: at (T, P) = (0.6, 0.9) the ten carry 0.658 of the mass and at
    (0.8, 0.95) 0.266, so the top-p boundary falls INSIDE the tie group and is resolved by index order."""
    gen = torch.Generator().manual_seed(seed)
    if kind.startswith("sigma"):
        return torch.randn(V, generator=gen) * float(kind[5:])
    if kind == "dominant":
        row = torch.randn(V, generator=gen) * 2.5
        row[V - 7] = 30.0
        return row
    if kind == "near_flat":
        return torch.randn(V, generator=gen) * 0.01
    assert kind == "ties4096" and V >= 8192
    row = torch.full((V,), -40.0)
    stride = V // 4096                                    # >= 8: ties at 3 (mod stride), the ten high entries at 5 (mod stride)
    row[torch.arange(4096) * stride + 3] = 0.0
    row[torch.arange(10) * 400 * stride + 5] = 4.0
    return row


def dense_specs(rows, seed):
    """(kind, seed) of every row of a dense block: rows = 1 -> six blocks of one row, rows = 8 -> ONE block of the same six rows
    and two more seeds (so the references of the six are computed once for both)."""
    six = [(k, seed + i) for i, k in enumerate(DENSE_KINDS)]
    if rows == 1:
        return [[s] for s in six]
    assert rows == 8
    return [six + [("sigma2.5", seed + 6), ("sigma8", seed + 7)]]


def norm_logits_f64(lg, T, k, P):
    """oracle.ref_ops.norm_logits restated in float64 (same filter: x = l / T in fp32 as the kernel and the oracle divide, top-k
    by `x < kth`, stable descending sort, drop a rank when the mass BEFORE it exceeds top_p, softmax over the kept set)."""
    x = (lg.float() / T)
    if k is not None and k > 0:
        kth = torch.topk(x, min(k, x.size(-1)))[0][:, [-1]]
        x = x.masked_fill(x < kth, float("-inf"))
    xd = x.double()
    if P > 0.0:
        sv, si = torch.sort(xd, descending=True, stable=True)
        cum = torch.cumsum(torch.softmax(sv, -1), -1)
        drop_sorted = torch.zeros_like(cum, dtype=torch.bool)
        drop_sorted[..., 1:] = cum[..., :-1] > P
        drop = torch.zeros_like(drop_sorted).scatter(1, si, drop_sorted)
        xd = xd.masked_fill(drop, float("-inf"))
    return torch.softmax(xd, -1)


def reference_kind(kind, V):
    """Which reference a dense row is compared with.  The oracle (fp32 softmax / cumsum over a sorted row) is itself only
    accurate to rtol 2e-6 on the smaller shapes; measured on these rows against norm_logits_f64 (CPU, this torch build):
      V <= 40 000, the five non-tie kinds : within the rules (max value deviation 1.7e-6) -> the ORACLE is the reference;
      ties4096 at every V                 : its fp32 softmax over 3 827 kept ties sums to 1 + 1.7e-5 (values off by 3.9e-6
                                            .. 1.8e-5, same kept set);
      V = 128 256 / 262 144               : values off by up to 1.0e-4 / 1.8e-4 where the kept sets differ at the boundary, up
                                            to 10 / 22 boundary entries flipped at (0.8, 0.95), 6.5e-6 on equal kept sets
    -> those rows are compared with the FLOAT64 restatement, under the same rules."""
    return "oracle" if V <= 40000 and kind != "ties4096" else "f64"


_REF_CACHE = {}


def reference(kind, V, seed, T, k, P):
    """((1, V) logits row, reference probabilities, "oracle" | "f64"), computed once per process."""
    from oracle import ref_ops as R
    key = (kind, V, seed, T, k, P)
    if key not in _REF_CACHE:
        lg = dense_row(kind, V, seed).unsqueeze(0)
        which = reference_kind(kind, V)
        want = R.norm_logits(lg.clone(), T, k, P) if which == "oracle" else norm_logits_f64(lg, T, k, P)
        _REF_CACHE[key] = (lg, want, which)
    return _REF_CACHE[key]


def check_rules(lg, got, want, T, k, P, what):
    """The comparison rules of tests/test_gpu_topk.py::_check_against_oracle, restated with the reference ``want`` handed in
    (fp32 oracle or float64 restatement; the cumulative sums that explain the reference's own tail cut at top_p = 1 are taken in
    the reference's dtype).  Same bounds: support = survivor set at top_p >= 1, nothing outside the survivors, at most 2 boundary
    flips within 2e-5 of top_p in cumulative mass, row sums within 1e-5, values at rtol 2e-6 (atol 1e-9)."""
    from tests import helpers as Hh
    x = lg / T
    S = x >= torch.topk(x, min(k, x.size(-1)))[0][:, [-1]]
    assert torch.isfinite(got).all(), what
    dev = float((got.sum(-1) - 1).abs().max())
    assert dev < 1e-5, f"{what}: a row sums to 1 +- {dev:.2e}"
    assert not bool(((got > 0) & ~S).any()), f"{what}: an entry outside the top-k survivor set is non-zero"
    if P < 1e-6:
        assert torch.equal(got, want.to(got.dtype)), what
        return
    for r in range(lg.shape[0]):
        sg, sw = got[r] > 0, want[r] > 0
        if P >= 1.0:
            assert torch.equal(sg, S[r]), f"{what} row {r}: support differs from the survivor set in {int((sg != S[r]).sum())} entries"
            if torch.equal(sw, S[r]):
                Hh.close(got[r], want[r].float(), what=what, rtol=2e-6, atol=1e-9)
            else:                                                  # the reference's own cumsum rounded above 1.0 before the last rank
                assert not bool((sw & ~S[r]).any())
                xs = (lg[r] / T).masked_fill(~S[r], float("-inf")).to(want.dtype)
                order = torch.sort(xs, descending=True, stable=True)
                cum = torch.cumsum(torch.softmax(order.values, -1), -1)
                first = int(torch.nonzero(cum > P).flatten()[0]) + 1
                dropped = torch.zeros_like(sw)
                dropped[order.indices[first:]] = True
                assert torch.equal(S[r] & ~sw, dropped & S[r]), f"{what} row {r}: reference and kernel differ beyond the cumsum tail"
                renorm = (got[r].double() / got[r][sw].double().sum()).float()
                Hh.close(renorm[sw], want[r][sw].float(), what=what + " (reference tail cut by its own cumsum)", rtol=2e-6, atol=1e-9)
            continue
        if torch.equal(sg, sw):
            Hh.close(got[r], want[r].float(), what=what, rtol=2e-6, atol=1e-9)
            continue
        diff = torch.nonzero(sg != sw).flatten()
        assert diff.numel() <= 2, f"{what} row {r}: kept sets differ in {diff.numel()} entries"
        p_full = torch.softmax((lg[r] / T).masked_fill(~S[r], float("-inf")), -1)
        order = torch.sort(p_full, descending=True, stable=True)
        cum = torch.cumsum(order.values.double(), 0)
        ranks = {int(t): i for i, t in enumerate(order.indices.tolist())}
        for t in diff.tolist():
            rk = ranks[t]
            before = float(cum[rk - 1]) if rk > 0 else 0.0
            assert abs(before - P) < 2e-5, f"{what} row {r}: token {t} (rank {rk}) flipped far from the boundary ({before} vs {P})"


def inverse_cdf_f64(values, u):
    """(index, margin) of the inverse-CDF draw over non-negative ``values`` (any float dtype) in float64: the first index with
    non-zero mass whose inclusive cumulative sum exceeds u * total; margin = how far u * total lies from the two cumulative sums
    that bracket the decision."""
    v = values.double()
    cum = torch.cumsum(v, 0)
    target = float(u) * float(cum[-1])
    idx = int(torch.nonzero((cum > target) & (v > 0))[0])
    below = float(cum[idx]) - float(v[idx])
    return idx, min(float(cum[idx]) - target, target - below)


def uniform_inside(values, idx):
    """A uniform that lands in the middle of entry ``idx`` of the inverse CDF over ``values`` (float64)."""
    v = values.double()
    cum = torch.cumsum(v, 0)
    return float((cum[idx] - 0.5 * v[idx]) / cum[-1])
