"""Min-p on the target tier: the float64 restatement that stands in for HF's rule, the guard band that keeps
a test row's entries away from the threshold, and the comparison rules shared by tests/test_minp_cpu.py and
tests/test_gpu_minp.py.

The rule (include/triforce_hip.h, tf_minp_probs): behind temperature -> top-k -> top-p, entry i stays iff
e_i = exp(x_i - max) >= min_p.  x = l / T and d = x - max are IEEE fp32 operations, identical on CPU and device; only the
exponential differs: the device's expf lies within a few fp32 ulps (6e-8 relative each) of exp(float64(d)).  A row whose
entries all keep e / min_p outside (1 - 1e-5, 1 + 1e-5) therefore has the same kept set under either exponential; the band is a
condition on the INPUTS, not a tolerance on the outputs.  d == 0 gives e = 1.0 exactly on both sides, so at min_p == 1 the row
maxima are exempt."""
import torch

from tests import large_vocab_ref as LR

BAND = 1e-5


def _e64(lg, T):
    x = lg.float() / T                                              # fp32 division, as the kernel and the oracle divide
    d = x - x.max(-1, keepdim=True).values                          # fp32
    return d, torch.exp(d.double())


def in_band(lg, T, min_p):
    """Entries whose e / min_p lies inside the guard band (the exact maxima at min_p == 1 excepted)."""
    d, e = _e64(lg, T)
    r = e / float(min_p)
    bad = (r > 1.0 - BAND) & (r < 1.0 + BAND)
    if float(min_p) == 1.0:
        bad &= d != 0
    return bad


def nudged(lg, T, min_ps):
    """A copy of ``lg`` in which every entry inside the guard band of one of ``min_ps`` is lowered by 0.01 until none is left
    (equal logits move together, so a planted tie group stays one); asserts the condition before returning."""
    lg = lg.clone()
    for _ in range(64):
        bad = torch.zeros_like(lg, dtype=torch.bool)
        for m in min_ps:
            bad |= in_band(lg, T, m)
        if not bool(bad.any()):
            break
        lg[bad] -= 0.01
    for m in min_ps:
        assert not bool(in_band(lg, T, m).any()), f"guard band of min_p={m} still holds an entry"
    return lg


def topp_part_f64(lg, T, k, P):
    """float64 probabilities after temperature / top-k / top-p (large_vocab_ref.norm_logits_f64); top_p >= 1 keeps everything,
    as the kernels define it (the sort-based cumsum could round above 1.0 before the last rank)."""
    return LR.norm_logits_f64(lg, T, k if k is not None and 0 < k < lg.shape[-1] else None, P if P < 1.0 else 0.0)


def minp_f64(lg, T, k, P, min_p):
    """(rows, V) float64 probabilities after temperature -> top-k -> top-p -> min-p."""
    p = topp_part_f64(lg, T, k, P)
    _, e = _e64(lg, T)
    keep = (p > 0) & (e >= float(min_p))
    q = torch.where(keep, e, torch.zeros_like(e))
    return q / q.sum(-1, keepdim=True)


def check(lg, got, T, k, P, min_p, what, flips=0):
    """``got`` (fp32, CPU) against minp_f64 on rows that satisfy the guard band: row sums within 1e-5; the support equal to
    the reference's, values at rtol 2e-6 (atol 1e-9) — the bounds of DESIGN sections 19 / 26.  ``flips`` > 0 (top_p < 1): the
    supports may differ in at most that many entries per row, each of them an entry min-p keeps (so the top-p cut is the
    tighter one there) and within 2e-5 of top_p in cumulative mass over the top-k survivors, as in large_vocab_ref.check_rules.
    Returns the number of rows whose support differed."""
    from tests import helpers as Hh
    assert not bool(in_band(lg, T, min_p).any()), f"{what}: a test row violates the guard band"
    want = minp_f64(lg, T, k, P, min_p)
    assert torch.isfinite(got).all(), what
    dev = float((got.double().sum(-1) - 1).abs().max())
    print(f"{what}: row sums within {dev:.2e} of 1")
    assert dev < 1e-5, f"{what}: a row sums to 1 +- {dev:.2e}"
    _, e = _e64(lg, T)
    flipped = 0
    for r in range(lg.shape[0]):
        sg, sw = got[r] > 0, want[r] > 0
        if torch.equal(sg, sw):
            Hh.close(got[r], want[r].float(), what=f"{what} row {r}", rtol=2e-6, atol=1e-9)
            continue
        diff = torch.nonzero(sg != sw).flatten()
        assert flips > 0 and P < 1.0, f"{what} row {r}: support differs from the reference's in {diff.numel()} entries"
        assert diff.numel() <= flips, f"{what} row {r}: kept sets differ in {diff.numel()} entries"
        x = lg[r].float() / T
        S = x >= torch.topk(x, k)[0][-1] if k is not None and 0 < k < lg.shape[-1] else torch.ones_like(x, dtype=torch.bool)
        order = torch.sort(torch.softmax(x.double().masked_fill(~S, float("-inf")), -1), descending=True, stable=True)
        cum = torch.cumsum(order.values, 0)
        ranks = {int(t): i for i, t in enumerate(order.indices.tolist())}
        for t in diff.tolist():
            assert float(e[r, t]) >= min_p, f"{what} row {r}: token {t} flipped although min-p is the tighter cut there"
            before = float(cum[ranks[t] - 1]) if ranks[t] > 0 else 0.0
            assert abs(before - P) < 2e-5, f"{what} row {r}: token {t} flipped far from the top-p boundary ({before} vs {P})"
        flipped += 1
    return flipped
