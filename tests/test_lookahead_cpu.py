"""Lookahead form of the inner loop, the parts that need no GPU: the two-stage decision restated in torch
against two successive single-stage decisions, the on/off policy, and the rule that keeps a read-ahead inside the uniform
stream's current block."""
import pytest
import torch

from triforce_amd import ops
from triforce_amd.utils.decoding import LookaheadPolicy, lookahead_fits
from triforce_amd.utils.sampling import UniformSource

V, GAMMA = 64, 6


def one_hot(i):
    r = torch.zeros(V)
    r[i] = 1.0
    return r


def build_case(kind, n, device="cpu", v=V):
    """Constructed rows: one-hot retrieval rows make every follow-up draw deterministic, the ratio p[d] / q[d] against the
    accept uniform decides accept / reject.  Returns (p, q1, q3, tokens, ubuf, cursor0, b_hat_is_hit).
    Tokens: d = 5 at n + 1, d' = 9 at n + 3; follow-up of an accepted stage 1 is token 7."""
    g = torch.Generator().manual_seed(17)
    p = torch.rand(GAMMA + 1, v, generator=g)
    p = p / p.sum(-1, keepdim=True)
    q1, q3 = torch.full((v,), 1.0 / v), torch.full((v,), 1.0 / v)
    d1, d2, b1 = 5, 9, 7
    u = torch.full((40,), 0.5)
    c0 = 11
    acc1 = kind not in ("reject", "nan")
    # stage 1: accepted -> ratio >= 1 (p = 1/v * 2); rejected -> ratio 0.1 against u = 0.5
    p[n] = torch.full((v,), (1.0 - (2.0 if acc1 else 0.1) / v) / (v - 1))
    p[n, d1] = (2.0 if acc1 else 0.1) / v
    if kind == "nan":
        p[n, d1], q1[d1] = 0.0, 0.0                            # 0 / 0: torch.min keeps NaN, the test `u < NaN` is False
    p[n + 1] = torch.zeros(v)
    p[n + 1, b1] = 1.0                                         # the follow-up of an accepted stage 1 is token 7, whatever u
    acc2 = kind == "hit_accept"
    p[n + 2] = torch.full((v,), (1.0 - (2.0 if acc2 else 0.1) / v) / (v - 1))
    p[n + 2, d2] = (2.0 if acc2 else 0.1) / v
    tokens = torch.full((GAMMA + 3,), 100 % v, dtype=torch.int64)
    tokens[:n + 1] = torch.arange(1, n + 2)
    tokens[n + 1] = d1
    tokens[n + 2] = b1 if kind in ("hit_reject", "hit_accept") else b1 + 1
    tokens[n + 3] = d2
    ubuf = torch.rand(c0 + 40, generator=g)
    ubuf[c0 + 1] = 0.5                                         # accept tests
    ubuf[c0 + 4] = 0.5
    cursor = torch.tensor([c0], dtype=torch.int64)
    return [t.to(device) for t in (p.contiguous(), q1, q3, tokens, ubuf, cursor)]


def two_single_stages(p, q1, q3, tokens, ubuf, cursor, n, host_accept):
    """The plain loop on the same state: one decision at n; if it accepted and the follow-up it wrote IS the token the
    lookahead guessed (rows n + 2, n + 3 of p are then the rows a fresh verify would give), the next decision at n + 2 —
    whose draft token the plain loop draws into tokens[n + 3] first (here: already there, the same draw).
    -> (tokens, cursor, 8-entry record) as the two-stage form must leave them."""
    guess = int(tokens[n + 2])
    rec1 = torch.zeros(4, dtype=torch.int64)
    host_accept(p, q1, tokens, ubuf, cursor, n, GAMMA, rec1)
    acc1, b1, d1, at = rec1.tolist()
    rec = [acc1, b1, d1, at, 0, 0, 0, 0]
    if acc1 and b1 == guess and n + 3 <= GAMMA:
        rec2 = torch.zeros(4, dtype=torch.int64)
        host_accept(p, q3, tokens, ubuf, cursor, n + 2, GAMMA, rec2)
        assert rec2[3] == at + 3
        rec[4:] = [1] + rec2[:3].tolist()
    return tokens, cursor, rec


CASES = [("reject", 0), ("miss", 1), ("hit_reject", 0), ("hit_accept", 2), ("nan", 1), ("hit_accept", GAMMA - 3),
         ("hit_reject", GAMMA - 3)]


@pytest.mark.parametrize("kind,n", CASES)
def test_two_stage_decision_equals_two_single_stage_decisions(kind, n):
    state = build_case(kind, n)
    p, q1, q3, tokens, ubuf, cursor = state
    ref_tokens, ref_cursor, ref_rec = two_single_stages(p, q1, q3, tokens.clone(), ubuf, cursor.clone(), n,
                                                        ops.middle_accept_host)
    out = torch.full((ops.MID2_RECORD,), -99, dtype=torch.int64)
    ops.middle_accept2_cur(p, q1, q3, tokens, ubuf, cursor, n, GAMMA, out)
    assert out.tolist() == ref_rec
    assert tokens.tolist() == ref_tokens.tolist() and int(cursor) == int(ref_cursor)
    # the constructed case is what its name says
    acc1, _, d1, at, ran2, acc2, _, d2 = out.tolist()
    assert (acc1, ran2, acc2) == {"reject": (0, 0, 0), "nan": (0, 0, 0), "miss": (1, 0, 0), "hit_reject": (1, 1, 0),
                                  "hit_accept": (1, 1, 1)}[kind]
    assert d1 == 5 and at == 11 and int(cursor) == 11 + (6 if ran2 else 3) and (d2 == 9 if ran2 else d2 == 0)
    if n == GAMMA - 3 and kind == "hit_accept":
        # write-limit edge: stage 2 at position gamma - 1 accepted -> its follow-up lands at index gamma + 1, the last entry
        # a token buffer of gamma + 3 entries takes (and none beyond)
        assert int(tokens[GAMMA + 1]) == out[6] and int(tokens[GAMMA + 2]) == 100 % V


def test_two_stage_entry_refuses_positions_whose_rows_would_leave_the_block():
    p, q1, q3, tokens, ubuf, cursor = build_case("miss", 0)
    out = torch.zeros(ops.MID2_RECORD, dtype=torch.int64)
    with pytest.raises(AssertionError):
        ops.middle_accept2_cur(p, q1, q3, tokens, ubuf, cursor, GAMMA - 2, GAMMA, out)
    with pytest.raises(AssertionError):
        ops.middle_accept2_cur(p, q1, q3, tokens, ubuf, cursor, 0, GAMMA, out[:7])


def test_policy_switches_off_below_break_even_and_probes_again():
    pol = LookaheadPolicy(break_even=0.25)
    assert pol.on()
    for i in range(LookaheadPolicy.WINDOW - 1):                # 7 hits of the first 31: nothing is judged before a full window
        pol.replayed(i % 4 == 0 and i < 28)
        assert pol.on()
    pol.replayed(False)                                        # 7 / 32 < 0.25
    assert not pol.on() and pol.switched_off == 1
    for _ in range(LookaheadPolicy.REST - 1):
        pol.passed(1)
        assert not pol.on()
    pol.passed(1)
    assert pol.on()                                            # probe again: a fresh window
    for i in range(4 * LookaheadPolicy.WINDOW):                # 1 hit in 4 = 0.25, not below break-even: stays on
        pol.replayed(i % 4 == 0)
        assert pol.on()
    assert pol.switched_off == 1
    for i in range(LookaheadPolicy.WINDOW):                    # the window slides: 32 misses in a row end it
        pol.replayed(False)
    assert not pol.on() and pol.switched_off == 2


def test_policy_never_hitting_costs_a_window_per_period():
    """Acceptance 0 (random weights): 32 lookahead replays, then 128 plain iterations, and so on."""
    pol, looks, plain = LookaheadPolicy(break_even=0.05), 0, 0
    for _ in range(10 * (LookaheadPolicy.WINDOW + LookaheadPolicy.REST)):
        if pol.on():
            pol.replayed(False)
            looks += 1
        else:
            pol.passed(1)
            plain += 1
    assert looks == 10 * LookaheadPolicy.WINDOW and plain == 10 * LookaheadPolicy.REST


def test_lookahead_is_refused_exactly_when_it_would_read_across_a_refill():
    rng = UniformSource("cpu", seed=5, block=48)
    for pos in range(0, 49):
        rng.pos = pos
        assert lookahead_fits(rng) == (pos + 6 <= 48)
    # ... which is exactly when the plain path refills between the two iterations (or before the first)
    for pos in range(0, 49):
        rng.pos = pos
        rng._room(3)
        first = rng.pos
        rng.pos = first + 3
        rng._room(3)
        refilled = first != pos or rng.pos != first + 3
        rng.pos = pos
        assert lookahead_fits(rng) == (not refilled)
