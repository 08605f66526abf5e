"""Depth-3 lookahead form of the inner loop, the parts that need no GPU: the N-stage decision restated in
torch against three successive single-stage decisions, the entry's range checks, the 3-versus-2 policy, the refill rule at
depth 3, and step 0's walk over recorded iterations."""
import os
import sys

import pytest
import torch

from triforce_amd import ops
from triforce_amd.utils.decoding import LookaheadDepthPolicy, lookahead_fits
from triforce_amd.utils.sampling import UniformSource

V, GAMMA, C0 = 64, 6, 11
FILL = 36                  # what the token buffer holds where nothing was put
D = (5, 9, 13)             # the draft token of stage s, at tokens[n + 2s + 1]
B = (7, 11, 15)            # the follow-up token of an ACCEPTED stage s (a one-hot row: whatever the uniform)

# what each stage does: "hit" = accepted and the guess behind it is its follow-up; "miss" = accepted, another guess;
# "acc" = accepted (last stage: there is no guess behind it); "rej" = rejected; "nan" = a 0 / 0 ratio (rejected)
CASES3 = [("reject", 0, ("rej",)),
          ("accept_miss", 1, ("miss",)),
          ("hit_reject", 0, ("hit", "rej")),
          ("hit_accept_miss", 1, ("hit", "miss")),
          ("hit_hit_reject", 0, ("hit", "hit", "rej")),
          ("hit_hit_accept", GAMMA - 5, ("hit", "hit", "acc")),         # n = 1: the write-limit edge
          ("nan_stage2", 0, ("hit", "nan")),
          ("nan_stage3", 1, ("hit", "hit", "nan"))]


def build_case3(stages, n, device="cpu", v=V):
    """Constructed rows in the style of test_lookahead_cpu.build_case, for up to three stages: the ratio p[d] / q[d] against
    the accept uniform 0.5 decides accept (2) / reject (0.1), a one-hot row behind an accepted stage makes its follow-up
    B[s].  Stages the outcome list does not reach keep random rows and a guess that cannot matter.
    Returns [p, (q1, q3, q5), tokens, ubuf, cursor]."""
    g = torch.Generator().manual_seed(17)
    p = torch.rand(GAMMA + 1, v, generator=g)
    p = p / p.sum(-1, keepdim=True)
    qs = [torch.full((v,), 1.0 / v) for _ in range(3)]
    tokens = torch.full((GAMMA + 3,), FILL, dtype=torch.int64)
    tokens[:n + 1] = torch.arange(1, n + 2)
    ubuf = torch.rand(C0 + 40, generator=g)
    for s in range(3):
        pos = n + 2 * s
        tokens[pos + 1] = D[s]
        ubuf[C0 + 3 * s + 1] = 0.5                             # the accept test of stage s
        if s >= len(stages):
            if pos + 2 <= GAMMA and s + 1 < 3:
                tokens[pos + 2] = B[s] + 1
            continue
        kind = stages[s]
        accepted = kind in ("hit", "miss", "acc")
        ratio = 2.0 if accepted else 0.1
        p[pos] = torch.full((v,), (1.0 - ratio / v) / (v - 1))
        p[pos, D[s]] = ratio / v
        if kind == "nan":
            p[pos, D[s]], qs[s][D[s]] = 0.0, 0.0
        p[pos + 1] = torch.zeros(v)
        p[pos + 1, B[s]] = 1.0
        if s + 1 < 3:
            tokens[pos + 2] = B[s] if kind == "hit" else B[s] + 1
    cursor = torch.tensor([C0], dtype=torch.int64)
    return [p.contiguous().to(device), tuple(q.to(device) for q in qs), tokens.to(device), ubuf.to(device), cursor.to(device)]


def three_single_stages(p, qs, tokens, ubuf, cursor, n, host_accept, depth=3):
    """The plain loop on the same state: a decision at n; while it accepted and the follow-up it wrote IS the token the
    lookahead guessed, the next decision two positions on (its draft token is already in place: the same draw).
    -> (tokens, cursor, record of 5 + 3 (depth - 1) entries) as the N-stage form must leave them."""
    rec, ran, at0 = [], 0, int(cursor[0])
    for s in range(depth):
        pos = n + 2 * s
        guess = int(tokens[pos + 2]) if s + 1 < depth else None
        r = torch.zeros(4, dtype=torch.int64)
        host_accept(p, qs[s], tokens, ubuf, cursor, pos, GAMMA, r)
        acc, b, d, at = r.tolist()
        assert at == at0 + 3 * s
        rec.append([acc, b, d])
        ran = s + 1
        if not (s + 1 < depth and acc and b == guess):
            break
    full = rec[0] + [at0, ran - 1]
    for s in range(1, depth):
        full += rec[s] if s < ran else [0, 0, 0]
    return tokens, cursor, full


def expected_shape(stages):
    """(stages run, accept flag per stage run) the named case must show."""
    return len(stages), [1 if k in ("hit", "miss", "acc") else 0 for k in stages]


def check_case(name, n, stages, out, tokens, cursor):
    ran, accs = expected_shape(stages)
    assert out[4] == ran - 1 and out[3] == C0 and int(cursor) == C0 + 3 * ran, name
    got = [out[0]] + [out[5 + 3 * (s - 1)] for s in range(1, ran)]
    assert got == accs, name
    assert out[2] == D[0] and all(out[5 + 3 * (s - 1) + 2] == D[s] for s in range(1, ran)), name
    assert all(v == 0 for v in out[5 + 3 * (ran - 1):]), name              # zeros for a stage that did not run
    if name == "hit_hit_accept":
        # stage 3 at position gamma - 1 accepted: its follow-up lands at index gamma + 1 and nothing beyond
        assert n + 6 == GAMMA + 1 and int(tokens[GAMMA + 1]) == B[2] == out[9] and int(tokens[GAMMA + 2]) == FILL


@pytest.mark.parametrize("name,n,stages", CASES3)
def test_three_stage_decision_equals_three_single_stage_decisions(name, n, stages):
    p, qs, tokens, ubuf, cursor = build_case3(stages, n)
    ref_tokens, ref_cursor, ref_rec = three_single_stages(p, qs, tokens.clone(), ubuf, cursor.clone(), n, ops.middle_accept_host)
    out = torch.full((ops.MID3_RECORD,), -99, dtype=torch.int64)
    ops.middle_accept_n_cur(p, qs, tokens, ubuf, cursor, n, GAMMA, out, depth=3)
    assert ops.MID3_RECORD == 11 and out.tolist() == ref_rec
    assert tokens.tolist() == ref_tokens.tolist() and int(cursor) == int(ref_cursor)
    check_case(name, n, stages, out.tolist(), tokens, cursor)


def test_n_stage_entry_refuses_what_would_leave_the_block_or_the_record():
    p, qs, tokens, ubuf, cursor = build_case3(("miss",), 0)
    out = torch.zeros(ops.MID3_RECORD, dtype=torch.int64)
    with pytest.raises(AssertionError):
        ops.middle_accept_n_cur(p, qs, tokens, ubuf, cursor, GAMMA - 4, GAMMA, out, depth=3)     # row n + 5 > gamma
    with pytest.raises(AssertionError):
        ops.middle_accept_n_cur(p, qs, tokens, ubuf, cursor, 0, GAMMA, out[:10], depth=3)        # a 10-entry record
    with pytest.raises(AssertionError):
        ops.middle_accept_n_cur(p, (qs[0], qs[1], None), tokens, ubuf, cursor, 0, GAMMA, out, depth=3)   # a null q5
    with pytest.raises(AssertionError):
        ops.middle_accept_n_cur(p, qs[:2], tokens, ubuf, cursor, 0, GAMMA, out, depth=3)
    assert int(cursor) == C0 and out.tolist() == [0] * 11                                        # nothing ran


@pytest.mark.parametrize("name,n,stages", [c for c in CASES3 if c[1] <= GAMMA - 3])
def test_depth_two_through_the_n_stage_entry_equals_the_two_stage_entry(name, n, stages):
    a, b = build_case3(stages, n), build_case3(stages, n)
    out2 = torch.full((ops.MID2_RECORD,), -99, dtype=torch.int64)
    ops.middle_accept2_cur(a[0], a[1][0], a[1][1], a[2], a[3], a[4], n, GAMMA, out2)
    outn = torch.full((ops.MID2_RECORD,), -99, dtype=torch.int64)
    ops.middle_accept_n_cur(b[0], b[1][:2], b[2], b[3], b[4], n, GAMMA, outn)
    assert outn.tolist() == out2.tolist() and a[2].tolist() == b[2].tolist() and int(a[4]) == int(b[4])


def test_depth_policy_switches_down_rests_and_probes_again():
    pol = LookaheadDepthPolicy(break_even=0.25)
    W, R = LookaheadDepthPolicy.WINDOW, LookaheadDepthPolicy.REST
    assert pol.on()
    for i in range(W - 1):                                     # 7 third decisions in the first 31: no verdict before a full window
        pol.replayed(i % 4 == 0 and i < 28)
        assert pol.on()
    pol.replayed(False)                                        # 7 / 32 < 0.25
    assert not pol.on() and pol.switched_down == 1
    pol.passed(R - 3)                                          # depth-2 replays deciding one or two iterations each
    assert not pol.on()
    pol.passed(2)
    assert not pol.on()
    pol.passed(2)                                              # (a replay may carry the count past the end)
    assert pol.on() and pol.recent == []                       # probe again: a fresh window
    for i in range(4 * W):                                     # 1 in 4 = 0.25, not below break-even: stays at depth 3
        pol.replayed(i % 4 == 0)
        assert pol.on()
    pol.passed(5)                                              # iterations at other positions while on: no effect
    assert pol.on() and pol.switched_down == 1
    for i in range(W):
        pol.replayed(False)
    assert not pol.on() and pol.switched_down == 2


def test_depth_three_is_refused_exactly_when_it_would_read_across_a_refill():
    rng = UniformSource("cpu", seed=5, block=48)
    for pos in range(0, 49):
        rng.pos = pos
        assert lookahead_fits(rng, 3) == (pos + 9 <= 48)
        assert lookahead_fits(rng) == lookahead_fits(rng, 2) == (pos + 6 <= 48)      # depth 2 stays the default


def test_walk_over_a_hand_written_list():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import lookahead_count as lc
    finally:
        sys.path.pop(0)

    def it(n, hit):
        return {"n": n, "hit": bool(hit)}

    steps = [
        [it(0, 1), it(2, 1), it(4, 0), it(5, 0)],      # depth 3 at 0 decides 0, 2, 4; plain at 5
        [it(0, 1), it(2, 0), it(3, 1), it(5, 0)],      # depth 3 at 0 decides 0, 2 (stage 2 missed); depth 2 at 3 decides 3, 5
        [it(0, 0), it(1, 1), it(3, 1), it(5, 0)],      # depth 3 at 0 decides 0; depth 3 at 1 decides 1, 3, 5
        [it(0, 0), it(1, 0), it(2, 1), it(4, 1)],      # depth 3 x 2 deciding one each; depth 2 at 2 decides 2, 4 (a last hit skips nothing)
        [it(0, 1), it(2, 1)],                          # the step ends behind stage 2: no third iteration to decide
    ]
    w3 = lc.walk_depth(steps, GAMMA, "hit", 3)
    assert w3["replays_by_depth"] == {1: 1, 2: 2, 3: 7} and w3["replays"] == 10
    assert w3["decided"] == {1: 4, 2: 4, 3: 2} and w3["iterations"] == sum(len(s) for s in steps) == 18
    assert w3["draft_steps"] == 1 * 1 + 2 * 3 + 7 * 5
    w2 = lc.walk_depth(steps, GAMMA, "hit", 2)
    # depth 2 over the same list: [0,2] [4] [5] | [0,2] [3,5] | [0] [1,3] [5] | [0] [1] [2,4] | [0,2]
    assert w2["replays"] == 12 and w2["replays_by_depth"] == {1: 3, 2: 9} and w2["decided"] == {1: 6, 2: 6}
    legacy = lc.walk(steps, GAMMA, "hit")
    assert legacy[0] == w2["replays"] and legacy[1] == w2["replays_by_depth"][2] and legacy[2] == w2["decided"][2]
    pr = lc.project_depth3(steps, GAMMA, "hit", rv_us=3000.0, draft_us=70.0, draw_us=10.0)
    more = w3["draft_steps"] - w2["draft_steps"]
    assert pr["skipped_replays_per_step"] == 0.4 and pr["depth3"]["third_decisions_per_step"] == 0.4
    assert pr["projected_net_saving_us_per_step"] == round((2 * 3000.0 - more * 80.0) / 5, 1)
