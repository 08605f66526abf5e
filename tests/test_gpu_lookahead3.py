"""Depth-3 lookahead form of the inner loop on the device: tf_middle_accept_n_cur against three successive
tf_middle_accept_cur launches, and the decode loop with the depth-3 graphs against the plain graphs and against the depth-2
form — same tokens, same accept counts, same uniform position, whatever the guesses do."""
import pytest
import torch

from tests import helpers as Hh
from tests.test_lookahead3_cpu import B, CASES3, GAMMA, build_case3, check_case, three_single_stages

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V_GPU = 4096

# Sampling settings of the end-to-end comparison, chosen on the GPU as tests/test_gpu_lookahead.py documents its choice: the
# golden engine's draft and retrieval model are unrelated random weights, a coupled draw from two different distributions hits
# when both are flat, and a THIRD decision needs two hits in a row at n <= 1 — so a still higher temperature than the depth-2
# test's.  Measured with the uniforms of seed 901, first + second prompt (replays that decided three iterations, of depth-3
# replays, of all retrieval-verify replays): T=8 / top_p=0.99: 2 + 0 of 36 + 36 of 99 + 96; T=20 / 0.99: 0 + 2 of 34 + 34 of
# 93 + 88; T=50 / 0.999: 7 + 13 of 35 + 34 of 66 + 62 (chosen); T=200 / 0.999: 10 + 12 of 33 + 33 of 60 + 57 — all at 230
# tokens.  The test runs the chosen setting for 120 tokens (17 steps), which keeps it short: 4 + 7 third decisions of 37
# depth-3 replays, 57 replays deciding fewer.
E2E3 = dict(temperature=50.0, top_p=0.999, seed=901, max_len=120)


def test_three_stage_kernel_equals_three_single_stage_launches_all_cases():
    """Every case of the CPU test at V = 4 096; the guesses are set by hand to the follow-up token of the accepted stage (the
    one-hot row's token: a hit) or to the next token id (a miss)."""
    from triforce_amd import ops

    def launch(p, q, tokens, ubuf, cursor, n, gamma, rec):
        dev_rec = torch.zeros(4, dtype=torch.int64, device=DEV)
        ops.middle_accept_cur(p, q, tokens, ubuf, cursor, n, gamma, dev_rec)
        rec.copy_(dev_rec)

    for name, n, stages in CASES3:
        p, qs, tokens, ubuf, cursor = build_case3(stages, n, device=DEV, v=V_GPU)
        for s, kind in enumerate(stages[:2]):
            tokens[n + 2 * s + 2] = B[s] if kind == "hit" else B[s] + 1
        ref_tokens, ref_cursor, ref_rec = three_single_stages(p, qs, tokens.clone(), ubuf, cursor.clone(), n, launch)
        out = torch.full((ops.MID3_RECORD,), -99, dtype=torch.int64, device=DEV)
        ops.middle_accept_n_cur(p, qs, tokens, ubuf, cursor, n, GAMMA, out, depth=3)
        assert out.tolist() == ref_rec, name
        assert tokens.tolist() == ref_tokens.tolist() and int(cursor) == int(ref_cursor), name
        check_case(name, n, stages, out.tolist(), tokens, cursor)
        # depth 2 through the new entry is the two-stage entry, entry for entry
        if n <= GAMMA - 3:
            a, b = build_case3(stages, n, device=DEV, v=V_GPU), build_case3(stages, n, device=DEV, v=V_GPU)
            o2 = torch.full((ops.MID2_RECORD,), -99, dtype=torch.int64, device=DEV)
            on = torch.full((ops.MID2_RECORD,), -99, dtype=torch.int64, device=DEV)
            ops.middle_accept2_cur(a[0], a[1][0], a[1][1], a[2], a[3], a[4], n, GAMMA, o2)
            ops.middle_accept_n_cur(b[0], b[1][:2], b[2], b[3], b[4], n, GAMMA, on)
            assert on.tolist() == o2.tolist() and a[2].tolist() == b[2].tolist() and int(a[4]) == int(b[4]), name
    # the C entry's own range checks (the wrapper's asserts stand in front of them): depth 3 at n = gamma - 4, a 10-entry
    # record, a null q5 -> TF_EINVAL, nothing launched
    from triforce_amd import hip
    p, qs, tokens, ubuf, cursor = build_case3(("miss",), 0, device=DEV, v=V_GPU)
    out = torch.zeros(ops.MID3_RECORD, dtype=torch.int64, device=DEV)
    ptr = ops._ptr

    def entry(n, q5, out_len):
        return hip.lib().tf_middle_accept_n_cur(ptr(p), ptr(qs[0]), ptr(qs[1]), ptr(tokens), tokens.numel(), ptr(ubuf), ptr(cursor),
                                                n, GAMMA, V_GPU, 3, ptr(out), None, q5, None, out_len)
    assert entry(GAMMA - 4, ptr(qs[2]), 11) == -22 and entry(0, ptr(qs[2]), 10) == -22 and entry(0, None, 11) == -22
    torch.cuda.synchronize()
    assert out.tolist() == [0] * 11 and int(cursor) == 11


def _decode3(monkeypatch, depth, make_rng, runs=(1, 2), max_len=None):
    """TriForce on a FRESH small_gamma6 engine with lookahead off (depth 1), the depth-2 form alone, or depth 3 -> per run
    (tokens, counts, final rng.pos, stats, rng), and the engine.  Both capture-time break-evens are replaced with 0.0: the small
    engine's replay times say nothing about the policies' use, and 0.0 keeps every form on throughout."""
    from triforce_amd.utils import graph_infer as Gi
    from triforce_amd.utils.decoding import TriForce
    monkeypatch.setenv("TRIFORCE_INNER_LOOKAHEAD", "0" if depth == 1 else "1")
    monkeypatch.setenv("TRIFORCE_INNER_LOOKAHEAD_DEPTH", str(max(depth, 2)))
    monkeypatch.setattr(Gi._InnerGraphs, "_measure_break_even", lambda self, rng: 0.0)
    monkeypatch.setattr(Gi._InnerGraphs, "_measure_break_even3", lambda self, rng: 0.0)
    g = dict(Hh.load_golden("small_gamma6"), gen_len=260, budget=320)
    prompt, tok = Hh.prompt_of(g).to(DEV), Hh.FakeTokenizer()
    ge = Hh.build_product(g, DEV, temperature=E2E3["temperature"], top_p=E2E3["top_p"], graphs=True)
    out = {}
    for run_no in runs:
        rng = make_rng(ge)
        res = TriForce(tok, ge, prompt, gamma=g["gamma"], max_len=max_len or E2E3["max_len"], top_k=-1, top_p=E2E3["top_p"],
                       temperature=E2E3["temperature"], rng=rng, return_details=True)
        out[run_no] = (res["tokens"], res["counts"], rng.pos, res, rng)
    return out, ge


def _same_stream(ref_runs, got_runs, what):
    for run_no in ref_runs:
        ref, got = ref_runs[run_no], got_runs[run_no]
        assert got[0] == ref[0], f"{what}, run {run_no}: tokens diverge at {Hh.common_prefix(got[0], ref[0])} of {len(ref[0])}"
        assert got[1] == ref[1] and got[2] == ref[2], f"{what}, run {run_no}: accept counts / uniform position differ"
        assert got[3]["acc_rate_middle"] == ref[3]["acc_rate_middle"] and got[3]["drafted"] == ref[3]["drafted"]


def test_depth3_graphs_emit_the_identical_stream(monkeypatch):
    """Depth 3 against lookahead off and against the depth-2 form alone: fresh engines, the same fixed uniforms, a first and a
    second prompt — tokens, per-step accept counts, drafted, acc_rate_middle and the final uniform position are identical; over
    the two prompts >= 3 replays decide three iterations and >= 10 decide fewer."""
    from triforce_amd.utils.sampling import UniformSource
    vals = Hh.fixed_uniforms(n=4096, seed=E2E3["seed"])
    plain, ge1 = _decode3(monkeypatch, 1, lambda ge: UniformSource(DEV, values=vals))
    two, ge2 = _decode3(monkeypatch, 2, lambda ge: UniformSource(DEV, values=vals))
    three, ge3 = _decode3(monkeypatch, 3, lambda ge: UniformSource(DEV, values=vals))
    assert all(not g.look for g in ge1._inner.values())
    assert all(g.look and not g.look3 for g in ge2._inner.values()) and all(g.look and g.look3 for g in ge3._inner.values())
    sts = [three[r][3] for r in (1, 2)]
    third = sum(st["lookahead_third"] for st in sts)
    fewer = sum(st["verify_replays"] - st["lookahead_third"] for st in sts)
    d3 = sum(st["lookahead_depth3_replays"] for st in sts)
    print(f"depth 3: {third} replays decided three iterations of {d3} depth-3 replays, {fewer} replays decided fewer; "
          f"per prompt {[s['lookahead_third'] for s in sts]}; depth 2 alone: {[two[r][3]['lookahead_hits'] for r in (1, 2)]} hits")
    _same_stream(plain, three, "depth 3 against lookahead off")
    _same_stream(two, three, "depth 3 against depth 2")
    assert len(plain[1][1]) >= E2E3["max_len"] // (GAMMA + 1)            # (a step emits at most gamma + 1 tokens)
    assert all(plain[r][3]["lookahead_replays"] == 0 and two[r][3]["lookahead_third"] == 0 for r in (1, 2))
    assert all(three[r][3]["verify_replays"] <= two[r][3]["verify_replays"] for r in (1, 2))
    assert third >= 3 and fewer >= 10, (third, fewer)
    Hh.note(f"depth-3 inner graphs: {len(plain[1][0])} tokens identical to the plain graphs and to the depth-2 form, first and "
            f"second prompt; {third} of {d3} depth-3 replays decided three iterations, {fewer} replays decided fewer "
            f"(T={E2E3['temperature']}, top_p={E2E3['top_p']}, uniforms seed {E2E3['seed']})")


def test_depth3_never_reads_across_a_refill(monkeypatch):
    """A seeded stream with a 48-number block refills every few steps: depth 3 must not read its nine numbers across a refill
    (it falls back to depth 2, then to the plain graph), so it refills as often as the plain run and emits its stream — with
    depth-3, depth-2 and plain replays all occurring."""
    from triforce_amd.utils.sampling import UniformSource
    refills = {}

    def make(mode):
        def factory(ge):
            rng = UniformSource(DEV, seed=5, block=48)
            room, marks = rng._room, refills.setdefault(mode, [])

            def counting(n):
                before = rng.pos
                room(n)
                if rng.pos < before:
                    marks.append(before)
            rng._room = counting
            return rng
        return factory

    plain, _ = _decode3(monkeypatch, 1, make("plain"), runs=(1,), max_len=96)
    three, _ = _decode3(monkeypatch, 3, make("three"), runs=(1,), max_len=96)
    _same_stream(plain, three, "48-number blocks")
    assert len(refills["three"]) == len(refills["plain"]) >= 3, refills
    st = three[1][3]
    d3, d2 = st["lookahead_depth3_replays"], st["lookahead_replays"] - st["lookahead_depth3_replays"]
    assert d3 > 0 and d2 > 0 and st["verify_replays"] - st["lookahead_replays"] > 0, st
