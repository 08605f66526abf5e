"""Lookahead form of the inner loop on the device: tf_middle_accept2_cur against two successive
tf_middle_accept_cur launches, and the decode loop with the lookahead graphs against the plain graphs — same tokens, same
accept counts, same uniform position, whatever the guesses do."""
import pytest
import torch

from tests import helpers as Hh
from tests.test_lookahead_cpu import CASES, GAMMA, build_case, two_single_stages

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V_GPU = 4096

# Sampling settings of the end-to-end comparisons, chosen on the GPU so that the run has both outcomes in number (the test
# asserts >= 10 lookahead replays that decided two iterations and >= 10 that did not, over its two prompts).  The golden
# engine's draft and retrieval model are unrelated random weights: a coupled draw from two different distributions hits
# when both are flat, i.e. at a high temperature.  Measured with the uniforms of seed 901, first + second prompt, hits of
# lookahead replays: T=0.8 / top_p=0.95: 1 + 3 of 261; T=3 / 0.95: 10 + 5 of 183; T=5 / 0.99: 7 + 8 of 135;
# T=8 / 0.99: 8 + 9 of 137 (chosen).
E2E = dict(temperature=8.0, top_p=0.99, seed=901, max_len=230)


@pytest.mark.parametrize("kind,n", CASES)
def test_two_stage_kernel_equals_two_single_stage_launches(kind, n):
    from triforce_amd import ops
    p, q1, q3, tokens, ubuf, cursor = build_case(kind, n, device=DEV, v=V_GPU)
    # the guess is set by hand: to the follow-up token the reference launch draws (hit), or to another token (miss)
    probe_t, probe_c, probe = tokens.clone(), cursor.clone(), torch.zeros(4, dtype=torch.int64, device=DEV)
    ops.middle_accept_cur(p, q1, probe_t, ubuf, probe_c, n, GAMMA, probe)
    b1 = int(probe[1])
    tokens[n + 2] = b1 if kind.startswith("hit") else (b1 + 1) % V_GPU

    def launch(p, q, tokens, ubuf, cursor, n, gamma, rec):
        dev_rec = torch.zeros(4, dtype=torch.int64, device=DEV)
        ops.middle_accept_cur(p, q, tokens, ubuf, cursor, n, gamma, dev_rec)
        rec.copy_(dev_rec)

    ref_tokens, ref_cursor, ref_rec = two_single_stages(p, q1, q3, tokens.clone(), ubuf, cursor.clone(), n, launch)
    out = torch.full((ops.MID2_RECORD,), -99, dtype=torch.int64, device=DEV)
    ops.middle_accept2_cur(p, q1, q3, tokens, ubuf, cursor, n, GAMMA, out)
    assert out.tolist() == ref_rec
    assert tokens.tolist() == ref_tokens.tolist() and int(cursor) == int(ref_cursor)
    acc1, _, _, _, ran2, acc2, _, _ = out.tolist()
    assert (acc1, ran2, acc2) == {"reject": (0, 0, 0), "nan": (0, 0, 0), "miss": (1, 0, 0), "hit_reject": (1, 1, 0),
                                  "hit_accept": (1, 1, 1)}[kind]


def _decode(monkeypatch, lookahead, make_rng, runs=(1, 2), break_even=0.0, window=None, max_len=None):
    """TriForce on a FRESH small_gamma6 engine with the lookahead graphs on or off -> per run (tokens, counts, final rng.pos,
    stats, rng), and the engine.  ``break_even``: what the capture-time measurement is replaced with — the small engine's
    replay times say nothing about the policy's use; 0.0 keeps the lookahead form on throughout."""
    from triforce_amd.utils import decoding as Dm
    from triforce_amd.utils import graph_infer as Gi
    from triforce_amd.utils.decoding import TriForce
    monkeypatch.setenv("TRIFORCE_INNER_LOOKAHEAD", "1" if lookahead else "0")
    monkeypatch.setattr(Gi._InnerGraphs, "_measure_break_even", lambda self, rng: break_even)
    if window is not None:
        monkeypatch.setattr(Dm.LookaheadPolicy, "WINDOW", window[0])
        monkeypatch.setattr(Dm.LookaheadPolicy, "REST", window[1])
    g = dict(Hh.load_golden("small_gamma6"), gen_len=260, budget=320)
    prompt, tok = Hh.prompt_of(g).to(DEV), Hh.FakeTokenizer()
    ge = Hh.build_product(g, DEV, temperature=E2E["temperature"], top_p=E2E["top_p"], graphs=True)
    out = {}
    for run_no in runs:
        rng = make_rng(ge)
        res = TriForce(tok, ge, prompt, gamma=g["gamma"], max_len=max_len or E2E["max_len"], top_k=-1, top_p=E2E["top_p"],
                       temperature=E2E["temperature"], rng=rng, return_details=True)
        out[run_no] = (res["tokens"], res["counts"], rng.pos, res, rng)
    return out, ge


def _same_stream(plain, look, what):
    for run_no in plain:
        ref, got = plain[run_no], look[run_no]
        assert got[0] == ref[0], f"{what}, run {run_no}: tokens diverge at {Hh.common_prefix(got[0], ref[0])} of {len(ref[0])}"
        assert got[1] == ref[1] and got[2] == ref[2], f"{what}, run {run_no}: accept counts / uniform position differ"
        assert got[3]["acc_rate_middle"] == ref[3]["acc_rate_middle"] and got[3]["drafted"] == ref[3]["drafted"]


def test_lookahead_graphs_emit_the_identical_stream(monkeypatch):
    """Lookahead on against off, fresh engines, the same fixed uniforms, a first and a second prompt: tokens, per-step accept
    counts and the final uniform position are identical, and the two runs together have >= 10 lookahead replays of each outcome."""
    from triforce_amd.utils.sampling import UniformSource
    vals = Hh.fixed_uniforms(n=4096, seed=E2E["seed"])
    plain, ge0 = _decode(monkeypatch, False, lambda ge: UniformSource(DEV, values=vals))
    look, ge1 = _decode(monkeypatch, True, lambda ge: UniformSource(DEV, values=vals))
    assert all(not g.look for g in ge0._inner.values()) and all(g.look for g in ge1._inner.values())
    sts = [look[r][3] for r in (1, 2)]
    hits = sum(st["lookahead_hits"] for st in sts)
    misses = sum(st["lookahead_replays"] - st["lookahead_hits"] for st in sts)
    st = dict(verify_replays=sum(st["verify_replays"] for st in sts))
    print(f"lookahead: {hits} hits, {misses} misses, {st['verify_replays']} verify replays for "
          f"{sum(plain[r][3]['outer_steps'] for r in (1, 2))} steps; per prompt {[s['lookahead_hits'] for s in sts]}")
    _same_stream(plain, look, "lookahead graphs")
    assert len(plain[1][1]) >= 30
    assert plain[2][3]["lookahead_replays"] == 0
    assert hits >= 10 and misses >= 10, (hits, misses)
    Hh.note(f"lookahead inner graphs: {len(plain[1][0])} tokens identical to the plain graphs, first and second prompt; "
            f"{hits} hits / {misses} misses in {st['verify_replays']} retrieval verifies (T={E2E['temperature']}, "
            f"top_p={E2E['top_p']}, uniforms seed {E2E['seed']})")


def test_lookahead_never_reads_across_a_refill(monkeypatch):
    """A seeded stream with a 48-number block refills every few steps: the lookahead form must refuse to read ahead across a
    refill, so both forms refill equally often (>= 3 times) and emit the same stream — with lookahead replays on both
    sides of a refill."""
    from triforce_amd.utils.sampling import UniformSource
    refills = {}

    def make(mode):
        def factory(ge):
            rng = UniformSource(DEV, seed=5, block=48)
            room, marks = rng._room, refills.setdefault(mode, [])

            def counting(n):
                before = rng.pos
                room(n)
                if rng.pos < before:                           # a refill: note the lookahead replays issued so far
                    look = getattr(getattr(ge, "_tf_spec_buffers", None), "lookahead", None)
                    marks.append(look.lookahead_replays if look is not None else 0)
            rng._room = counting
            return rng
        return factory

    plain, _ = _decode(monkeypatch, False, make("plain"), runs=(1,), max_len=96)
    look, _ = _decode(monkeypatch, True, make("look"), runs=(1,), max_len=96)
    _same_stream(plain, look, "48-number blocks")
    assert len(refills["look"]) == len(refills["plain"]) >= 3, refills
    total, marks = look[1][3]["lookahead_replays"], refills["look"]
    assert any(0 < m < total for m in marks), (marks, total)   # some refill has lookahead replays before AND after it


def test_policy_switching_mid_run_leaves_the_stream_alone(monkeypatch):
    """A policy that keeps falling below break-even (windows of 8 lookahead replays, 16 plain iterations of rest) switches
    the form off and on many times inside one run: the stream is the plain graphs' stream."""
    from triforce_amd.utils.sampling import UniformSource
    vals = Hh.fixed_uniforms(n=4096, seed=E2E["seed"])
    plain, _ = _decode(monkeypatch, False, lambda ge: UniformSource(DEV, values=vals), runs=(1,))
    look, ge = _decode(monkeypatch, True, lambda ge: UniformSource(DEV, values=vals), runs=(1,), break_even=2.0, window=(8, 16))
    _same_stream(plain, look, "policy switching")
    st, pol = look[1][3], ge._tf_spec_buffers.lookahead.policy
    assert pol.switched_off >= 3 and st["lookahead_replays"] == 8 * pol.switched_off + len(pol.recent)
    assert st["verify_replays"] > st["lookahead_replays"] > 0
