"""The attention probes (tests/attn_probes.py) proven on the CPU oracle, for every case tests/test_gpu_attn_probes.py runs.

Conditions on the inputs, per case and mode (needle / decoy in both parities, NaN or +65504 in the spare capacity):
  (a) the oracle on k[:sk], v[:sk] returns v[target] bit for bit on every probed row;
  (b) the leak, sum over a row's other visible keys of exp(s - s_target), is at most 2^-16: one fp16 half-ulp is 2^-12
      relative at worst, so the kernel keeps 15/16 of it;
  (c) every decoy leads its row's target by at least 20 nats;
  (d) every |score| is at most 256 nats: an fp32 score's own rounding (256 log2(e) 2^-24 < 2^-15) stays inside the half-ulp.
These are conditions the oracle alone must meet, not measurements of the kernels: a seed that breaks one is changed
(attn_probes.SEED_BUMP), never the cap.  Seeds: attn_probes.seed_of, a function of the case's shape; one case is bumped.
Measured over all cases (smallest target-to-runner-up gap / largest leak / smallest decoy lead / largest |score|):
D = 128: 35.4 nats / 4.4e-16 / 45.25 / 135.8;  D = 64: 13 nats (one prefill row; 16 elsewhere) / 2.3e-6 = 2^-18.7 / 31.97 / 96.0.

Power of the assertion: the GPU file's checking function is run on mutated oracles (attn_probes.mutants) — mask one key
wider / narrower, key sk read (its score, or P = 0 times its V row), one key dropped at each boundary, a 16-key tile dropped
or counted twice, query head h on KV head h % Hkv, the tree bit column off by one.  Each must be rejected on at least one
case of its entry point, with a message that names the row, the head and the key the output is nearest to.

Why the probes: with randn q / k / v the softmax is nearly uniform and a single-key mistake moves an output by |v| / sk.
The same mutants against the fp32 oracle on randn inputs, max |d| / (atol + rtol |want|) at the block kernels' 2e-3 / 2e-3
(below 1 = the mutant PASSES), two seeds each (tests/test_gpu_ops.py's seeds 3 + sq and 41 + sq):

  sq, sk, H, D          | one key too wide | one too narrow | key below the causal band lost | key 0 lost
  33, 5000, 4, 128      | 2.67, 2.27       | 4.77, 2.68     | 1.65, 3.35                     | 1.35, 1.82
  128, 9000, 4, 64      | 4.91, 1.43       | 1.93, 2.79     | 1.58, 1.23                     | 2.15, 1.47
  1024, 5000, 2, 128    | 5.46, 3.71       | 3.76, 6.46     | 6.54, 6.23                     | 6.72, 4.79
  64, 20000, 2, 128     | 0.86, 0.61       | 0.55, 0.98     | 0.63, 0.60                     | 0.50, 0.35
"""
import re

import pytest
import torch

from tests import attn_probes as P
from tests.test_gpu_attn_probes import TOL, check


def _plain_close(got, want, what="", atol=None, rtol=None):
    torch.testing.assert_close(got, want, atol=atol, rtol=rtol)       # (helpers.close would write parity rows for mutants)


def _quantize(c):
    from triforce_amd import ops
    return ops.kv_quantize_ref if c["ep"] in ("fp8", "fp8_tail") else None


@pytest.mark.parametrize("c", P.ALL_CASES, ids=P.case_id)
def test_probe_inputs_meet_the_conditions_on_the_oracle(c):
    for kind, parity, poison in P.MODES:
        inp = P.build(c, kind, parity, poison, quantize=_quantize(c))
        what = f"{P.case_id(c)} {kind}{parity} {poison}"
        sk, cap = inp["sk"], inp["cap"]
        assert cap - sk >= 16
        # poison fills the whole spare capacity of V, and of K apart from the planted decoys
        bad = ~torch.isfinite(inp["v"][sk:].float()) | (inp["v"][sk:].float() == 65504.0)
        assert bool(bad.all()), what
        for t in range(sk, cap):
            assert (t in inp["planted"]) != bool((~torch.isfinite(inp["k"][t].float()) | (inp["k"][t].float() == 65504.0)).all())
        want = P.oracle(inp)
        check(inp, want, want, what, close=_plain_close)                        # (a): bit for bit on every probed row
        fig = P.conditions(inp)
        assert fig["leak"] <= P.LEAK_CAP, f"{what}: leak {fig['leak']:.3e} (gap {fig['gap']:.1f} nats): change the seed"      # (b)
        assert fig["lead"] >= P.DECOY_LEAD, f"{what}: a decoy leads by {fig['lead']:.1f} nats only"                          # (c)
        assert fig["max_score"] <= P.SCORE_CAP, what                                                                        # (d)
        # a second, differently ordered fp32 attention passes the same check: it is the mutations that the mutants fail on
        check(inp, P.masked_attn(inp), want, what, close=_plain_close)
        tgt = inp["target"]
        probed = int((tgt >= 0).sum())
        assert probed > 0
        if kind == "decoy" and (inp["sq"] > 1 or parity == 0):           # (one row: it is the parity-0 row)
            assert inp["decoys"] and all(not bool(inp["vis"][i, f]) for i, h, f in inp["decoys"])       # unseen by their own row
            assert all(int(tgt[i, h]) not in inp["planted"] for i in range(inp["sq"]) for h in range(inp["H"]))
            if c["ep"] != "tree":
                assert any(f == sk for _, _, f in inp["decoys"]) == (parity == 0)      # the last row's decoy sits at index sk
                assert any(f == cap - 1 for _, _, f in inp["decoys"])
        for h in range(inp["H"]):                                       # no two rows of a head share a target
            col = tgt[:, h][tgt[:, h] >= 0].tolist()
            assert len(col) == len(set(col))
        for i in range(inp["sq"]):                                      # the query heads of a row differ
            row = tgt[i][tgt[i] >= 0].tolist()
            assert len(row) == len(set(row))
        if sk > inp["sq"] + 2 * inp["H"] and kind == "needle":          # (sq == sk: a row may have no free target)
            assert probed == tgt.numel(), f"{what}: {tgt.numel() - probed} rows without a target"
        assert 2 * probed >= tgt.numel() - 2 * inp["H"], what              # (decoys take every other key from the late rows of sk ~ sq)
        _COVERED.setdefault(P.case_id(c), set()).update(inp["covered"])


_COVERED = {}                                     # case id -> labels its targets landed on (filled by the test above)


def _labels(c):
    if P.case_id(c) not in _COVERED:
        for kind, parity, poison in P.MODES:
            _COVERED.setdefault(P.case_id(c), set()).update(P.build(c, kind, parity, poison, quantize=_quantize(c))["covered"])
    return _COVERED[P.case_id(c)]


@pytest.mark.parametrize("ep", list(P.CASES))
def test_targets_land_on_every_boundary_of_the_entry_point(ep):
    """Over the cases of one entry point: key 0, a row's own edge, 15 | 16, 63 | 64, the first and last key of every split of
    every explicit split count (the prefill kernels: of the rule's count), sk_codes - 1 | sk_codes, tree columns 31 | 32 | 63 | 64."""
    need = {"key0", "edge", "t15", "t16", "s63", "s64"}
    got = set()
    for c in P.CASES[ep]:
        got |= _labels(c)
        need |= {lab for lab, _ in P.specials(c) if lab.startswith(("split", "codes", "col", "prefix", "tree"))}
    assert need <= got, sorted(need - got)
    if ep not in ("tree", "rope", "prefill", "prefill_gqa"):
        assert any(lab.startswith("split3.") for lab in got)
    if ep in ("prefill", "prefill_gqa"):
        assert any(lab.startswith("split") for lab in got)


NAMES_THE_KEY = re.compile(r"row \d+ head \d+: expected V row of key \d+ .*nearest to the V row of key \d+ \(KV head \d+\)", re.S)


def _rejected(inp, out, want):
    """The check's message when it rejects ``out``, else None."""
    try:
        check(inp, out, want, "mutant", close=_plain_close, exact=inp["kind"] != "sink")
    except AssertionError as e:
        return str(e)
    return None


def _mutant_cases(ep):
    small = [c for c in P.CASES[ep] if c["sk"] <= 700]
    big = [c for c in P.CASES[ep] if c["sk"] > 700]
    return small[:6] + small[-4:] + big[-1:]


@pytest.mark.parametrize("ep", list(P.CASES))
def test_every_mutant_is_rejected_and_the_message_names_the_leaked_key(ep):
    caught, seen, leaked = {}, set(), {}
    sinks = [P.build_sink(c, quantize=_quantize(c)) for c in P.SINK_CASES if c["ep"] == ep]
    for inp in [P.build(c, kind, parity, poison, quantize=_quantize(c)) for c in _mutant_cases(ep)
                for kind, parity, poison in P.MODES] + sinks:
        want = P.oracle(inp)
        for name, fn in P.mutants(inp).items():
            seen.add(name)
            msg = _rejected(inp, fn(), want)
            if msg is not None:
                caught.setdefault(name, []).append(msg)
                m = re.search(r"nearest to the V row of key (\d+)", msg)
                if m and inp["kind"] != "sink":
                    leaked.setdefault(name, (int(m.group(1)), inp))
    assert seen == set(caught), f"mutants that passed every case of {ep}: {sorted(seen - set(caught))}"
    expect = {"drop_key0", "drop_t15", "drop_t16", "drop_s63", "drop_s64", "tile_dropped", "tile_twice", "pv_past_sk"}
    if ep != "tree":
        expect |= {"mask_one_wider", "mask_one_narrower", "key_sk_read"}
    else:
        expect |= {"tree_bit_plus_one", "tree_bit_minus_one"}
    if ep not in ("rope", "tree"):
        expect |= {"drop_first", "drop_last"}
    if ep in ("decode_gqa", "prefill_gqa"):
        expect.add("head_mod_hkv")
    assert expect <= seen, sorted(expect - seen)
    for name in seen - {"tile_twice", "pv_past_sk"}:                  # (those two fail the tolerance / the NaN assertion)
        assert any(NAMES_THE_KEY.search(m) for m in caught[name]), f"{name}: {caught[name][0][:300]}"
    # the key the message names is the one the mutation let in
    for name in ("mask_one_wider", "key_sk_read"):
        if name in leaked:
            key, inp = leaked[name]
            assert key in inp["planted"], f"{name}: names key {key}, planted {sorted(inp['planted'])}"


@pytest.mark.parametrize("c", P.SINK_CASES, ids=P.case_id)
def test_sink_inputs_put_about_half_of_every_row_on_key_zero(c):
    inp = P.build_sink(c, quantize=_quantize(c))
    k = inp["k"][:inp["sk"]]
    if c["ep"] == "rope":
        from oracle import ref_ops as R
        k = R.apply_rope(k, inp["cos"], inp["sin"], torch.arange(inp["sk"]))
    s = torch.einsum("ihd,thd->hit", inp["q"].float(), k.float()[:, inp["kvmap"]]) * float(inp["scale"])
    p0 = torch.softmax(s.masked_fill(~inp["vis"][None, :, :inp["sk"]], float("-inf")), dim=-1)[:, :, 0]
    assert 0.03 < float(p0.min()) and float(p0.max()) < 0.97 and 0.3 < float(p0.mean()) < 0.7, (p0.min(), p0.mean(), p0.max())
    want = P.oracle(inp)
    check(inp, P.masked_attn(inp), want, "sink", close=_plain_close, exact=False)


def test_tree_decoys_sit_on_both_sides_and_on_the_word_edges():
    """Non-ancestor columns below and above the row's own, columns 31 | 32 and 63 | 64 (the mask's word edges) among them."""
    cols, below, above = set(), 0, 0
    for c in P.CASES["tree"]:
        for kind, parity, poison in P.MODES[1:]:
            inp = P.build(c, kind, parity, poison)
            for i, h, f in inp["decoys"]:
                assert inp["prefix"] <= f < inp["sk"] and not bool(inp["vis"][i, f])
                cols.add(f - inp["prefix"])
                below += f < P.edge_of(inp, i)
                above += f > P.edge_of(inp, i)
    assert {31, 32, 63, 64} <= cols and below > 100 and above > 100


def test_sign_keys_and_their_decoys_are_exact_fp8_codes():
    from triforce_amd import ops
    c = P.CASES["fp8"][0]
    inp = P.build(c, "decoy", 0, None, quantize=ops.kv_quantize_ref)
    for name in ("k", "v"):
        assert torch.equal(ops.kv_quantize_ref(inp[name])[2], inp[name])
    assert float(inp["k"].abs().max()) == 1.5


def test_tolerances_are_the_entry_points_own():
    from tests import test_gpu_ops as T
    assert TOL["decode"] == (T.DECODE_ATOL, T.DECODE_RTOL) == (2e-5, 1.5e-3)
    assert TOL["block"] == TOL["prefill"] == TOL["tree"] == (T.ATTN_ATOL, T.ATTN_RTOL) == (2e-3, 2e-3)
    assert TOL["rope"] == (6e-4, 2e-3)
