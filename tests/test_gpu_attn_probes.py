"""The attention kernels on selection inputs (tests/attn_probes.py): every probed (row, head) must return its target key's
V row BIT FOR BIT, with the hottest key of all planted one past the row's causal edge / in the spare capacity / on a
non-ancestor tree column, and NaN, +65504 or FP8 NaN codes in every cache row past sk.

Per launch, in order (attn_probes.check): 1. no NaN / Inf in the output; 2. the entry point's EXISTING tolerance against the
oracle on all rows (through helpers.close: the parity table gets its rows); 3. torch.equal(out, v[target]) on the probed rows;
4. a failure names row, head, expected key and the key whose V row the output is nearest to.

Why bit equality is owed: the softmax sum has one term.  The target's P is exp2 of an fp32 rounding residue below 2^-15, l has
the same value, the other visible keys add at most 2^-16 (condition (b) of test_attn_probes_cpu) — in total less than the 2^-12
half-ulp of fp16, whether P reaches the matrix core rounded once or as hi + lo.
"""
import time

import pytest
import torch

from oracle import ref_ops as R                                       # noqa: F401  (the oracle behind attn_probes.oracle)
from tests import attn_probes as P
from tests import helpers as Hh
from tests.test_gpu_ops import ATTN_ATOL, ATTN_RTOL, DECODE_ATOL, DECODE_RTOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the existing tolerance of each entry point (tests/test_gpu_ops.py, test_gpu_gqa.py, test_gpu_sequoia.py)
TOL = {"decode": (DECODE_ATOL, DECODE_RTOL), "decode_gqa": (DECODE_ATOL, DECODE_RTOL), "fp8": (DECODE_ATOL, DECODE_RTOL),
       "fp8_tail": (DECODE_ATOL, DECODE_RTOL), "block": (ATTN_ATOL, ATTN_RTOL), "prefill": (ATTN_ATOL, ATTN_RTOL),
       "prefill_gqa": (ATTN_ATOL, ATTN_RTOL), "tree": (ATTN_ATOL, ATTN_RTOL), "rope": (6e-4, 2e-3)}


def check(inp, out, want, what, exact=True, close=Hh.close):
    atol, rtol = TOL[inp["ep"]]
    P.check(inp, out, want, atol, rtol, close, what=what, exact=exact)


def _ops():
    from triforce_amd import ops
    return ops


def _head_major(x):
    return x.permute(1, 0, 2).contiguous().to(DEV)


def _f8_layer(ops, inp, lo, hi, coded):
    """Logical rows [lo, hi) of K and V as an FP8 layer: codes (Hkv, T, D), exponent bytes (Hkv, T).  Rows at or past
    ``coded`` that hold no planted decoy are poison: code 0x7F (NaN) with exponent byte 0xFF."""
    out = []
    for name in ("k", "v"):
        x = inp[name][lo:hi]
        live = torch.tensor([t < coded or (name == "k" and t in inp["planted"]) for t in range(lo, hi)])
        codes, exps, deq = ops.kv_quantize_ref(torch.where(live.view(-1, 1, 1), x, torch.zeros_like(x)))
        assert torch.equal(deq[live], x[live]), "the probe's K / V rows must be exact in the FP8 format"
        codes = codes.view(torch.uint8).clone()
        codes[~live], exps[~live] = 0x7F, 0xFF
        out += [codes.view(torch.float8_e4m3fn).permute(1, 0, 2).contiguous().to(DEV), exps.permute(1, 0).contiguous().to(DEV)]
    kc, ke, vc, ve = out
    return kc, vc, ke, ve


def _launcher(ops, inp, monkeypatch):
    """-> run(nsplit, fused) for the case's entry point, on device copies made once."""
    ep, sq, sk, cap, scale = inp["ep"], inp["sq"], inp["sk"], inp["cap"], inp["scale"]
    qd = inp["q"].to(DEV)
    if ep in ("fp8", "fp8_tail"):
        skc = sk - inp.get("n_tail", 0)
        kc, vc, ke, ve = _f8_layer(ops, inp, 0, cap if ep == "fp8" else skc + P.SPARE, sk if ep == "fp8" else skc)
        kt, vt = _head_major(inp["k"][skc:]), _head_major(inp["v"][skc:])

        def run(nsplit, fused):
            monkeypatch.setattr(ops, "ATTN_FUSED_MERGE", fused)
            if ep == "fp8":
                return ops.attn_decode_fp8(qd, kc, vc, ke, ve, sk, scale, nsplit=nsplit)
            return ops.attn_decode_fp8_tail(qd, kc, vc, ke, ve, kt, vt, skc, scale, n_tail=inp["n_tail"], nsplit=nsplit)
        return run
    if inp.get("skdev"):                                      # token-major view, key count from device memory, launch sized by cap
        kd, vd = inp["k"].to(DEV).permute(1, 0, 2), inp["v"].to(DEV).permute(1, 0, 2)
        skd = torch.tensor([sk], dtype=torch.int32, device=DEV)
    else:
        kd, vd, skd = _head_major(inp["k"]), _head_major(inp["v"]), None
    if ep == "decode":
        def run(nsplit, fused):
            monkeypatch.setattr(ops, "ATTN_FUSED_MERGE", fused)
            return ops.attn_decode(qd, kd, vd, cap if skd is not None else sk, scale, sk_dev=skd, nsplit=nsplit)
    elif ep == "decode_gqa":
        def run(nsplit, fused):
            return ops.attn_decode_gqa(qd, kd, vd, sk, scale, nsplit=nsplit, fused_merge=fused)
    elif ep == "block":
        def run(nsplit, fused):
            return ops.attn_block(qd, kd, vd, sk, scale, nsplit=nsplit)
    elif ep == "prefill":
        assert ops.hip.lib().tf_attn_prefill_pick_nsplit(inp["H"], sq, sk) == P.prefill_nsplit(inp["H"], sq, sk)

        def run(nsplit, fused):
            return ops.attn_prefill(qd, kd, vd, sk, scale)
    elif ep == "prefill_gqa":
        assert ops.hip.lib().tf_attn_prefill_pick_nsplit(inp["H"], sq, sk) == P.prefill_nsplit(inp["H"], sq, sk)

        def run(nsplit, fused):
            return ops.attn_prefill_gqa(qd, kd, vd, sk, scale)
    elif ep == "tree":
        bits = ops.pack_tree_mask(inp["mask"].to(DEV))

        def run(nsplit, fused):
            if nsplit is None:
                return ops.attn_tree(qd, kd, vd, sk, scale, bits, inp["prefix"], mask_row0=inp["row0"])
            return ops.attn_block(qd, kd, vd, sk, scale, nsplit=nsplit, tree_mask=bits, mask_row0=inp["row0"],
                                  tree_start=inp["prefix"])
    else:
        cos, sin = inp["cos"].to(DEV), inp["sin"].to(DEV)

        def run(nsplit, fused):
            return ops.attn_rope_on_read(qd, kd, vd, cos, sin, sk, scale)
    return run


MERGE_FORMS = ("decode", "decode_gqa", "fp8", "fp8_tail")      # entry points with a one- and a two-launch merge


def _probe(inp, monkeypatch, exact=True):
    ops = _ops()
    _t0.append(time.time())
    want = P.oracle(inp)
    run = _launcher(ops, inp, monkeypatch)
    for nsplit in inp["nsplits"]:
        what = f"{P.case_id(inp)} {inp['kind']} poison {inp['poison']} nsplit {nsplit}"
        got = run(nsplit, False)
        check(inp, got, want, what, exact=exact)
        if inp["ep"] in MERGE_FORMS:
            assert torch.equal(run(nsplit, True), got), f"{what}: the one-launch merge differs from the two-launch one"


def _quantize(c):
    return _ops().kv_quantize_ref if c["ep"] in ("fp8", "fp8_tail") else None


def _cases(ep):
    return pytest.mark.parametrize("c", P.CASES[ep], ids=P.case_id)


_modes = pytest.mark.parametrize("kind,parity,poison", P.MODES, ids=P.MODE_IDS)
_t0 = []                                                         # when the first probe of the file started


def _select(c, kind, parity, poison, monkeypatch):
    _probe(P.build(c, kind, parity, poison, quantize=_quantize(c)), monkeypatch)


@_modes
@_cases("decode")
def test_attn_decode_selects(c, kind, parity, poison, monkeypatch):
    """tf_attn_decode_act: one and two q-tiles, the eager and the long loop (4103 keys: nsplit 8 / 1), every split's first
    and last key, sk_dev below a launch bound of cap over a token-major view; both merge forms, bit-identical."""
    _select(c, kind, parity, poison, monkeypatch)


@_modes
@_cases("decode_gqa")
def test_attn_decode_gqa_selects(c, kind, parity, poison, monkeypatch):
    """tf_attn_decode_gqa_act: stacked rows across a q-tile, two sub-groups per KV head, gs = 1; every query head of a group has
    a target of its own, so h / g against h % g is a wrong KEY, not a tolerance."""
    _select(c, kind, parity, poison, monkeypatch)


@_modes
@_cases("fp8")
def test_attn_decode_fp8_selects(c, kind, parity, poison, monkeypatch):
    """tf_attn_decode_fp8_act: sign keys and their 1.5x decoys are exact e4m3 codes, V is a dequantised image."""
    _select(c, kind, parity, poison, monkeypatch)


@_modes
@_cases("fp8_tail")
def test_attn_decode_fp8_tail_selects(c, kind, parity, poison, monkeypatch):
    """tf_attn_decode_fp8_tail_act: targets on both sides of sk_codes, the edge decoys in the fp16 tail rows, poison codes past
    sk_codes and poison rows past n_tail."""
    _select(c, kind, parity, poison, monkeypatch)


@_modes
@_cases("block")
def test_attn_block_selects(c, kind, parity, poison, monkeypatch):
    """tf_attn_block: rg = 1 (32 rows), rg = 2 (33, 64) and the LDS kernel (65, 128); sk = sq, sq + 1, 640, 4103."""
    _select(c, kind, parity, poison, monkeypatch)


@_modes
@_cases("prefill")
def test_attn_prefill_selects(c, kind, parity, poison, monkeypatch):
    """tf_attn_prefill (one launch): a ragged last block, rows 127 | 128, splits wholly past a block's causal edge."""
    _select(c, kind, parity, poison, monkeypatch)


@_modes
@_cases("prefill_gqa")
def test_attn_prefill_gqa_selects(c, kind, parity, poison, monkeypatch):
    _select(c, kind, parity, poison, monkeypatch)


@_modes
@_cases("tree")
def test_attn_tree_selects(c, kind, parity, poison, monkeypatch):
    """tf_attn_block with a tree mask, one and two passes, mask_row0 zero and nonzero; decoys on non-ancestor columns below and
    above the row's own, columns 31 | 32 and 63 | 64 among targets and decoys."""
    _select(c, kind, parity, poison, monkeypatch)


@_modes
@_cases("rope")
def test_attn_rope_on_read_selects(c, kind, parity, poison, monkeypatch):
    """tf_attn_rope_on_read: q = BETA * the oracle's rotated key; the MFMA kernel (5, 259, 384 keys) and the scalar one (400)."""
    _select(c, kind, parity, poison, monkeypatch)


@pytest.mark.parametrize("c", P.SINK_CASES, ids=P.case_id)
def test_attention_sink_rows_match_oracle(c, monkeypatch):
    """Key 0 carries about half of every row's mass (what real checkpoints show): P spans 1 to far below it in one row.
    Assertions 1 and 2 only."""
    _probe(P.build_sink(c, quantize=_quantize(c)), monkeypatch, exact=False)


def test_zz_wall_time_of_this_file():
    if not _t0:                                                  # (run on its own: nothing to report)
        return
    Hh.note(f"attention probes: {time.time() - _t0[0]:.1f} s from the first probe to the last of the file")
