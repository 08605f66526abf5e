"""The wide grouped-query decode attention (tf_attn_decode_gqa_wide_act) on a real MI355X: all g query heads of
a KV head as one problem of g * sq <= 64 stacked rows.  Inputs, oracle and bounds are those of tests/test_gpu_gqa.py."""
import pytest
import torch

from oracle import ref_ops as R
from oracle import specs
from tests import attn_probes as P
from tests import helpers as Hh
from tests import test_gpu_gqa as G
from tests.test_gpu_gqa import DECODE_ATOL, DECODE_RTOL, DEV, _decode_inputs, _expand, _ops
from tests.test_gqa_cpu import gqa_state_dicts

pytestmark = pytest.mark.gpu

WIDE_SHAPES = [(7, 1, 128, 7),      # 49 rows: a head's rows straddle q-tile edges, the last q-tile is 1 row full
               (8, 1, 128, 8),      # 64: exactly full
               (8, 2, 64, 7),       # 56: two KV heads, D = 64
               (2, 1, 128, 17),     # 34: third q-tile 2 rows full, fourth all padding
               (5, 1, 128, 12),     # 60
               (8, 1, 64, 5)]       # 40


@pytest.mark.parametrize("sk_kind", ["sq", 33, 1031, 4103])
@pytest.mark.parametrize("H,Hkv,D,sq", WIDE_SHAPES)
def test_wide_decode_attention_matches_oracle_and_the_multi_head_bits(H, Hkv, D, sq, sk_kind):
    """Every split count the key count allows: the oracle on the expanded K / V, the one-launch merge twice against the
    two-launch one (ticket row zero afterwards), the multi-head kernel's bits on the repeated K / V, both output layouts."""
    ops = _ops()
    sk, g, scale = (sq if sk_kind == "sq" else sk_kind), H // Hkv, R.softmax_scale_for(D)
    q, k, v, kd, vd = _decode_inputs(H, Hkv, D, sq, sk)
    want = R.attn_kvcache(q, _expand(k, g, 1), _expand(v, g, 1), scale).reshape(sq, H * D).float()
    qd = q.to(DEV)
    ke, ve = _expand(kd, g, 0).contiguous(), _expand(vd, g, 0).contiguous()
    for nsplit in [n for n in (1, 3, 8, 9) if n <= (sk + 15) // 16] + [None]:
        two = ops.attn_decode_gqa_wide(qd, kd, vd, sk, scale, nsplit=nsplit, fused_merge=False)
        Hh.close(two.float().cpu(), want, what=f"gqa wide decode {H}/{Hkv} D{D} sq{sq} sk{sk} nsplit{nsplit}", atol=DECODE_ATOL,
                 rtol=DECODE_RTOL)
        for _ in range(2):                                    # the second call runs on the tickets the first one left
            assert torch.equal(ops.attn_decode_gqa_wide(qd, kd, vd, sk, scale, nsplit=nsplit, fused_merge=True), two)
        row = ops._ticket_row(qd.device, torch.cuda.current_stream().cuda_stream or 0)
        torch.cuda.synchronize()
        assert int(row.abs().sum()) == 0
        if nsplit is not None:
            assert torch.equal(two, ops.attn_decode(qd, ke, ve, sk, scale, nsplit=nsplit)), "not the multi-head kernel's bits"
        act = ops.Act.empty(sq, H * D, DEV, R=sq + 3)         # k-octet-major and row-major outputs: sentinel rows stay
        act.t.fill_(-7.0)
        ops.attn_decode_gqa_wide(qd, kd, vd, sk, scale, nsplit=nsplit, out=act)
        assert torch.equal(act.rows(), two) and bool((act.t[:, sq:] == -7.0).all())
        rows = torch.full((sq + 3, H * D), -7.0, dtype=torch.float16, device=DEV)
        ops.attn_decode_gqa_wide(qd, kd, vd, sk, scale, nsplit=nsplit, fused_merge=False, out=rows[:sq])
        assert torch.equal(rows[:sq], two) and bool((rows[sq:] == -7.0).all())


@pytest.mark.parametrize("H,Hkv,D,sq", [(7, 1, 128, 7), (8, 2, 64, 7), (2, 1, 128, 17)])
def test_wide_device_key_count_and_token_major_cache(H, Hkv, D, sq):
    """sk_dev = 777 under a launch bound of 1024 (the captured forward's form) over a token-major cache view."""
    ops = _ops()
    sk, cap, g, scale = 777, 1024, H // Hkv, R.softmax_scale_for(D)
    q, k, v, _, _ = _decode_inputs(H, Hkv, D, sq, sk, cap=cap)
    kd, vd = k.to(DEV).permute(1, 0, 2), v.to(DEV).permute(1, 0, 2)            # (Hkv, T, D) views of [T][Hkv][D] storage
    want = R.attn_kvcache(q, _expand(k[:sk], g, 1), _expand(v[:sk], g, 1), scale).reshape(sq, H * D).float()
    skd = torch.tensor([sk], dtype=torch.int32, device=DEV)
    for fused in (False, True):
        got = ops.attn_decode_gqa_wide(q.to(DEV), kd, vd, cap, scale, sk_dev=skd, nsplit=4, fused_merge=fused)
        Hh.close(got.float().cpu(), want, what=f"gqa wide decode sk_dev {H}/{Hkv} sq{sq}", atol=DECODE_ATOL, rtol=DECODE_RTOL)


@pytest.mark.parametrize("H,Hkv,sq,knob,want", [(7, 1, 7, True, (1, 0)), (4, 1, 7, True, (0, 1)), (8, 1, 9, True, (0, 1)),
                                                (7, 1, 7, False, (0, 1)), (8, 1, 7, False, (0, 1))])
def test_attn_decode_dispatch(H, Hkv, sq, knob, want, monkeypatch):
    """(wide, stacked) launches of one ops.attn_decode call: the wide kernel where the stacked one would re-read K / V and the
    rows fit 64; with TRIFORCE_GQA_WIDE=0 (ops.GQA_WIDE) the stacked kernel everywhere."""
    ops = _ops()
    L, n = ops.hip.lib(), []
    monkeypatch.setattr(ops, "GQA_WIDE", knob)
    for name in ("tf_attn_decode_gqa_wide_act", "tf_attn_decode_gqa_act"):
        monkeypatch.setattr(L, name, lambda *a, _f=getattr(L, name), _n=name: (n.append(_n), _f(*a))[1])
    q, _, _, kd, vd = _decode_inputs(H, Hkv, 128, sq, 333)
    ops.attn_decode(q.to(DEV), kd, vd, 333, R.softmax_scale_for(128))
    torch.cuda.synchronize()
    assert (n.count("tf_attn_decode_gqa_wide_act"), n.count("tf_attn_decode_gqa_act")) == want


def test_wide_entry_point_gates():
    ops = _ops()
    buf = torch.zeros(1 << 16, dtype=torch.float16, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    L, p, w, s = ops.hip.lib(), ops._ptr(buf), ops._ptr(ws), ops._stream()

    def call(H, Hkv, D, sq, ws_floats=ws.numel()):
        return L.tf_attn_decode_gqa_wide_act(p, p, p, p, H * D, 8, D, 4096, sq, 16, None, H, Hkv, D, 0.1, 1, w, ws_floats, None, s)
    assert [call(13, 1, 128, 5), call(1, 1, 128, 33), call(4, 2, 96, 7), call(8, 3, 128, 2)] == [-22] * 4      # g * sq = 65, ...
    need = L.tf_attn_decode_ws_floats(1, 49, 128, 1)
    assert call(7, 1, 128, 7, need - 1) == -28 and call(7, 1, 128, 7, need) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind,parity,poison", P.MODES, ids=P.MODE_IDS)
@pytest.mark.parametrize("H,Hkv,sk", [(7, 1, 333), (7, 1, 4103), (8, 2, 333), (8, 2, 4103)])
def test_wide_selects(H, Hkv, sk, kind, parity, poison):
    """One-hot probes at 7 rows: every query head of a group has a target key of its own, so a wrong head -> KV-head map or
    a wrong causal edge is a wrong KEY, not a tolerance."""
    ops = _ops()
    inp = P.build(P.case("decode_gqa", 7, sk, H=H, Hkv=Hkv, nsplits=(1, 3, None)), kind, parity, poison)
    want = P.oracle(inp)
    qd = inp["q"].to(DEV)
    kd, vd = (inp[n].permute(1, 0, 2).contiguous().to(DEV) for n in ("k", "v"))
    for nsplit in inp["nsplits"]:
        what = f"wide {P.case_id(inp)} {kind} poison {poison} nsplit {nsplit}"
        got = ops.attn_decode_gqa_wide(qd, kd, vd, sk, inp["scale"], nsplit=nsplit, fused_merge=False)
        P.check(inp, got, want, DECODE_ATOL, DECODE_RTOL, Hh.close, what=what)
        assert torch.equal(ops.attn_decode_gqa_wide(qd, kd, vd, sk, inp["scale"], nsplit=nsplit, fused_merge=True), got), what


def test_greedy_triforce_7_over_1_heads_matches_the_expanded_oracle(monkeypatch):
    """zoo "tiny-gqa" at 7 query heads over 1 KV head (hidden 896; 4 096 positions, as test_gpu_gqa's case): the 7- and 8-row
    verifies stack 49 and 56 rows.  Greedy TriForce, graphs on, 32 tokens, teacher-forced through the expanded-weight oracle."""
    from triforce_amd.models import zoo
    from triforce_amd.utils.decoding import TriForceRunner
    g = G._case(gen_len=64)
    g["tcfg"] = dict(zoo.CONFIGS["tiny-gqa"], num_attention_heads=7, num_key_value_heads=7, hidden_size=896,
                     vocab_size=g["tcfg"]["vocab_size"], max_position_embeddings=4096)
    dsd = specs.random_state_dict(g["dcfg"], g["dseed"], head_std=g["head_std"])
    monkeypatch.setitem(G._WEIGHTS, "w", gqa_state_dicts(g["tcfg"], g["tseed"], 1) + (dsd,))     # what G._product / G._oracle draw from
    ge = G._product(g, graphs=True)
    prompt = Hh.prompt_of(g)
    tok = Hh.FakeTokenizer()
    tok.eos_token_id = -1
    run = TriForceRunner(tok, ge, g["gamma"], top_k=-1, top_p=g["top_p"], temperature=g["temperature"])
    run.prefill(prompt.to(DEV))
    while run.n < 32:
        run.step()
    assert len(run.emitted) >= 33 and (run.accepted_count > 0 or run.resample_count > 0)
    G._check_stream("wide 7 / 1 triforce", g, prompt, list(run.emitted))
