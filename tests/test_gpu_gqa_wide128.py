"""The 128-row grouped-query decode attention (tf_attn_decode_gqa_wide128_act) on a real MI355X.  Inputs,
oracle and bounds are those of tests/test_gpu_gqa.py; bit equality with the multi-head kernel is not in this kernel's contract."""
import pytest
import torch

from oracle import ref_ops as R
from oracle import specs
from tests import attn_probes as P
from tests import helpers as Hh
from tests import test_gpu_gqa as G
from tests.test_gpu_gqa import DECODE_ATOL, DECODE_RTOL, DEV, _decode_inputs, _expand
from tests.test_gqa_cpu import gqa_state_dicts
from triforce_amd import ops

pytestmark = pytest.mark.gpu
ENTRY = "tf_attn_decode_gqa_wide128_act"


# stacked rows: 65 (the first past the 64-row kernel), 68, 72 (two KV heads), 112, 119 (last q-tile 7 rows full), 128 (full)
@pytest.mark.parametrize("H,Hkv,D,sq", [(13, 1, 128, 5), (4, 1, 128, 17), (8, 2, 128, 9), (16, 1, 128, 7), (7, 1, 64, 17), (16, 1, 64, 8)])
@pytest.mark.parametrize("sk_kind", ["sq", 33, 1031, 4103])
def test_wide128_decode_attention_matches_oracle(H, Hkv, D, sq, sk_kind):
    """Per split count: the oracle on the expanded K / V, one-launch merge twice = two-launch merge, tickets zero, both layouts."""
    sk, g, scale = (sq if sk_kind == "sq" else sk_kind), H // Hkv, R.softmax_scale_for(D)
    q, k, v, kd, vd = _decode_inputs(H, Hkv, D, sq, sk)
    want, qd = R.attn_kvcache(q, _expand(k, g, 1), _expand(v, g, 1), scale).reshape(sq, H * D).float(), q.to(DEV)
    for nsplit in [n for n in (1, 3, 8, 9) if n <= (sk + 15) // 16] + [None]:
        two = ops.attn_decode_gqa_wide128(qd, kd, vd, sk, scale, nsplit=nsplit, fused_merge=False)
        Hh.close(two.float().cpu(), want, what=f"wide128 {H}/{Hkv} D{D} sq{sq} sk{sk} nsplit{nsplit}", atol=DECODE_ATOL, rtol=DECODE_RTOL)
        for _ in range(2):                                    # the second call runs on the tickets the first one left
            assert torch.equal(ops.attn_decode_gqa_wide128(qd, kd, vd, sk, scale, nsplit=nsplit, fused_merge=True), two)
        torch.cuda.synchronize()
        assert int(ops._ticket_row(qd.device, torch.cuda.current_stream().cuda_stream or 0).abs().sum()) == 0
        act = ops.Act.empty(sq, H * D, DEV, R=sq + 3)         # k-octet-major and row-major outputs: sentinel rows stay
        act.t.fill_(-7.0)
        ops.attn_decode_gqa_wide128(qd, kd, vd, sk, scale, nsplit=nsplit, out=act)
        assert torch.equal(act.rows(), two) and bool((act.t[:, sq:] == -7.0).all())
        rows = torch.full((sq + 3, H * D), -7.0, dtype=torch.float16, device=DEV)
        ops.attn_decode_gqa_wide128(qd, kd, vd, sk, scale, nsplit=nsplit, fused_merge=False, out=rows[:sq])
        assert torch.equal(rows[:sq], two) and bool((rows[sq:] == -7.0).all())


@pytest.mark.parametrize("H,Hkv,D,sq", [(16, 1, 128, 7), (8, 2, 128, 9), (7, 1, 64, 17)])
def test_wide128_device_key_count_and_token_major_cache(H, Hkv, D, sq):
    sk, cap, g, scale = 777, 1024, H // Hkv, R.softmax_scale_for(D)
    q, k, v, _, _ = _decode_inputs(H, Hkv, D, sq, sk, cap=cap)
    kd, vd = k.to(DEV).permute(1, 0, 2), v.to(DEV).permute(1, 0, 2)            # (Hkv, T, D) views of [T][Hkv][D] storage
    want = R.attn_kvcache(q, _expand(k[:sk], g, 1), _expand(v[:sk], g, 1), scale).reshape(sq, H * D).float()
    for fused in (False, True):
        skd = torch.tensor([sk], dtype=torch.int32, device=DEV)
        got = ops.attn_decode_gqa_wide128(q.to(DEV), kd, vd, cap, scale, sk_dev=skd, nsplit=4, fused_merge=fused)
        Hh.close(got.float().cpu(), want, what=f"gqa wide128 decode sk_dev {H}/{Hkv} sq{sq}", atol=DECODE_ATOL, rtol=DECODE_RTOL)


@pytest.mark.parametrize("kind,parity,poison", P.MODES, ids=P.MODE_IDS)
@pytest.mark.parametrize("sk", [333, 4103])
@pytest.mark.parametrize("H,Hkv,sq", [(16, 1, 8), (14, 1, 9), (8, 2, 9)])
def test_wide128_selects(H, Hkv, sq, sk, kind, parity, poison):
    """One-hot probes.  16 heads x 9 rows = 144 stacked rows is past the kernel: 16 heads run at 8 rows (128), 9 rows at 14 heads."""
    inp = P.build(P.case("decode_gqa", sq, sk, H=H, Hkv=Hkv, nsplits=(1, 3, None)), kind, parity, poison)
    want, qd = P.oracle(inp), inp["q"].to(DEV)
    kd, vd = (inp[n].permute(1, 0, 2).contiguous().to(DEV) for n in ("k", "v"))
    for nsplit in inp["nsplits"]:
        what = f"wide128 {P.case_id(inp)} {kind} poison {poison} nsplit {nsplit}"
        got = ops.attn_decode_gqa_wide128(qd, kd, vd, sk, inp["scale"], nsplit=nsplit, fused_merge=False)
        P.check(inp, got, want, DECODE_ATOL, DECODE_RTOL, Hh.close, what=what)
        assert torch.equal(ops.attn_decode_gqa_wide128(qd, kd, vd, sk, inp["scale"], nsplit=nsplit, fused_merge=True), got), what


def test_wide128_entry_point_gates():
    buf, ws = torch.zeros(1 << 17, dtype=torch.float16, device=DEV), torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    L, p, w, s = ops.hip.lib(), ops._ptr(buf), ops._ptr(ws), ops._stream()
    def call(H, Hkv, D, sq, ws_floats=ws.numel(), st=None, nsplit=1, q=p):
        return getattr(L, ENTRY)(q, p, p, p, H * D, 8, st or D, 4096, sq, 16, None, H, Hkv, D, 0.1, nsplit, w, ws_floats, None, s)
    # NULL q, 33 rows per head, 129 stacked rows, H % Hkv, D = 96, a stride of 4 halves, 0 and 129 splits
    assert [call(4, 1, 128, 7, q=None), call(1, 1, 128, 33), call(43, 1, 128, 3), call(8, 3, 128, 2), call(4, 2, 96, 7),
            call(4, 1, 128, 7, st=132), call(4, 1, 128, 7, nsplit=0), call(4, 1, 128, 7, nsplit=129)] == [-22] * 8
    need = L.tf_attn_decode_ws_floats(1, 65, 128, 1)
    assert [call(13, 1, 128, 5, need - 1), call(13, 1, 128, 5, need), call(7, 1, 128, 7)] == [-28, 0, 0]     # (49 rows are accepted)


@pytest.mark.parametrize("H,Hkv,sq,rows,want", [(8, 1, 9, 128, (1, 0, 0)), (16, 1, 7, 128, (1, 0, 0)), (7, 1, 7, 128, (0, 1, 0)),
                                                (8, 1, 9, 64, (0, 0, 1)), (16, 1, 7, 64, (0, 0, 1)), (7, 1, 7, 64, (0, 1, 0))])
def test_attn_decode_dispatch(H, Hkv, sq, rows, want, monkeypatch):
    """(128-row, 64-row, stacked) launches of one ops.attn_decode call under ops.GQA_WIDE_ROWS = 128 and under the default."""
    L, n = ops.hip.lib(), []
    monkeypatch.setattr(ops, "GQA_WIDE_ROWS", rows)
    names = (ENTRY, "tf_attn_decode_gqa_wide_act", "tf_attn_decode_gqa_act")
    for name in names:
        monkeypatch.setattr(L, name, lambda *a, _f=getattr(L, name), _n=name: (n.append(_n), _f(*a))[1])
    q, _, _, kd, vd = _decode_inputs(H, Hkv, 128, sq, 333)
    ops.attn_decode(q.to(DEV), kd, vd, 333, R.softmax_scale_for(128))
    torch.cuda.synchronize()
    assert tuple(n.count(name) for name in names) == want


def test_greedy_triforce_16_over_1_heads_matches_the_expanded_oracle(monkeypatch):
    """zoo "tiny-gqa16" at 4 096 positions under the knob (verifies of 112 and 128 rows): greedy, graphs on, 32 tokens."""
    from triforce_amd.models import zoo
    from triforce_amd.utils.decoding import TriForceRunner
    monkeypatch.setattr(ops, "GQA_WIDE_ROWS", 128)
    g = G._case(gen_len=64)
    g["tcfg"] = dict(zoo.CONFIGS["tiny-gqa16"], num_key_value_heads=16, vocab_size=g["tcfg"]["vocab_size"], max_position_embeddings=4096)
    dsd = specs.random_state_dict(g["dcfg"], g["dseed"], head_std=g["head_std"])
    monkeypatch.setitem(G._WEIGHTS, "w", gqa_state_dicts(g["tcfg"], g["tseed"], 1) + (dsd,))     # what G._product / G._oracle draw from
    ge = G._product(g, graphs=True)
    prompt, tok = Hh.prompt_of(g), Hh.FakeTokenizer()
    tok.eos_token_id = -1
    run = TriForceRunner(tok, ge, g["gamma"], top_k=-1, top_p=g["top_p"], temperature=g["temperature"])
    run.prefill(prompt.to(DEV))
    while run.n < 32:
        run.step()
    assert len(run.emitted) >= 33 and (run.accepted_count > 0 or run.resample_count > 0)
    G._check_stream("wide128 16 / 1 triforce", g, prompt, list(run.emitted))
