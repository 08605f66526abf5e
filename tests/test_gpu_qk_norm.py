"""QK norm on the device: tf_qk_norm_rope_append and the models that run through it.

Exact probes.  Inputs are multiples of 2^-4 with |x| <= 8: the D squares sum exactly in fp32 in any order (at most 2^21
units of 2^-8; tests/test_qk_norm_cpu.py checks the premise), and everything after the sum is a fixed sequence of correctly
rounded fp32 / fp16 operations, so the QK NORM contract (include/triforce_hip.h) leaves no freedom: torch.equal against
ops.qk_norm_rope_ref evaluated on the CPU.  Norm weights are multiples of 2^-3 in [0.5, 4], positions are scattered over a
4096-row table (position 0 included), the caches and the row padding are pre-filled with a sentinel.  A sub-family with eps = 0 and a mean
square that is a power of 4 has an exact inv in any implementation: it separates a divide / sqrt rounding difference from
everything else.

Random data against the bound tests/test_gpu_ops.py gives tf_rmsnorm, the TF_EINVAL gates, and the model: logits of
tiny-qknorm / tiny-gqa-qknorm against the fp64 truth with the CPU restatement's own deviation as the yardstick, greedy
TriForce (eager, captured, extend, TRIFORCE_FUSE=none, FP8 KV cache) teacher-forced through QkNormOracleTarget, and the
launch list of a norm-free model.
"""
import collections

import pytest
import torch

from oracle import ref_model as M
from oracle import ref_ops as R
from oracle import specs
from tests import helpers as Hh
from tests import qk_norm_ref as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP_TOL = 8e-3                                   # tests/test_gpu_gqa.py
SENTINEL = -777.0
TABLE = 4096
EPS = 1e-6
SHAPES = [(2, 2, 128), (4, 2, 128), (8, 1, 128), (4, 4, 64), (4, 2, 64)]
ROWS = [1, 7, 17, 32, 130]


def _ops():
    from triforce_amd import ops
    return ops


_TABLES = {}


def _tables(D):
    if D not in _TABLES:
        _TABLES[D] = R.rope_tables_plain(D, TABLE, 1e6)
    return _TABLES[D]


def _material(H, Hkv, D, rows, seed, pow4=False, one_hot=None):
    """(qkv rows with ``pad`` extra columns of sentinel behind each row, qn, kn, positions): exact-sum inputs."""
    gen = torch.Generator().manual_seed(seed)
    N = (H + 2 * Hkv) * D
    if pow4:                        # every element of a head +-2^k: mean square 4^k, inv = 2^-k exactly (eps = 0)
        k = torch.randint(-2, 4, (rows, H + 2 * Hkv, 1), generator=gen).float()
        sign = torch.randint(0, 2, (rows, H + 2 * Hkv, D), generator=gen).float() * 2 - 1
        x = (sign * torch.exp2(k)).reshape(rows, N)
    else:
        x = torch.randint(-128, 129, (rows, N), generator=gen).float() / 16
    if one_hot is not None:         # only query head ``one_hot`` is non-zero
        keep = torch.zeros(N, dtype=torch.bool)
        keep[one_hot * D:(one_hot + 1) * D] = True
        keep[H * D:] = True
        x = x * keep
    qn, kn = (torch.randint(4, 33, (D,), generator=gen).float() / 8 for _ in range(2))
    pos = torch.randperm(TABLE, generator=gen)[:rows].contiguous()
    pos[0] = 0
    return x.half(), qn.half(), kn.half(), pos


def _first_diff(a, b):
    ne = (a != b).nonzero()
    return None if ne.numel() == 0 else tuple(int(i) for i in ne[0])


def _run(ops, x, qn, kn, pos, H, Hkv, D, eps, rotate_k, slot_dev, pad, token_major, slot=5, tail=3):
    """Launch the kernel into sentinel-filled outputs; -> (q, k cache, v cache) on the CPU, caches as (Hkv, T, D)."""
    rows, N = x.shape
    cos, sin = _tables(D)
    buf = torch.full((rows, N + pad), SENTINEL, dtype=torch.float16, device=DEV)
    buf[:, :N] = x.to(DEV)
    T = slot + rows + tail
    if token_major:
        kc, vc = (torch.full((T, Hkv, D), SENTINEL, dtype=torch.float16, device=DEV).permute(1, 0, 2) for _ in range(2))
    else:
        kc, vc = (torch.full((Hkv, T, D), SENTINEL, dtype=torch.float16, device=DEV) for _ in range(2))
    sd = torch.tensor([slot], dtype=torch.int32, device=DEV) if slot_dev else None
    q = ops.qk_norm_rope_append(buf[:, :N], qn.to(DEV), kn.to(DEV), eps, cos.to(DEV), sin.to(DEV), pos.to(DEV), kc, vc,
                                0 if slot_dev else slot, H, D, rotate_k=rotate_k, slot0_dev=sd, Hkv=Hkv)
    torch.cuda.synchronize()
    assert bool((buf[:, N:] == SENTINEL).all()) and torch.equal(buf[:, :N].cpu(), x), "the input rows were written"
    return q.cpu(), kc.cpu(), vc.cpu()


def _check(ops, where, x, qn, kn, pos, H, Hkv, D, eps, rotate_k, got, slot=5):
    rows = x.shape[0]
    cos, sin = _tables(D)
    wq, wk, wv = ops.qk_norm_rope_ref(x, qn, kn, eps, cos, sin, pos, H, D, rotate_k=rotate_k, Hkv=Hkv)
    q, kc, vc = got
    idx = _first_diff(q, wq)
    assert idx is None, f"{where}: q (row, head, d) {idx}: got {float(q[idx])}, expected {float(wq[idx])}"
    for name, cache, want_rows in (("k", kc, wk), ("v", vc, wv)):
        want = torch.full(tuple(cache.shape), SENTINEL, dtype=torch.float16)
        want[:, slot:slot + rows] = want_rows.permute(1, 0, 2)
        idx = _first_diff(cache, want)
        assert idx is None, f"{where}: {name} cache (head, slot, d) {idx}: got {float(cache[idx])}, expected {float(want[idx])}"


# ---- exact probes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("H,Hkv,D", SHAPES)
def test_exact_probe(H, Hkv, D, rows):
    ops = _ops()
    x, qn, kn, pos = _material(H, Hkv, D, rows, seed=1000 * H + 10 * D + rows)
    n = 0
    for rotate_k in (True, False):
        for slot_dev in (False, True):
            for pad, token_major in ((0, False), (24, True), (8, False), (0, True)):
                where = f"H{H} Hkv{Hkv} D{D} rows{rows} rotate_k={rotate_k} slot_dev={slot_dev} pad={pad} token_major={token_major}"
                got = _run(ops, x, qn, kn, pos, H, Hkv, D, EPS, rotate_k, slot_dev, pad, token_major)
                _check(ops, where, x, qn, kn, pos, H, Hkv, D, EPS, rotate_k, got)
                n += 1
    assert n == 16


@pytest.mark.parametrize("H,Hkv,D", SHAPES)
def test_exact_probe_with_an_exact_inverse(H, Hkv, D):
    """eps = 0 and a mean square of 4^k: inv = 2^-k whatever rounds the divide and the square root.  If test_exact_probe fails
    where this passes, the divide / sqrt rounding of the build is the first suspect."""
    ops = _ops()
    for rows in (7, 130):
        x, qn, kn, pos = _material(H, Hkv, D, rows, seed=77 + rows + D, pow4=True)
        for rotate_k in (True, False):
            got = _run(ops, x, qn, kn, pos, H, Hkv, D, 0.0, rotate_k, rotate_k, 8, not rotate_k)
            _check(ops, f"pow4 H{H} Hkv{Hkv} D{D} rows{rows} rotate_k={rotate_k}", x, qn, kn, pos, H, Hkv, D, 0.0, rotate_k, got)


@pytest.mark.parametrize("H,Hkv,D", SHAPES)
def test_one_hot_query_heads_do_not_leak(H, Hkv, D):
    ops = _ops()
    rows = 17
    for h in range(H):
        x, qn, kn, pos = _material(H, Hkv, D, rows, seed=500 + h, one_hot=h)
        got = _run(ops, x, qn, kn, pos, H, Hkv, D, EPS, True, False, 0, False)
        _check(ops, f"one-hot head {h} of H{H} Hkv{Hkv} D{D}", x, qn, kn, pos, H, Hkv, D, EPS, True, got)
        q = got[0]
        others = [j for j in range(H) if j != h]
        assert bool(q[:, h].any()) and not bool(q[:, others].any()), f"query head {h} leaked into a neighbour"


# ---- random data ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hkv,D,rows", [(2, 2, 128, 7), (4, 2, 128, 130), (4, 2, 64, 33), (32, 8, 128, 17)])
def test_random_rows_within_the_rmsnorm_bound(H, Hkv, D, rows):
    """N(0,1) rows, weights 1 + 0.1 N(0,1), every position 0: cos = 1 and sin = 0 exactly, so the rotation is the identity
    and the output is the normalised value.  The device sums the squares in another order than the CPU: the bound
    tests/test_gpu_ops.py gives tf_rmsnorm for that (<= 2 fp16 ulp on <= 1 % of the elements).  v is copied: bit-equal."""
    from tests.test_gpu_ops import ulp_report
    ops = _ops()
    gen = torch.Generator().manual_seed(H * D + rows)
    x = torch.randn(rows, (H + 2 * Hkv) * D, generator=gen).half()
    qn, kn = ((1 + 0.1 * torch.randn(D, generator=gen)).half() for _ in range(2))
    pos = torch.zeros(rows, dtype=torch.int64)
    cos, sin = _tables(D)
    assert bool((cos[0] == 1).all()) and not bool(sin[0].any())
    q, kc, vc = _run(ops, x, qn, kn, pos, H, Hkv, D, EPS, True, False, 0, False)
    wq = R.rms_norm(x[:, :H * D].reshape(rows, H, D), qn, EPS)
    wk = R.rms_norm(x[:, H * D:(H + Hkv) * D].reshape(rows, Hkv, D), kn, EPS)
    ulp_report(f"qk_norm q H{H} Hkv{Hkv} D{D} rows{rows}", q, wq, max_ulp_frac=1e-2, ulps=2)
    ulp_report(f"qk_norm k H{H} Hkv{Hkv} D{D} rows{rows}", kc[:, 5:5 + rows].permute(1, 0, 2), wk, max_ulp_frac=1e-2, ulps=2)
    assert torch.equal(vc[:, 5:5 + rows].permute(1, 0, 2).reshape(rows, -1), x[:, (H + Hkv) * D:])


def test_a_prefill_chunk_of_4096_rows():
    """The largest row count the path launches (one prefill chunk): exact material, every row checked."""
    ops = _ops()
    H, Hkv, D, rows = 4, 2, 128, 4096
    x, qn, kn, pos = _material(H, Hkv, D, rows, seed=4096)
    got = _run(ops, x, qn, kn, pos, H, Hkv, D, EPS, True, False, 0, False)
    _check(ops, "4096 rows", x, qn, kn, pos, H, Hkv, D, EPS, True, got)


# ---- gates ------------------------------------------------------------------------------------------------------------------------
def test_entry_point_returns_einval():
    ops = _ops()
    L = ops.hip.lib()
    buf = torch.zeros(1 << 16, dtype=torch.float16, device=DEV)
    pos = torch.zeros(8, dtype=torch.int64, device=DEV)
    p, ps, s = ops._ptr(buf), ops._ptr(pos), ops._stream()
    odd = ops._ptr(buf[1:])                                                             # 2-byte aligned

    def call(qkv=p, cos=p, sin=p, positions=ps, q=p, k=p, v=p, rows=1, H=2, Hkv=1, D=128, qn=p, kn=p, eps=1e-6):
        return L.tf_qk_norm_rope_append(qkv, (H + 2 * Hkv) * D, cos, sin, positions, q, k, v, D, 4096, 0, None, rows, H, Hkv, D, 1,
                                        qn, kn, eps, s)
    assert call() == 0 and call(D=64) == 0 and call(H=2, Hkv=2) == 0                    # the call is otherwise well formed
    for name in ("qkv", "cos", "sin", "positions", "q", "k", "v", "qn", "kn"):
        assert call(**{name: None}) == -22, name                                        # NULL buffers
    assert call(D=96) == -22 and call(D=256) == -22 and call(D=32) == -22               # D outside {64, 128}
    assert call(H=3, Hkv=2) == -22 and call(H=0) == -22 and call(Hkv=0) == -22          # H % Hkv, the neighbour's head gates
    assert call(H=65536, Hkv=65536) == -22
    assert call(qn=odd) == -22 and call(kn=odd) == -22                                  # misaligned norm weights
    assert call(rows=-1) == -22 and call(eps=-1.0) == -22
    buf.fill_(SENTINEL)
    assert call(rows=0) == 0                                                            # a no-op after the gates
    assert call(rows=0, D=96) == -22
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()), "rows == 0 wrote something"


# ---- model ------------------------------------------------------------------------------------------------------------------------
ZOO = ["tiny-qknorm", "tiny-gqa-qknorm"]
_W = {}


def _weights(name):
    if name not in _W:                                       # drawn once, shared, left unchanged
        g = Q.zoo_case(name, gen_len=160)                    # (capacity for the stream, one chat turn and its answer)
        _W[name] = (g,) + Q.zoo_state_dicts(g)
    return _W[name]


def _product(name, graphs, **kw):
    g, sd, _, dsd = _weights(name)
    return Hh.build_product(g, DEV, sd, dsd, graphs=graphs, **kw)


@pytest.mark.parametrize("name", ZOO)
def test_model_logits_within_the_restatements_own_error(name):
    """A 128-token prefill chunk, then 7 decode rows, eager and captured.  Truth: the fp64 evaluation of the stored weights
    (tests/qk_norm_ref.forward_fp64, pinned against transformers' Qwen3).  Yardstick: the CPU restatement's deviation from it.
    Device: within 2 x its max and 1.25 x its mean (the margins of tests/test_gpu_attn_bias.py)."""
    g, sd, esd, dsd = _weights(name)
    ge = _product(name, graphs=True)
    W = ge.engine.model.weights
    assert W.qk_norm and W.wqkv[0].wp_rope is None and W.wqkv[0].wp is not None
    prompt = specs.random_prompt(g["tcfg"]["vocab_size"], 128, g["pseed"])
    rows = torch.randint(3, g["tcfg"]["vocab_size"], (1, 7), generator=torch.Generator().manual_seed(7))
    truth = Q.forward_fp64(g["tcfg"], sd, torch.cat([prompt, rows], dim=1)[0])
    t_pre, t_dec = truth[127], truth[128:]
    ot, okv = Q.QkNormOracleTarget(g["ecfg"], esd), M.FullCache(g["ecfg"], 256)
    o_pre = ot.forward(prompt, okv, None)[0, -1].double()
    o_dec = ot.forward(rows, okv, None)[0].double()
    kvc = ge.engine.kv_cache
    kvc.reset()
    d_pre = ge.inference(prompt.to(DEV))[0, -1].double().cpu()
    S = kvc.seq_len
    assert S == 128
    eager = ge.inference(rows.to(DEV), eager=True)[0].double().cpu()
    kvc.seq_len = S
    captured = ge.inference(rows.to(DEV))[0].double().cpu()
    kvc.seq_len = S
    for what, dev, ora, tru in (("prefill chunk, last row", d_pre, o_pre, t_pre), ("7 decode rows, eager", eager, o_dec, t_dec),
                                ("7 decode rows, captured", captured, o_dec, t_dec)):
        y, d = (ora - tru).abs(), (dev - tru).abs()
        ymax, ymean, dmax, dmean = float(y.max()), float(y.mean()), float(d.max()), float(d.mean())
        print(f"[qk-norm] {name} {what}: restatement max {ymax:.3e} mean {ymean:.3e} | device max {dmax:.3e} mean {dmean:.3e}")
        ok_max = Hh.bound(f"qk norm {name} {what}: max |dlogit| vs fp64 (limit 2 x restatement)", dmax, 2.0 * ymax)
        ok_mean = Hh.bound(f"qk norm {name} {what}: mean |dlogit| vs fp64 (limit 1.25 x restatement)", dmean, 1.25 * ymean)
        assert ok_max and ok_mean, (name, what, dict(restatement=(ymax, ymean), device=(dmax, dmean)))
    # captured vs eager: the captured attention is sized by the cache capacity, another split-KV partition and so another
    # fp32 summation order — the bound tests/test_gpu_e2e.py puts on exactly that (two fp16 spacings of the largest logit)
    from tests.test_gpu_e2e import _logit_check
    _logit_check(f"qk norm {name}: captured vs eager decode rows", captured.float(), eager.float())


def _check_stream(what, name, prompt, stream):
    g, _, esd, _ = _weights(name)
    ot, okv = Q.QkNormOracleTarget(g["ecfg"], esd), M.FullCache(g["ecfg"], prompt.shape[1] + len(stream) + 8)
    logits = ot.forward(prompt, okv, None)[0, -1]           # (as tests/test_gpu_gqa.py _gaps, through the QK-norm oracle)
    gaps = [float(logits.max() - logits[stream[0]])]
    for i in range(len(stream) - 1):
        logits = ot.forward(torch.tensor([[stream[i]]]), okv, None)[0, -1]
        gaps.append(float(logits.max() - logits[stream[i + 1]]))
    worst = max(gaps)
    Hh.record("bound", worst / GAP_TOL, what=f"qk norm {name} {what}: worst teacher-forced gap", value=worst, limit=GAP_TOL)
    assert worst < GAP_TOL, f"{what}: token {gaps.index(worst)} trails the QK-norm oracle's argmax by {worst:.4f} logit"
    exact = sum(1 for x in gaps if x == 0.0)
    assert exact >= len(gaps) - 3, f"{what}: only {exact}/{len(gaps)} tokens are the QK-norm oracle's exact argmax"


def _run_triforce(ge, g, prompt, n):
    from triforce_amd.utils.decoding import TriForceRunner
    tok = Hh.FakeTokenizer()
    tok.eos_token_id = -1
    run = TriForceRunner(tok, ge, g["gamma"], top_k=-1, top_p=g["top_p"], temperature=g["temperature"])
    run.prefill(prompt.to(DEV))
    while run.n < n:
        run.step()
    return run


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("name", ZOO)
def test_greedy_triforce_and_extend_follow_the_qk_norm_oracle(name, graphs):
    g = _weights(name)[0]
    ge = _product(name, graphs=graphs)
    prompt = Hh.prompt_of(g)
    run = _run_triforce(ge, g, prompt, 32)
    stream = list(run.emitted)
    assert len(stream) >= 33
    _check_stream(f"triforce graphs={graphs}", name, prompt, stream)
    if graphs:
        turn = torch.randint(3, g["tcfg"]["vocab_size"], (1, 64), generator=torch.Generator().manual_seed(77))
        run.extend(turn.to(DEV))
        history = torch.cat([prompt, torch.tensor([stream]), turn], dim=1)
        assert torch.equal(run.history.cpu(), history) and run.n == 0
        while run.n < 12:
            run.step()
        _check_stream("extend", name, history, list(run.emitted))


def _count_calls(ops, monkeypatch):
    """Every call through hip.lib() by name."""
    L, calls = ops.hip.lib(), collections.Counter()
    for fn_name in ops.hip.SIGNATURES:
        real = getattr(L, fn_name)

        def wrapped(*a, _real=real, _name=fn_name):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(L, fn_name, wrapped)
    return calls


def test_unfused_layer_follows_the_qk_norm_oracle(monkeypatch):
    """TRIFORCE_FUSE=none: q|k|v through the plain GEMM, then tf_qk_norm_rope_append in tf_rope_append's place."""
    ops = _ops()
    monkeypatch.setattr(ops, "FUSE_MODE", "none")
    calls = _count_calls(ops, monkeypatch)
    counted = ops.hip.lib().tf_rope_append
    target_heads = []                                # tf_rope_append calls with the TARGET's head width (argument 14 = D)

    def rope_append(*a):
        if a[14] == 128:                             # (the draft of these cases has heads of 64)
            target_heads.append(a[13])
        return counted(*a)
    monkeypatch.setattr(ops.hip.lib(), "tf_rope_append", rope_append)
    for name in ZOO:
        g = _weights(name)[0]
        ge = _product(name, graphs=False)
        prompt = Hh.prompt_of(g)
        n0 = calls["tf_qk_norm_rope_append"]
        run = _run_triforce(ge, g, prompt, 24)
        # (tf_rope_append itself stays in use: the 68M draft's un-fused layers take it)
        assert calls["tf_qk_norm_rope_append"] > n0 and calls["tf_rope_append_gqa"] == 0 and not target_heads
        _check_stream("TRIFORCE_FUSE=none", name, prompt, list(run.emitted))


def test_fp8_kv_cache_stays_lossless_against_its_own_target(monkeypatch):
    """TRIFORCE_KV_CACHE=fp8 (multi-head): the cache is not lossless against the fp16 model, so greedy TriForce is checked
    against the FP8-KV target's own Autoregressive steps, as tests/test_gpu_fp8_kv.py does."""
    from tests.test_gpu_fp8_kv import _ar_gaps
    monkeypatch.setenv("TRIFORCE_KV_CACHE", "fp8")
    g = _weights("tiny-qknorm")[0]
    ge = _product("tiny-qknorm", graphs=True)
    assert ge.engine.kv_cache.fp8 and ge.engine.model.weights.qk_norm
    prompt = Hh.prompt_of(g)
    run = _run_triforce(ge, g, prompt, 32)
    stream = list(run.emitted)
    gaps = _ar_gaps(ge.engine.model, prompt.to(DEV), stream, g["prefill"] + len(stream) + 16)
    assert max(gaps) < GAP_TOL, f"token {gaps.index(max(gaps))} trails the FP8-KV target's argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x == 0.0) >= len(gaps) - 3


def _launches(calls):
    """The launch list of one decode forward, by entry point, with the attention entries folded into one name."""
    out = collections.Counter()
    for k, v in calls.items():
        if k.endswith(("_ws_floats", "_pick_nsplit", "_tune")) or k in ("tf_abi_version", "tf_sg_workspace"):
            continue
        out["attn_decode" if k.startswith("tf_attn_decode") else k] += v
    return dict(out)


def test_a_norm_free_model_keeps_its_launch_list_and_a_qk_norm_model_adds_one_per_layer(monkeypatch):
    """Two engines of different commits cannot be compared bit for bit, so the statement is about launches: a decode forward
    of the norm-free ``tiny`` issues what it issued before — per layer one fused q|k|v launch, attention, o GEMM, gate|up,
    down GEMM, and no tf_qk_norm_rope_append — and its prefill chunk takes tf_rope_append; the QK-norm model's decode forward
    replaces the fused q|k|v launch by a plain GEMM + tf_qk_norm_rope_append (6 per layer)."""
    from triforce_amd.models import zoo
    from triforce_amd.models.cache import FlashSimpleCache
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    ops = _ops()
    models = {n: LlamaForCausalLM(zoo.config(n), DEV).init_random(3) for n in ("tiny", "tiny-qknorm")}
    ids = torch.randint(3, 32000, (1, 128 + 7), generator=torch.Generator().manual_seed(5)).to(DEV)
    calls = _count_calls(ops, monkeypatch)
    seen = {}
    for n, m in models.items():
        cache = FlashSimpleCache(m, 256)
        calls.clear()
        m(input_ids=ids[:, :128], kv_cache=cache)
        pre = dict(calls)
        calls.clear()
        m(input_ids=ids[:, 128:], kv_cache=cache)
        seen[n] = (pre, _launches(calls))
    torch.cuda.synchronize()
    Lyr = 2
    pre, dec = seen["tiny"]
    assert pre.get("tf_qk_norm_rope_append", 0) == 0 and pre["tf_rope_append"] == Lyr
    assert dec == {"tf_embed_rows": 1, "tf_skinny_qkv_rope_act": Lyr, "attn_decode": Lyr, "tf_skinny_gemm_act": 2 * Lyr + 1,
                   "tf_skinny_gemm_swiglu_act": Lyr}, dec
    pre, dec = seen["tiny-qknorm"]
    assert pre["tf_qk_norm_rope_append"] == Lyr and pre.get("tf_rope_append", 0) == 0
    assert dec == {"tf_embed_rows": 1, "tf_qk_norm_rope_append": Lyr, "attn_decode": Lyr, "tf_skinny_gemm_act": 3 * Lyr + 1,
                   "tf_skinny_gemm_swiglu_act": Lyr}, dec
