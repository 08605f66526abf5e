"""Re-anchoring the retrieval cache and the chunk-mean index on a real MI355X: the two index kernels
against the one-pass scorer, bit for bit, and generation / sessions past the retrieval budget through the real kernels and
the captured graphs.

Greedy streams are judged as tests/test_gpu_session.py judges them: teacher-forced against plain autoregressive forwards of
the same target over a FRESH cache that one plain prefill of the whole history filled."""
import copy

import pytest
import torch

from tests import helpers as Hh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GAP_TOL = 8e-3        # as tests/test_gpu_e2e.py: an emitted token may trail the target's argmax by ~2 fp16 spacings
GREEDY = dict(top_k=-1, top_p=1e-9, temperature=1.0)
N = 48                # reanchor_at: 6 verify blocks of gamma + 2 = 8 rows under the 64-row budget
# Seeds: small_gamma6's weights and prompt seed 203 at prefill 128 (tests/test_reanchor_cpu.py).  The plain loop's first 60 tokens
# meet the argmax condition for them on the device too: test_plain_loop_meets_the_argmax_condition_for_the_seed.


# =====================================================================================================================
# 1. kernels
# =====================================================================================================================
def _kq(C, chunk, D, H, seed=0):
    """K as a strided view (rows [5, 5 + C * chunk) of a longer cache) of N(0, 1) fp16 values, with rows of +-65 504: a chunk of
    +65 504 alone (an fp16 sum overflows at its second row, the fp32 sum does not), and chunks that mix both signs."""
    gen = torch.Generator().manual_seed(seed + 1000 * C + chunk + D + H)
    cache = torch.randn(H, 5 + C * chunk + 11, D, generator=gen).half().to(DEV)
    k = cache[:, 5:5 + C * chunk]
    big = torch.finfo(torch.float16).max
    k[:, :chunk] = big
    if C >= 3:
        k[:, chunk:2 * chunk:2] = big
        k[:, chunk + 1:2 * chunk:2] = -big
        k[:, 2 * chunk + 1, ::3] = -big
    q = torch.randn(H, D, generator=gen).half().to(DEV)
    assert not k.is_contiguous() and k.stride(0) > C * chunk * D
    return k, q


def _means(k, C, chunk):
    """tf_chunk_mean's contract in torch: fp32 sum in row order, times 1.0f / chunk, rounded to fp16."""
    H, _, D = k.shape
    rows = k[:, :C * chunk].reshape(H, C, chunk, D)
    acc = torch.zeros(H, C, D, dtype=torch.float32, device=k.device)
    for r in range(chunk):
        acc = acc + rows[:, :, r].float()
    return (acc * torch.tensor(1.0 / chunk, dtype=torch.float32, device=k.device)).half()


def _sentinel(H, cmax, D):
    return torch.full((H, cmax, D), -1, dtype=torch.int16, device=DEV).view(torch.float16)      # 0xFFFF in every element


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("H", [2, 32])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("chunk", [8, 16])
@pytest.mark.parametrize("C", [1, 3, 17, 1000])
def test_index_then_indexed_score_is_the_one_pass_scorer(C, chunk, D, H):
    from triforce_amd import ops
    k, q = _kq(C, chunk, D, H)
    want = ops.retrieval_score(k, q, C, chunk)
    index = _sentinel(H, C + 3, D)
    ops.chunk_mean(k, index, 0, C, chunk)
    got = ops.retrieval_score_indexed(index, q, C)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want))
    means = _means(k, C, chunk)
    assert torch.equal(_bits(index[:, :C]), _bits(means))
    assert bool((means[:, 0] == torch.finfo(torch.float16).max).all())          # the fp32 sum did not overflow
    assert bool((_bits(index[:, C:]) == -1).all())                              # chunks outside [0, C) untouched
    assert not bool(torch.isnan(want.float()).any())


@pytest.mark.parametrize("H", [2, 32])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("C", [17, 1000])
def test_index_built_in_pieces_and_untouched_chunks(C, D, H):
    from triforce_amd import ops
    chunk = 8
    k, q = _kq(C, chunk, D, H, seed=7)
    whole = _sentinel(H, C + 2, D)
    ops.chunk_mean(k, whole, 0, C, chunk)
    pieces = _sentinel(H, C + 2, D)
    for c0, c1 in ((6, C), (0, 5), (5, 6), (3, 3)):
        ops.chunk_mean(k, pieces, c0, c1, chunk)
    assert torch.equal(_bits(pieces), _bits(whole))
    part = _sentinel(H, C + 2, D)
    ops.chunk_mean(k, part, 2, C - 1, chunk)
    assert torch.equal(_bits(part[:, 2:C - 1]), _bits(whole[:, 2:C - 1]))
    assert bool((_bits(part[:, :2]) == -1).all()) and bool((_bits(part[:, C - 1:]) == -1).all())
    # fewer chunks scored than indexed: the head stride is the index's, not the chunk count
    assert torch.equal(_bits(ops.retrieval_score_indexed(whole, q, C - 4)), _bits(ops.retrieval_score(k, q, C - 4, chunk)))
    with pytest.raises(IndexError):
        ops.chunk_mean(k, whole, 0, C + 3, chunk)
    with pytest.raises(IndexError):
        ops.chunk_mean(k[:, :C * chunk - 1], whole, 0, C, chunk)
    with pytest.raises(IndexError):
        ops.retrieval_score_indexed(whole, q, C + 3)


# =====================================================================================================================
# 2. - 4. end to end
# =====================================================================================================================
def _golden(fp8=False, **over):
    g = copy.deepcopy(Hh.load_golden("small_gamma6"))
    g.update(dict(dict(prefill=128, budget=64, chunk=8, gen_len=300, pseed=203), **over))
    if fp8:                                                # head_dim 128, the FP8 cache's only head size: 256 = 2 x 128
        g["tcfg"]["num_attention_heads"] = g["tcfg"]["num_key_value_heads"] = 2
    return g


def _question(g, n, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(3, g["tcfg"]["vocab_size"], (1, n), generator=gen).to(DEV)


def _set_path(monkeypatch, path, fp8=False, index=False):
    """"on_device": inner graphs + the device-set captured verify (the default step form); "eager": TRIFORCE_TARGET_GRAPH=0,
    eager target verify and four-launch inner iterations."""
    from triforce_amd.utils import decoding as Dm
    monkeypatch.setattr(Dm, "INNER_GRAPH", path == "on_device")
    monkeypatch.setenv("TRIFORCE_INNER_GRAPH", "1" if path == "on_device" else "0")
    monkeypatch.setenv("TRIFORCE_TARGET_GRAPH", "0" if path == "eager" else "1")
    monkeypatch.setenv("TRIFORCE_RETRIEVAL_INDEX", "1" if index else "0")
    if fp8:
        monkeypatch.setenv("TRIFORCE_KV_CACHE", "fp8")
    else:
        monkeypatch.delenv("TRIFORCE_KV_CACHE", raising=False)


def _check_path(run, path):
    if path == "on_device":
        assert run.inner is not None and run._device_sets() is not None
    else:
        assert run.inner is None and not run.ge.target_graphs


def _steps(run, n):
    while run.n < n:
        run.step()
    return list(run.emitted)


def _lossless(what, model, prompt, stream, g, fp8):
    """Teacher-forced argmax gaps of the target itself: a fresh cache, the prompt as one plain prefill, then one
    autoregressive step per emitted token; within GAP_TOL of the best logit, exactly the best for all but <= 2."""
    from triforce_amd.models.cache import FlashSimpleCache
    cache = FlashSimpleCache(model, g["prefill"] + g["gen_len"] + 16, kv_dtype="fp8" if fp8 else "fp16")
    logits = model(input_ids=prompt, kv_cache=cache).logits[0, -1]
    gaps = [float(logits.max() - logits[stream[0]])]
    for i in range(len(stream) - 1):
        logits = model(input_ids=torch.tensor([[stream[i]]], device=DEV), kv_cache=cache).logits[0, -1]
        gaps.append(float(logits.max() - logits[stream[i + 1]]))
    Hh.note(f"reanchor {what}: {len(gaps)} tokens, max teacher-forced gap {max(gaps):.5f}, "
            f"{sum(1 for x in gaps if x > 0.0)} not the argmax")
    assert max(gaps) < GAP_TOL, f"{what}: token {gaps.index(max(gaps))} trails the target's argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x == 0.0) >= len(gaps) - 2


def _graphs(ge, run):
    out = [fn.graph for fn in ge.callables.values()] + [ge.callable_model_verify.graph]
    out += [tg.graph for tg in ge.target_graphs.values()]
    return out + (list(run.inner.graphs) if run.inner is not None else [])


@pytest.mark.parametrize("fp8", [False, True], ids=["fp16kv", "fp8kv"])
def test_plain_loop_meets_the_argmax_condition_for_the_seed(fp8, monkeypatch):
    """The condition the seed was picked by, on the device: without re-anchoring the first 60 tokens are within the cap."""
    from triforce_amd.utils.decoding import TriForceRunner
    _set_path(monkeypatch, "on_device", fp8)
    g = _golden(fp8)
    ge = Hh.build_product(g, DEV, graphs=True)
    doc = Hh.prompt_of(g).to(DEV)
    run = TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], **GREEDY)
    run.prefill(doc)
    _lossless(f"plain loop fp8={fp8}", ge.engine.model, doc, _steps(run, 56)[:61], g, fp8)


@pytest.mark.parametrize("fp8", [False, True], ids=["fp16kv", "fp8kv"])
@pytest.mark.parametrize("path", ["on_device", "eager"])
def test_generation_crosses_the_retrieval_budget(path, fp8, monkeypatch):
    """200 greedy tokens over a 64-row retrieval budget with reanchor_at=48, index off then on: both complete, keep the
    invariants between steps, emit the same stream with the same accept counts, the stream is the target's own continuation,
    and no hipGraph is captured once the runner exists — the graph objects after the run are those before it."""
    from triforce_amd.utils import graph_infer as gi
    from triforce_amd.utils.decoding import TriForceRunner
    out = []
    for index in (False, True):
        _set_path(monkeypatch, path, fp8, index)
        g = _golden(fp8)
        gamma = g["gamma"]
        ge = Hh.build_product(g, DEV, graphs=True)
        kv, rc = ge.engine.kv_cache, ge.engine.graph_cache
        assert kv.fp8 == fp8 and rc.use_index == index and rc.index is None
        doc = Hh.prompt_of(g).to(DEV)
        run = TriForceRunner(Hh.FakeTokenizer(), ge, gamma, reanchor_at=N, **GREEDY)
        _check_path(run, path)
        run.prefill(doc)
        before, inner, bufs = _graphs(ge, run), run.inner, run.bufs
        captures = []
        real = gi._capture
        monkeypatch.setattr(gi, "_capture", lambda *a, **k: (captures.append(1), real(*a, **k))[1])
        while run.n < 200:
            run.step()
            assert rc.prefill % 8 == 0 and kv.seq_len - rc.prefill + gamma + 2 <= 64
        monkeypatch.setattr(gi, "_capture", real)
        after = _graphs(ge, run)
        assert captures == [] and len(after) == len(before) and all(a is b for a, b in zip(after, before))
        assert run.inner is inner and run.bufs is bufs
        assert run.reanchors >= 3 and rc.prefill > rc.prefill0 == g["prefill"]
        assert (rc.indexed_chunks == [rc.chunks] * rc.layers) if index else rc.index is None
        out.append((list(run.emitted), list(run.counts)))
        if not index:
            _lossless(f"{path} fp8={fp8} 200 tokens", ge.engine.model, doc, run.emitted, g, fp8)
        del run, ge
    assert out[0] == out[1], f"index on / off diverge at token {Hh.common_prefix(out[0][0], out[1][0])}"


def test_sampled_run_across_two_reanchors_repeats(monkeypatch):
    """T = 0.8 / top-p 0.95 with a fixed uniform stream: two identical runs that cross the bound twice emit identical
    streams, accept counts and stream positions."""
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.sampling import UniformSource
    _set_path(monkeypatch, "on_device")
    g = _golden()
    doc = Hh.prompt_of(g).to(DEV)
    vals = Hh.fixed_uniforms(n=4096, seed=77)
    out = []
    for _ in range(2):
        ge = Hh.build_product(g, DEV, temperature=0.8, top_p=0.95, graphs=True)
        rng = UniformSource(DEV, values=vals)
        run = TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], top_k=-1, top_p=0.95, temperature=0.8, rng=rng,
                             reanchor_at=N)
        assert run.inner is not None
        run.prefill(doc)
        _steps(run, 130)
        assert run.reanchors >= 2
        out.append((list(run.emitted), list(run.counts), rng.pos, run.reanchors))
    assert out[0] == out[1]


@pytest.mark.parametrize("fp8", [False, True], ids=["fp16kv", "fp8kv"])
def test_sessions_cross_the_retrieval_budget(fp8, monkeypatch):
    """Three chat turns (20, 70, 20 rows) against a 64-row budget, each answer the target's continuation of the whole
    history; the plain runner refuses the second.  Then ask(keep=document) re-anchors down and equals — tokens and accept
    counts — the same question asked first."""
    from triforce_amd.utils.decoding import TriForceSession
    _set_path(monkeypatch, "on_device", fp8, index=True)
    g = _golden(fp8)
    doc, q = Hh.prompt_of(g).to(DEV), _question(g, 12, 32)
    turns = [_question(g, n, 21 + i) for i, n in enumerate((20, 70, 20))]
    ge = Hh.build_product(g, DEV, graphs=True)
    s = TriForceSession(Hh.FakeTokenizer(), ge, g["gamma"], reanchor_at=N, **GREEDY)
    kv, rc, model = ge.engine.kv_cache, ge.engine.graph_cache, ge.engine.model
    s.prefill(doc)
    history = torch.cat([doc, torch.tensor([s.generate(10)["tokens"]], device=DEV)], dim=1)
    for t in turns:
        st = s.turn(t, 14)
        history = torch.cat([history, t], dim=1)
        assert torch.equal(s.run.history, history)
        assert rc.prefill % 8 == 0 and kv.seq_len - rc.prefill + g["gamma"] + 2 <= 64
        _lossless(f"turn of {t.shape[1]} fp8={fp8}", model, history, st["tokens"], g, fp8)
        history = torch.cat([history, torch.tensor([st["tokens"]], device=DEV)], dim=1)
    assert rc.prefill > g["prefill"] + 64 and s.document == g["prefill"]
    grown = s.ask(q, 24)
    assert rc.prefill == g["prefill"] and rc.indexed_chunks == [16] * rc.layers
    _lossless(f"ask after growth fp8={fp8}", model, torch.cat([doc, q], dim=1), grown["tokens"], g, fp8)

    ge2 = Hh.build_product(g, DEV, graphs=True)
    s2 = TriForceSession(Hh.FakeTokenizer(), ge2, g["gamma"], reanchor_at=N, **GREEDY)
    s2.prefill(doc)
    s2.generate(10)
    first = s2.ask(q, 24)
    assert (grown["tokens"], grown["counts"]) == (first["tokens"], first["counts"])

    plain = TriForceSession(Hh.FakeTokenizer(), ge2, g["gamma"], **GREEDY)
    plain.prefill(doc)
    plain.generate(10)
    plain.turn(turns[0], 14)
    with pytest.raises(ValueError, match=r"retrieval budget max_budget=64: the covered region \[0, 128\) is fixed"):
        plain.turn(turns[1], 14)
