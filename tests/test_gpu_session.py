"""TriForceRunner.extend / TriForceSession on a real MI355X: a prefilled document kept across follow-up
questions and chat turns, through the real kernels and the captured graphs.

Greedy answers are judged the way tests/test_gpu_e2e.py judges them: teacher-forced against plain autoregressive forwards of
the same target — here over a FRESH cache that a plain prefill of (document + question) filled, so the rows extend() fed are
checked too — every emitted token the argmax up to GAP_TOL where two logits are within fp16 noise."""
import copy

import pytest
import torch

from tests import helpers as Hh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GAP_TOL = 8e-3        # as tests/test_gpu_e2e.py: an emitted token may trail the target's argmax by ~2 fp16 spacings
GREEDY = dict(top_k=-1, top_p=1e-9, temperature=1.0)
PATHS = ["on_device", "verify_probs_ids", "eager"]


def _golden(fp8=False, **over):
    g = copy.deepcopy(Hh.load_golden("small_gamma6"))
    g.update(dict(dict(gen_len=260, budget=320), **over))
    if fp8:                                                # head_dim 128, the FP8 cache's only head size: 256 = 2 x 128
        g["tcfg"]["num_attention_heads"] = g["tcfg"]["num_key_value_heads"] = 2
    return g


def _question(g, n, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(3, g["tcfg"]["vocab_size"], (1, n), generator=gen).to(DEV)


def _set_path(monkeypatch, path, fp8=False):
    """The three forms of the outer step: inner graphs + the device-set verify; the captured verify without inner graphs;
    eager target verify and four-launch inner iterations."""
    from triforce_amd.utils import decoding as Dm
    monkeypatch.setattr(Dm, "INNER_GRAPH", path == "on_device")
    monkeypatch.setenv("TRIFORCE_INNER_GRAPH", "1" if path == "on_device" else "0")
    monkeypatch.setenv("TRIFORCE_TARGET_GRAPH", "0" if path == "eager" else "1")
    if fp8:
        monkeypatch.setenv("TRIFORCE_KV_CACHE", "fp8")
    else:
        monkeypatch.delenv("TRIFORCE_KV_CACHE", raising=False)


def _check_path(run, path):
    ge = run.ge
    if path == "on_device":
        assert run.inner is not None and run._device_sets() is not None
    elif path == "verify_probs_ids":
        assert run.inner is None and sorted(ge.target_graphs) == [1, run.gamma + 1, run.gamma + 2]
    else:
        assert run.inner is None and not ge.target_graphs


def _steps(run, n):
    while run.n < n:
        run.step()
    return list(run.emitted)


def _ar_gaps(model, prompt, stream, budget, fp8):
    """Teacher-forced argmax gaps of the target itself: a fresh cache, the prompt as one plain prefill, then one
    autoregressive step per emitted token."""
    from triforce_amd.models.cache import FlashSimpleCache
    cache = FlashSimpleCache(model, budget, kv_dtype="fp8" if fp8 else "fp16")
    logits = model(input_ids=prompt, kv_cache=cache).logits[0, -1]
    gaps = [float(logits.max() - logits[stream[0]])]
    for i in range(len(stream) - 1):
        logits = model(input_ids=torch.tensor([[stream[i]]], device=DEV), kv_cache=cache).logits[0, -1]
        gaps.append(float(logits.max() - logits[stream[i + 1]]))
    return gaps


def _lossless(what, run, prompt, stream, g, fp8):
    gaps = _ar_gaps(run.eng.model, prompt, stream, g["prefill"] + g["gen_len"] + 16, fp8)
    Hh.note(f"session {what}: {len(gaps)} tokens, max teacher-forced gap {max(gaps):.5f}, "
            f"{sum(1 for x in gaps if x > 0.0)} not the argmax")
    assert max(gaps) < GAP_TOL, f"{what}: token {gaps.index(max(gaps))} trails the target's argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x == 0.0) >= len(gaps) - 3


@pytest.mark.parametrize("fp8", [False, True], ids=["fp16kv", "fp8kv"])
@pytest.mark.parametrize("path", PATHS)
def test_follow_up_question_and_chat_turn_are_lossless_small(path, fp8, monkeypatch):
    """prefill(doc), steps, extend(q, keep=P), steps, extend(turn), steps on small_gamma6-size models: both answers are the
    greedy continuation of the target over (document + question) and over the whole history, on each of the three step
    forms, with the fp16 and the FP8 full cache."""
    from triforce_amd.utils.decoding import TriForceRunner
    _set_path(monkeypatch, path, fp8)
    g = _golden(fp8)
    P = g["prefill"]
    ge = Hh.build_product(g, DEV, graphs=True)
    assert ge.engine.kv_cache.fp8 == fp8
    doc = Hh.prompt_of(g).to(DEV)
    run = TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], **GREEDY)
    _check_path(run, path)
    run.prefill(doc)
    first = _steps(run, 12)
    q = _question(g, 40, 11)                               # 39 rows through the verify route, the last row alone
    run.extend(q, keep=P)
    assert run.n == 0 and len(run.emitted) == 1 and ge.engine.kv_cache.seq_len == P + 40
    answer = _steps(run, 30)
    assert ge.engine.kv_cache.seq_len == P + 40 + len(answer) - 1
    _lossless(f"{path} fp8={fp8} ask", run, torch.cat([doc, q], dim=1), answer, g, fp8)
    turn = _question(g, 5, 12)
    run.extend(turn)                                       # chat turn: [pending] + 5 ids, 5 rows + the last row
    history = torch.cat([doc, q, torch.tensor([answer], device=DEV), turn], dim=1)
    assert torch.equal(run.history, history)
    reply = _steps(run, 20)
    _lossless(f"{path} fp8={fp8} turn", run, history, reply, g, fp8)
    assert len(first) >= 13 and (run.accepted_count > 0 or run.resample_count > 0)


@pytest.mark.parametrize("q_len", [2, 8, 70])
def test_every_feeding_route_is_lossless_small(q_len, monkeypatch):
    """The other piece sizes on the default path: the autoregressive step (one body row), the captured verify length
    (gamma + 2 = 8 rows -> 7 body rows), and prefill chunks (69 body rows)."""
    from triforce_amd.utils.decoding import TriForceRunner
    _set_path(monkeypatch, "on_device")
    g = _golden()
    ge = Hh.build_product(g, DEV, graphs=True)
    doc = Hh.prompt_of(g).to(DEV)
    run = TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], **GREEDY)
    run.prefill(doc)
    _steps(run, 9)
    q = _question(g, q_len, 13)
    run.extend(q, keep=g["prefill"])
    _lossless(f"route q_len={q_len}", run, torch.cat([doc, q], dim=1), _steps(run, 30), g, False)


@pytest.mark.parametrize("fp8", [False, True], ids=["fp16kv", "fp8kv"])
def test_document_rows_are_byte_identical_across_extend(fp8, monkeypatch):
    """Rows [0, P) of the full cache — fp16 K / V, or FP8 codes and exponent bytes — do not change a bit across a follow-up
    question (verify route and prefill chunks) nor across a chat turn."""
    from triforce_amd.utils.decoding import TriForceRunner
    _set_path(monkeypatch, "on_device", fp8)
    g = _golden(fp8)
    P = g["prefill"]
    ge = Hh.build_product(g, DEV, graphs=True)
    kv = ge.engine.kv_cache
    run = TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], **GREEDY)
    run.prefill(Hh.prompt_of(g).to(DEV))
    planes = (kv.kc, kv.vc, kv.ke, kv.ve) if fp8 else (kv.k, kv.v)
    before = [t[:, :, :P].view(torch.uint8).clone() if t.dtype == torch.float8_e4m3fn else t[:, :, :P].clone() for t in planes]

    def same():
        torch.cuda.synchronize()
        for t, b in zip(planes, before):
            now = t[:, :, :P].view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t[:, :, :P]
            assert torch.equal(now, b)
    _steps(run, 9)
    same()
    for q_len in (33, 70):
        run.extend(_question(g, q_len, 20 + q_len), keep=P)
        same()
        _steps(run, 9)
        same()
    run.extend(_question(g, 4, 29))
    _steps(run, 9)
    same()


@pytest.mark.parametrize("path", PATHS[:2])
def test_nothing_is_recaptured_across_extend(path, monkeypatch):
    """No hipGraph is captured during extend() or the steps after it, the graph objects are the ones captured when the engine
    and the runner were built, and the next step sets the verify graphs' device scalars again (dev_len)."""
    from triforce_amd.utils import graph_infer as gi
    from triforce_amd.utils.decoding import TriForceRunner
    _set_path(monkeypatch, path)
    g = _golden(prefill=1088)                              # 17 full 64-token chunks: the draft-prefill graph exists after prefill()
    ge = Hh.build_product(g, DEV, graphs=True)
    run = TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], **GREEDY)
    _check_path(run, path)
    run.prefill(Hh.prompt_of(g).to(DEV))
    _steps(run, 9)

    def graphs():
        out = [fn.graph for fn in ge.callables.values()] + [ge.callable_model_verify.graph]
        out += [tg.graph for tg in ge.target_graphs.values()]
        out += list(run.inner.graphs) if run.inner is not None else []
        out.append(ge.engine._dpf_graph[1][0])
        return out
    before, inner, bufs = graphs(), run.inner, run.bufs
    captures = []
    real = gi._capture
    monkeypatch.setattr(gi, "_capture", lambda *a, **k: (captures.append(1), real(*a, **k))[1])
    for keep in (g["prefill"], None):
        run.extend(_question(g, 21, 30), keep=keep)
        assert ge.dev_len is None and not ge.verify_lengths_current(g["gamma"])
        run.step()
        if path == "on_device":
            assert ge.dev_len == ge.engine.kv_cache.seq_len and ge.verify_lengths_current(g["gamma"])
        _steps(run, 12)
    after = graphs()
    assert captures == [] and len(after) == len(before) and all(a is b for a, b in zip(after, before))
    assert run.inner is inner and run.bufs is bufs and ge._tf_spec_buffers is bufs


def test_stochastic_sessions_repeat_and_match_the_four_launch_form(monkeypatch):
    """T = 0.8 / top-p 0.95 with a fixed uniform stream: two identical sessions emit identical streams across ask() and
    turn(), and the session under the inner graphs — uniforms read behind the device cursor, which the kernels advance —
    emits the stream, accept counts and stream position of the four-launch form, which reads them through host pointers."""
    from triforce_amd.utils.decoding import TriForceSession
    from triforce_amd.utils.sampling import UniformSource
    g = _golden()
    doc = Hh.prompt_of(g).to(DEV)
    q, t = _question(g, 40, 41), _question(g, 6, 42)
    vals = Hh.fixed_uniforms(n=4096, seed=77)
    out = []
    for path in ("on_device", "on_device", "verify_probs_ids"):
        _set_path(monkeypatch, path)
        ge = Hh.build_product(g, DEV, temperature=0.8, top_p=0.95, graphs=True)
        rng = UniformSource(DEV, values=vals)
        s = TriForceSession(Hh.FakeTokenizer(), ge, g["gamma"], top_k=-1, top_p=0.95, temperature=0.8, rng=rng)
        assert (s.run.inner is not None) == (path == "on_device")
        s.prefill(doc)
        rec = [s.generate(30)]
        rec.append(s.ask(q, 40))
        rec.append(s.turn(t, 40))
        rec.append(s.ask(t, 30))
        out.append(([r["tokens"] for r in rec], [r["counts"] for r in rec], rng.pos))
        assert all(r["ttft"] > 0 for r in rec)
    assert out[0] == out[1], "two identical sessions diverge"
    for i in range(4):
        a, b = out[0][0][i], out[2][0][i]
        assert a == b, f"answer {i}: inner graphs diverge from the four-launch form at {Hh.common_prefix(a, b)} of {len(b)}"
    assert out[0][1] == out[2][1] and out[0][2] == out[2][2]
    # (a step emits at most gamma + 2 tokens: the four answers took at least this many outer steps and records)
    assert sum(len(c) for c in out[0][1]) >= (30 + 40 + 40 + 30) // (g["gamma"] + 2)
    Hh.note(f"stochastic session: {sum(len(x) for x in out[0][0])} tokens over 4 answers identical twice and to the four-launch form")


def test_retrieval_fp8_weights_follow_up_is_lossless_small(monkeypatch):
    """TRIFORCE_RETRIEVAL_WEIGHTS=fp8 changes the drafting tier only: a follow-up answer is still the target's."""
    from triforce_amd.utils.decoding import TriForceRunner
    _set_path(monkeypatch, "on_device")
    monkeypatch.setenv("TRIFORCE_RETRIEVAL_WEIGHTS", "fp8")
    g = _golden()
    ge = Hh.build_product(g, DEV, graphs=True)
    assert ge.engine.model.weights.fp8_active()
    doc = Hh.prompt_of(g).to(DEV)
    run = TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], **GREEDY)
    run.prefill(doc)
    _steps(run, 9)
    q = _question(g, 40, 51)
    run.extend(q, keep=g["prefill"])
    _lossless("retrieval fp8 weights ask", run, torch.cat([doc, q], dim=1), _steps(run, 30), g, False)


def test_full_scale_7b_follow_up_question_is_lossless():
    """configs[1] shape: 7B, 124 928-token document through a REAL chunked prefill, budget 4096, gamma 6, hipGraphs, aligned
    weights.  After ask(q, keep=P) with a 64-token question, at least 64 emitted tokens are each the teacher-forced argmax
    (up to GAP_TOL) of the target's own autoregressive steps over the same cache rolled back to document + question; rows
    [0, P) of layer 0 and of the last layer are byte-identical across the call."""
    import argparse
    import bench
    from triforce_amd.utils.decoding import TriForceSession
    from triforce_amd.utils.sampling import UniformSource
    args = argparse.Namespace(target="llama-7B-128K", prefill=124928, budget=4096, chunk_size=8, gamma=6, temp=1.0,
                              top_p=1e-9, gen_cap=256, seed=0, no_graphs=False)
    dev = torch.device(DEV)
    target, draft = bench.load_models(args, dev, "aligned", "aligned:0.7:0.9", "aligned:0.7:0.9")
    ge = bench.build_engine(args, dev, target, draft)
    assert sorted(ge.target_graphs) == [1, 7, 8]
    kv = ge.engine.kv_cache
    tcfg, _ = bench.target_config(args.target)
    gen = torch.Generator().manual_seed(0)
    ids = torch.randint(3, tcfg.vocab_size, (1, args.prefill), generator=gen).to(dev)
    q = torch.randint(3, tcfg.vocab_size, (1, 64), generator=gen).to(dev)
    s = TriForceSession(bench._Tok(), ge, args.gamma, top_k=-1, top_p=args.top_p, temperature=args.temp,
                        rng=UniformSource(dev, seed=0))
    s.prefill(ids)
    P = kv.seq_len
    assert P == args.prefill == s.document
    first = s.generate(16)
    last = kv.layers - 1
    before = [kv.k[0, :, :P].clone(), kv.v[0, :, :P].clone(), kv.k[last, :, :P].clone(), kv.v[last, :, :P].clone()]
    st = s.ask(q, 64, keep=P)
    stream = list(st["tokens"])
    assert len(stream) >= 65 and kv.seq_len == P + 64 + st["n"]
    for b, now in zip(before, (kv.k[0, :, :P], kv.v[0, :, :P], kv.k[last, :, :P], kv.v[last, :, :P])):
        assert torch.equal(b, now)
    kv.seq_len = P + 64                                    # AR steps over document + question
    gaps = []
    for i in range(len(stream) - 1):
        tok = torch.tensor([[stream[i]]], device=dev)
        logits = ge.engine.model(input_ids=tok, kv_cache=kv, graph_cache=None).logits[0, -1]
        gaps.append(float(logits.max() - logits[stream[i + 1]]))
    Hh.note(f"session full 7B: ask ttft {st['ttft']:.3f} s vs prefill {first['ttft']:.2f} s, {len(gaps)} tokens, max gap "
            f"{max(gaps):.5f}, acceptance {st['acceptance_rate']:.3f}")
    assert len(gaps) >= 64
    assert max(gaps) < GAP_TOL, f"token {gaps.index(max(gaps)) + 1} trails the autoregressive argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x == 0.0) >= len(gaps) - 2
    del ge, s, kv, target, draft, before
    torch.cuda.empty_cache()
