"""Prompt-lookup n-gram draft tier on the device: tf_ngram_draft / tf_ngram_commit torch.equal to the host
restatement tests/test_ngram_draft_cpu.py checks against a brute force, and the decode loop over NgramDraft end to end at
prefill 2 048 on three target forms."""
import pytest
import torch

from tests import helpers as Hh
from tests.test_ngram_draft_cpu import GREEDY, NAMED, check_invariant, commit_cases, random_cases, repetitive_prompt, run_rule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def same_as_host(hist, L, blk, N, V, q=None, ws=None):
    """One launch over device copies (q as given: its old contents must not matter) against ops.ngram_draft_host."""
    from triforce_amd import ops
    L_t = torch.tensor([L], dtype=torch.int32)
    want_q, want_info = ops.ngram_draft_host(hist, L_t, blk, N, V)
    q, info = ops.ngram_draft(hist.to(DEV), L_t.to(DEV), blk.to(DEV), N, V, q=q, ws=ws)
    assert info.cpu().tolist() == want_info.tolist(), (L, N, V, info.cpu().tolist(), want_info.tolist())
    assert torch.equal(q.cpu(), want_q)
    return want_info.tolist()


@pytest.mark.parametrize("case", NAMED, ids=[c[0] for c in NAMED])
def test_named_cases(case):
    _, hist, blk, N, V, want = case
    q, info = run_rule(hist, blk, N, V, device=DEV, q_fill=float("nan"))
    assert tuple(info) == want
    one_hot = torch.zeros(V)
    one_hot[want[0]] = 1.0
    assert torch.equal(q.cpu(), one_hot)


def test_random_contexts_on_small_alphabets():
    for hist, blk, N, V in random_cases(150, 6):
        h = torch.tensor(hist + [0], dtype=torch.int64).to(torch.int32)        # (cap = L + 1)
        same_as_host(h, len(hist), torch.tensor(blk, dtype=torch.int64), N, V)


def _edges():
    """Where the implementation's slices begin and end: a thread's group of four, a workgroup's 1 024 candidates of one pass,
    and the whole grid's stride (4 x threads)."""
    from triforce_amd import ops
    stride = 4 * ops.ngram_draft_threads()
    return sorted({b + o for b in (0, 4, 8, 1024, 2048, stride, stride + 1024) for o in (-1, 0, 1, 3, 4)} - {-1})


def test_history_length_at_every_slice_edge_and_at_capacity():
    """L at each edge and one either side over a four-symbol history (the last candidates j = L - 1 .. and the block's sit on
    the edge), at a capacity that is no multiple of four, and L == cap."""
    gen = torch.Generator().manual_seed(8)
    edges = _edges()
    cap = edges[-1] + 6
    assert cap % 4 != 0
    hist = torch.randint(0, 4, (cap,), generator=gen).to(torch.int32)
    for L in [e for e in edges if e >= 0] + [cap - 1, cap]:
        blk = torch.randint(0, 4, (1 + L % 5,), generator=gen)
        same_as_host(hist, L, blk, 1 + L % 8, 4)


def test_a_planted_match_at_every_slice_edge():
    """One three-token match, unique in a history of other ids, ending at j = each thread's / workgroup's / pass's first and
    last candidate: the proposal is the token behind it."""
    from triforce_amd import ops
    gen = torch.Generator().manual_seed(9)
    edges = [e for e in _edges() if e >= 2]
    cap = edges[-1] + 9
    V = 5000
    base = torch.randint(0, 1000, (cap,), generator=gen).to(torch.int32)
    blk = torch.tensor([4001, 4002, 4003], dtype=torch.int64)
    ws = ops.ngram_workspace(DEV)                      # one workspace for every launch: each leaves it zero
    for j in edges:
        hist = base.clone()
        hist[j - 2:j + 1] = blk.to(torch.int32)
        hist[j + 1] = 4500 + j % 400
        info = same_as_host(hist, cap, blk, 3, V, ws=ws)
        assert info == [4500 + j % 400, 3, j, cap + 3]
    assert ws.cpu().tolist() == [0, 0]


@pytest.mark.parametrize("V", [7, 32000, 151936])
def test_row_is_rewritten_whatever_it_held(V):
    """NaN-filled rows at three vocabularies (7: no 16-byte body; a row of a (3, V) block whose start is not 16-byte aligned
    when V is odd), the proposal at ids 0, V - 1 and in between."""
    for d in (0, V - 1, V // 2):
        hist = torch.tensor([1, d, 2, 2], dtype=torch.int64).to(torch.int32)       # ... 1 d ... 1 -> d
        blk = torch.tensor([1], dtype=torch.int64)
        block = torch.full((3, V), float("nan"), dtype=torch.float32, device=DEV)
        for r in range(3):
            info = same_as_host(hist, 4, blk, 3, V, q=block[r])
            assert info[0] == d
        assert float(block.sum()) == 3.0


@torch.inference_mode()
def test_one_captured_graph_replayed_over_changed_inputs():
    """The same hipGraph three times back to back over changed blk, hist and len_dev: the key and the ticket must have reset.
    (Under inference mode, like the engines' captures: such a capture works whatever captures came before it.)"""
    from triforce_amd import ops
    V, cap = 32000, 9000
    gen = torch.Generator().manual_seed(10)
    hist = torch.zeros(cap, dtype=torch.int32, device=DEV)
    L = torch.zeros(1, dtype=torch.int32, device=DEV)
    blk = torch.zeros(4, dtype=torch.int64, device=DEV)
    q = torch.full((V,), float("nan"), dtype=torch.float32, device=DEV)
    info = torch.zeros(4, dtype=torch.int32, device=DEV)
    ws = ops.ngram_workspace(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ngram_draft(hist, L, blk, 3, V, q=q, info=info, ws=ws)
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.ngram_draft(hist, L, blk, 3, V, q=q, info=info, ws=ws)
    seen = set()
    for length, alphabet in ((8000, 6), (37, 3), (9000, 20000)):       # a long match, a short history, (almost surely) no match
        h = torch.randint(0, alphabet, (cap,), generator=gen).to(torch.int32)
        b = torch.randint(0, alphabet, (4,), generator=gen)
        hist.copy_(h)
        L.fill_(length)
        blk.copy_(b)
        graph.replay()
        want_q, want_info = ops.ngram_draft_host(h, torch.tensor([length], dtype=torch.int32), b, 3, V)
        assert info.cpu().tolist() == want_info.tolist() and torch.equal(q.cpu(), want_q)
        seen.add(int(want_info[1]))
    assert 3 in seen and 0 in seen
    assert ws.cpu().tolist() == [0, 0]


def test_entry_points_refuse_bad_arguments():
    from triforce_amd import hip, ops
    hist = torch.zeros(16, dtype=torch.int32, device=DEV)
    L = torch.zeros(1, dtype=torch.int32, device=DEV)
    blk = torch.zeros(40, dtype=torch.int64, device=DEV)
    q = torch.zeros(64, dtype=torch.float32, device=DEV)
    info = torch.zeros(4, dtype=torch.int32, device=DEV)
    ws = ops.ngram_workspace(DEV)
    p, lib = ops._ptr, hip.lib()

    def draft(h=hist, cap=16, m=1, N=3, V=64, qq=q, w=ws):
        return lib.tf_ngram_draft(p(h) if h is not None else None, cap, p(L), p(blk), m, N, V, p(qq), p(info), p(w), None)
    assert draft(h=None) == -22 and draft(cap=0) == -22 and draft(m=0) == -22 and draft(m=33) == -22
    assert draft(N=0) == -22 and draft(N=9) == -22 and draft(V=0) == -22 and draft(h=hist[1:]) == -22
    assert lib.tf_ngram_commit(None, 16, p(L), p(blk), 0, None) == -22
    assert lib.tf_ngram_commit(p(hist), 16, p(L), p(blk), 65, None) == -22
    assert lib.tf_ngram_commit(p(hist), 16, p(L), p(blk), 0, None) == 0
    torch.cuda.synchronize()
    assert int(L) == 0 and ws.cpu().tolist() == [0, 0]


def test_commit():
    commit_cases(DEV)


# ---- end to end --------------------------------------------------------------------------------------------------------
PREFILL, GAMMA, GEN = 2048, 6, 48
TARGETS = ["tiny", "tiny-gqa", "tiny-v128k"]


@pytest.fixture(scope="module")
def engines():
    """The module's engines, one per (target, graphs / eager, sampling settings), released when the module is done: hipGraphs
    that were created under inference mode and stay alive keep torch's capture state in a form that makes every later capture
    OUTSIDE inference mode (other test modules') fail."""
    import gc
    cache = {}
    yield cache
    cache.clear()
    gc.collect()


def _engine(_engines, name, mode, temperature, top_p):
    from triforce_amd.models import zoo
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    from triforce_amd.models.ngram_draft import NgramCache, NgramDraft
    from triforce_amd.utils.graph_infer import GraphInferenceEngine
    key = (name, mode, temperature, top_p)
    if key not in _engines:
        target = LlamaForCausalLM.from_pretrained("random:1", config=zoo.config(name), device_map=DEV)
        V = target.config.vocab_size
        full = FlashSimpleCache(target, PREFILL + 400)
        ge = GraphInferenceEngine(target, full, RetrievalCache(target, max_budget=512, prefill=PREFILL, gamma=GAMMA, chunk_size=8),
                                  NgramDraft(V, DEV, ngram_max=3), NgramCache(full.max_budget, DEV, gamma=GAMMA))
        if mode == "graphs":
            ge.initialize_cuda_graph(GAMMA, probs=True, temperature=temperature, top_p=top_p, verbose=False)
        else:
            ge.initialize_eager(GAMMA, probs=True, temperature=temperature, top_p=top_p)
        _engines[key] = ge
    return _engines[key]


def _prompt(ge, seed=1):
    return repetitive_prompt(ge.engine.model.config.vocab_size, PREFILL, seed).to(DEV)


@pytest.mark.parametrize("mode", ["graphs", "eager"])
@pytest.mark.parametrize("name", TARGETS)
def test_greedy_stream_is_the_autoregressive_stream(engines, name, mode):
    from triforce_amd.utils.decoding import Autoregressive, TriForceRunner
    ge = _engine(engines, name, mode, GREEDY["temperature"], GREEDY["top_p"])
    prompt = _prompt(ge)
    run = TriForceRunner(Hh.FakeTokenizer(), ge, GAMMA, **GREEDY)
    assert run.ngram is ge.engine.draft_cache and (mode == "graphs" or run.inner is None)
    run.prefill(prompt)
    check_invariant(run)
    while run.n < GEN:
        run.step()
    check_invariant(run)
    got = list(run.emitted)
    _, ar = Autoregressive(Hh.FakeTokenizer(), ge, prompt, max_len=len(got) - 1, return_tokens=True, **GREEDY)
    print(f"{name} / {mode}: {run.n} tokens in {len(run.counts)} steps, {run.accepted_count} of {run.draft_count} drafted "
          f"tokens accepted by the target, common prefix with the autoregressive stream {Hh.common_prefix(got, ar)}")
    assert got == ar


@pytest.mark.parametrize("name", TARGETS)
def test_stochastic_stream_is_the_same_on_every_inner_path(engines, name, monkeypatch):
    """T 0.6 / top-p 0.9 over one fixed uniform stream: the four-launch inner iteration (TRIFORCE_INNER_GRAPH=0), the inner
    graphs without lookahead, and lookahead depth 3 emit identical tokens with identical accept counts."""
    from triforce_amd.utils import decoding as Dm
    from triforce_amd.utils import graph_infer as Gi
    from triforce_amd.utils.decoding import TriForce
    from triforce_amd.utils.sampling import UniformSource
    monkeypatch.setattr(Gi._InnerGraphs, "_measure_break_even", lambda self, rng: 0.0)     # (keeps every form on throughout)
    monkeypatch.setattr(Gi._InnerGraphs, "_measure_break_even3", lambda self, rng: 0.0)
    ge = _engine(engines, name, "graphs", 0.6, 0.9)
    prompt, vals = _prompt(ge, seed=2), Hh.fixed_uniforms(n=4096, seed=77)
    out = {}
    for setting, inner, look, depth in (("four launches", False, "0", "2"), ("inner graphs", True, "0", "2"),
                                        ("lookahead depth 3", True, "1", "3")):
        monkeypatch.setattr(Dm, "INNER_GRAPH", inner)
        monkeypatch.setenv("TRIFORCE_INNER_GRAPH", "1" if inner else "0")
        monkeypatch.setenv("TRIFORCE_INNER_LOOKAHEAD", look)
        monkeypatch.setenv("TRIFORCE_INNER_LOOKAHEAD_DEPTH", depth)
        st = TriForce(Hh.FakeTokenizer(), ge, prompt, gamma=GAMMA, max_len=GEN, top_k=-1, top_p=0.9, temperature=0.6,
                      rng=UniformSource(DEV, values=vals), return_details=True)
        out[setting] = st
        dc = ge.engine.draft_cache
        assert dc.length == ge.engine.kv_cache.seq_len == int(dc.len_dev)
    ref = out["four launches"]
    for setting in ("inner graphs", "lookahead depth 3"):
        st = out[setting]
        assert st["tokens"] == ref["tokens"], f"{setting}: tokens diverge at {Hh.common_prefix(st['tokens'], ref['tokens'])}"
        assert st["counts"] == ref["counts"] and st["drafted"] == ref["drafted"]
        assert st["acc_rate_middle"] == ref["acc_rate_middle"]
    look = out["lookahead depth 3"]
    print(f"{name}: {ref['n']} tokens, middle acceptance {ref['acc_rate_middle']:.3f}, target acceptance "
          f"{ref['acceptance_rate']:.3f}; lookahead replays {look['lookahead_replays']} (depth 3: "
          f"{look['lookahead_depth3_replays']}), hits {look['lookahead_hits']}, third {look['lookahead_third']}")
    assert ref["verify_replays"] == 0 and out["inner graphs"]["lookahead_replays"] == 0
    assert look["lookahead_replays"] > 0 and look["lookahead_depth3_replays"] > 0


@pytest.mark.parametrize("name", TARGETS)
def test_session_follow_up(engines, name):
    """One TriForceSession.ask on the prefilled document: the history is set again (the invariant holds), and the greedy answer
    is the target's own continuation — the same extend() again, then one autoregressive step per token."""
    from triforce_amd.utils.decoding import TriForceSession
    ge = _engine(engines, name, "graphs", GREEDY["temperature"], GREEDY["top_p"])
    prompt = _prompt(ge, seed=3)
    s = TriForceSession(Hh.FakeTokenizer(), ge, GAMMA, **GREEDY)
    s.prefill(prompt)
    s.generate(12)
    question = torch.randint(3, ge.engine.model.config.vocab_size, (1, 9), generator=torch.Generator().manual_seed(5)).to(DEV)
    st = s.ask(question, 24)
    run = s.run
    check_invariant(run)
    assert run.history[0].tolist() == prompt[0].tolist() + question[0].tolist() and st["n"] >= 24
    stream = list(st["tokens"])
    run.extend(question, keep=PREFILL)                 # the same state again
    check_invariant(run)
    assert run.next_token == stream[0]
    for i in range(len(stream) - 1):
        logits = ge.decode_step(torch.tensor([[stream[i]]], device=DEV))[0, -1]
        assert int(logits.argmax()) == stream[i + 1], f"token {i + 1} is not the target's greedy continuation"
