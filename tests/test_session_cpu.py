"""TriForceRunner.extend / TriForceSession on CPU, every HIP op swapped for its oracle restatement
(cpu_ops): a prefilled document is kept across follow-up questions and chat turns, and what comes out is still the
target's own greedy continuation.  Host logic only — the kernels are checked in tests/test_gpu_session.py."""
import pytest
import torch

from tests import helpers as Hh

GREEDY = dict(top_k=-1, top_p=1e-9, temperature=1.0)           # --greedy: the only greedy the reference's sampler admits
GAP_TOL = 8e-3        # as tests/test_gpu_e2e.py: an emitted token may trail the target's argmax by ~2 fp16 spacings


def _golden(**over):
    # room for several answers: full cache 1000 + 260 + 16 rows, retrieval tail up to 320 rows
    return dict(Hh.load_golden("small_gamma6"), **dict(dict(gen_len=260, budget=320), **over))


def _runner(g, ge=None):
    from triforce_amd.utils.decoding import TriForceRunner
    ge = ge or Hh.build_product(g, "cpu")
    return TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], **GREEDY)


def _question(g, n, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(3, g["tcfg"]["vocab_size"], (1, n), generator=gen)


def _steps(run, n):
    """Speculative steps until at least n tokens follow the first one; returns the emitted stream."""
    while run.n < n:
        run.step()
    return list(run.emitted)


def _follow(ar, stream):
    """Teacher-forced greedy check.  ``ar`` is a runner over the same target whose pending token is stream[0]; it is stepped
    autoregressively (one row per forward over its own full cache: no draft, no retrieval cache) over ``stream``, keeping
    the runner's books the way step() does, and every next token of the stream must be the argmax of that forward.
    Two logits of this fp16 model can tie exactly (the lm_head's output is fp16: spacing 2^-9 at the top logits' magnitude),
    and the 1-row forward and the verify's 7-row forward then break the tie differently, so "is the argmax" is stated as in
    tests/test_gpu_e2e.py: within GAP_TOL (~2 fp16 spacings) of the best logit, and exactly the best for all but <= 2
    tokens.  Following the stream keeps both runners in the same state past such a tie."""
    assert ar.next_token == stream[0]                  # the same extend() / prefill() on the same state: the same first token
    gaps = []
    for i in range(len(stream) - 1):
        logits = ar.ge.decode_step(torch.tensor([[stream[i]]]))[0, -1]
        ar._fed.append(stream[i])
        gaps.append(float(logits.max() - logits[stream[i + 1]]))
    ar.next_token, ar.emitted = stream[-1], list(stream)
    print(f"teacher-forced gaps: max {max(gaps):.5f}, {sum(1 for x in gaps if x > 0.0)} of {len(gaps)} not the argmax")
    assert max(gaps) < GAP_TOL, f"token {gaps.index(max(gaps)) + 1} trails the target's argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x == 0.0) >= len(gaps) - 2


@pytest.mark.parametrize("q_len", [1, 2, 8, 40, 70])
def test_follow_up_question_is_the_targets_greedy_continuation(cpu_ops, q_len):
    """prefill(doc), a few steps, extend(q, keep=P), steps — against the same target brought to the same state by the same
    extend() and then stepped autoregressively.  The question lengths take every feeding route: one row alone (1), the
    autoregressive step (2), the verify route (8, 40) and prefill chunks (70)."""
    g = _golden()
    doc, q = Hh.prompt_of(g), _question(g, q_len, 11)
    P = g["prefill"]
    spec = _runner(g)
    spec.prefill(doc)
    _steps(spec, 12)
    spec.extend(q, keep=P)
    assert spec.n == 0 and len(spec.emitted) == 1 and spec.counts == []
    got = _steps(spec, 30)
    ar = _runner(g)
    ar.prefill(doc)
    ar.extend(q, keep=P)
    _follow(ar, got)
    assert spec.eng.kv_cache.seq_len == P + q_len + len(got) - 1 == ar.eng.kv_cache.seq_len
    assert spec.accepted_count > 0 or spec.resample_count > 0        # the answer did come out of the speculative loop


@pytest.mark.parametrize("turn_len", [1, 9])
def test_two_chat_turns_are_the_targets_greedy_continuation(cpu_ops, turn_len):
    """keep=None: everything generated stays, the pending token is fed in front of the new ids."""
    g = _golden()
    doc = Hh.prompt_of(g)
    turns = [_question(g, turn_len, 21), _question(g, turn_len + 3, 22)]
    spec, ar = _runner(g), _runner(g)
    spec.prefill(doc)
    ar.prefill(doc)
    _follow(ar, _steps(spec, 10))
    for t in turns:
        before = spec.eng.kv_cache.seq_len
        spec.extend(t)
        ar.extend(t)
        assert spec.eng.kv_cache.seq_len == before + 1 + t.shape[1] == ar.eng.kv_cache.seq_len
        _follow(ar, _steps(spec, 14))
    assert torch.equal(spec.history[:, :g["prefill"]], doc)
    assert spec.history.shape[1] + len(spec._fed) == spec.eng.kv_cache.seq_len
    assert torch.equal(spec.history, ar.history) and spec._fed == ar._fed


def test_second_question_does_not_depend_on_the_first(cpu_ops):
    """ask(q1) then ask(q2), both with keep=P, against asking q2 first: tokens AND accept counts agree, so neither the full
    cache's rows [0, P), nor the retrieval selection, nor the draft's window carry anything over from the first answer."""
    from triforce_amd.utils.decoding import TriForceSession
    g = _golden()
    doc, q1, q2 = Hh.prompt_of(g), _question(g, 37, 31), _question(g, 12, 32)
    out = []
    for first in (True, False):
        s = TriForceSession(Hh.FakeTokenizer(), Hh.build_product(g, "cpu"), g["gamma"], **GREEDY)
        s.prefill(doc)
        st0 = s.generate(10)
        assert st0["n"] >= 10 and st0["ttft"] > 0
        if first:
            s.ask(q1, 20)
        st = s.ask(q2, 24)
        assert st["n"] >= 24 and st["ttft"] > 0 and len(st["tokens"]) == st["n"] + 1
        out.append((st["tokens"], st["counts"]))
    assert out[0] == out[1]
    assert s.document == g["prefill"]


def test_session_turn_keeps_the_answer_in_the_context(cpu_ops):
    from triforce_amd.utils.decoding import TriForceSession
    g = _golden()
    s = TriForceSession(Hh.FakeTokenizer(), Hh.build_product(g, "cpu"), g["gamma"], **GREEDY)
    s.prefill(Hh.prompt_of(g))
    st = s.generate(8)
    kv = s.run.eng.kv_cache
    assert kv.seq_len == g["prefill"] + st["n"]
    before = kv.seq_len
    st = s.turn(_question(g, 5, 41), 8)
    assert kv.seq_len == before + 1 + 5 + st["n"]


def test_bounds_are_refused_before_any_state_changes(cpu_ops):
    """Every refusal names its limit and leaves the runner as it was: a twin that was never disturbed emits the same stream."""
    g = _golden(gen_len=100, budget=64)          # tail bound 64 rows < the full cache's 116 rows of room
    doc = Hh.prompt_of(g)
    P, gamma = g["prefill"], g["gamma"]
    run, twin = _runner(g), _runner(g)
    with pytest.raises(ValueError, match="prefill"):
        run.extend(_question(g, 4, 1), keep=P)                        # never prefilled
    run.prefill(doc)
    twin.prefill(doc)
    _steps(run, 6)
    _steps(twin, 6)
    kv, rc = run.eng.kv_cache, run.eng.graph_cache
    S = kv.seq_len
    state = (S, list(run.emitted), run.next_token, run.n, run.rng.pos, rc.k.clone(), run.eng.draft_cache.k.clone())
    q = _question(g, 4, 1)
    with pytest.raises(ValueError, match=rf"keep={P - 1} is outside \[{P}, {S}\]"):
        run.extend(q, keep=P - 1)
    with pytest.raises(ValueError, match=rf"keep={S + 1} is outside"):
        run.extend(q, keep=S + 1)
    with pytest.raises(ValueError, match="at least one input token"):
        run.extend(torch.zeros((1, 0), dtype=torch.long), keep=P)
    with pytest.raises(ValueError, match="at least one input token"):
        run.extend([])
    # the tail: k + rows - P + gamma + 2 <= max_budget is the last length that fits
    fits = rc.max_budget - (gamma + 2)
    with pytest.raises(ValueError, match=r"retrieval budget max_budget=64"):
        run.extend(_question(g, fits + 1, 2), keep=P)
    with pytest.raises(ValueError, match=r"retrieval budget max_budget=64"):
        run.extend(_question(g, fits - (S - P), 2))                   # keep=None: the pending token is one more row
    assert (kv.seq_len, run.emitted, run.next_token, run.n, run.rng.pos) == state[:5]
    assert torch.equal(rc.k, state[5]) and torch.equal(run.eng.draft_cache.k, state[6])
    assert _steps(run, 14) == _steps(twin, 14)
    run.extend(_question(g, fits, 3), keep=P)                         # the bound itself is fine, and leaves room for a step
    run.step()
    assert kv.seq_len - P <= rc.max_budget

    # the full cache's capacity, on an engine whose retrieval budget is not the tighter limit
    g2 = _golden(gen_len=40, budget=320)                              # capacity 1000 + 40 + 16
    run2 = _runner(g2)
    run2.prefill(Hh.prompt_of(g2))
    cap = run2.eng.kv_cache.max_budget
    with pytest.raises(ValueError, match=rf"full cache's capacity max_budget={cap}"):
        run2.extend(_question(g2, cap - P - (gamma + 2) + 1, 4), keep=P)
    run2.extend(_question(g2, cap - P - (gamma + 2), 4), keep=P)
    run2.step()


def test_unsupported_engines_are_refused(cpu_ops):
    from triforce_amd.models.cache import OffloadingFlashSimpleCache
    from triforce_amd.utils.decoding import _DistEngine
    g = _golden()
    run = _runner(g)
    run.prefill(Hh.prompt_of(g))
    q = _question(g, 4, 1)
    ge, kv = run.ge, run.eng.kv_cache
    run.eng.kv_cache = OffloadingFlashSimpleCache.__new__(OffloadingFlashSimpleCache)
    with pytest.raises(NotImplementedError, match="OffloadingFlashSimpleCache"):
        run.extend(q, keep=g["prefill"])
    run.eng.kv_cache = kv
    run.ge = _DistEngine.__new__(_DistEngine)
    with pytest.raises(NotImplementedError, match="_DistEngine"):
        run.extend(q, keep=g["prefill"])
    run.ge = ge
    run.sync_record = lambda t: None                                  # the tensor-parallel loop's runner
    with pytest.raises(NotImplementedError, match="single-GPU"):
        run.extend(q, keep=g["prefill"])
    run.sync_record = None
    run.extend(q, keep=g["prefill"])
    run.step()


@pytest.mark.parametrize("keep_doc", [True, False])
def test_retrieval_cache_after_extend(cpu_ops, keep_doc):
    """The selection is made once per layer, by the LAST row's query, over rows [0, P): it equals what init_graph_cache
    gives a fresh retrieval cache for that query; the tail slots hold rows [P, seq_len) of the full cache."""
    from triforce_amd.models.cache import RetrievalCache
    g = _golden()
    P = g["prefill"]
    run = _runner(g)
    run.prefill(Hh.prompt_of(g))
    _steps(run, 9)
    kv, rc = run.eng.kv_cache, run.eng.graph_cache
    S = kv.seq_len
    q = _question(g, 19, 51)
    calls = []
    real = rc.init_graph_cache

    def spy(kv_cache, query_states, layer_idx):
        calls.append((layer_idx, query_states.clone(), kv_cache.seq_len))
        return real(kv_cache, query_states, layer_idx)
    rc.init_graph_cache = spy
    run.extend(q, keep=P if keep_doc else None)
    rc.init_graph_cache = real
    end = (P if keep_doc else S + 1) + 19
    assert kv.seq_len == end
    assert [c[0] for c in calls] == list(range(rc.layers))
    assert all(c[1].reshape(-1, rc.num_heads, rc.head_dim).shape[0] == 1 for c in calls)
    # ... all in the forward that fed the last row alone (the last layer's append has advanced seq_len by then)
    assert [c[2] for c in calls] == [end - 1] * (rc.layers - 1) + [end]
    fresh = RetrievalCache(run.eng.model, max_budget=g["budget"], prefill=P, gamma=g["gamma"], chunk_size=g["chunk"])
    tail = end - P
    B = rc.max_budget
    for layer, query, _ in calls:
        fresh.init_graph_cache(kv, query, layer)
        assert torch.equal(rc.last_idx[layer], fresh.last_idx[layer])
        assert torch.equal(rc.k[layer, :, :B - tail], fresh.k[layer, :, :B - tail])
        assert torch.equal(rc.v[layer, :, :B - tail], fresh.v[layer, :, :B - tail])
        assert torch.equal(rc.k[layer, :, B - tail:B], kv.k[layer, :, P:end])
        assert torch.equal(rc.v[layer, :, B - tail:B], kv.v[layer, :, P:end])


def test_document_rows_are_untouched_and_history_feeds_the_draft(cpu_ops):
    """Rows [0, P) of the full cache are bit-identical across extend, and the draft's window is the one a first prompt of
    the whole token history leaves on a fresh engine."""
    g = _golden()
    P = g["prefill"]
    doc, q = Hh.prompt_of(g), _question(g, 70, 61)
    run = _runner(g)
    run.prefill(doc)
    kv = run.eng.kv_cache
    k0, v0 = kv.k[:, :, :P].clone(), kv.v[:, :, :P].clone()
    _steps(run, 9)
    run.extend(q, keep=P)
    assert torch.equal(kv.k[:, :, :P], k0) and torch.equal(kv.v[:, :, :P], v0)
    assert torch.equal(run.history, torch.cat([doc, q], dim=1))
    fresh = Hh.build_product(g, "cpu")
    fresh.graph_draft_prefill(input_ids=run.history)
    dc, fdc = run.eng.draft_cache, fresh.engine.draft_cache
    assert dc.seq_len == fdc.seq_len
    assert torch.equal(dc.k[:, :, :dc.seq_len], fdc.k[:, :, :dc.seq_len])
    assert torch.equal(dc.v[:, :, :dc.seq_len], fdc.v[:, :, :dc.seq_len])


def test_on_chip_follow_up_flags():
    from triforce_amd.utils import cli
    a = cli.parse("on_chip", [])
    assert a.followups == 0 and a.followup_len == 0
    a = cli.parse("on_chip", ["--followups", "3", "--followup_len", "64"])
    assert (a.followups, a.followup_len) == (3, 64)
    for script in ("offloading", "offloading_TP", "offloading_seqouia"):          # the on-chip script's own flags
        with pytest.raises(SystemExit):
            cli.parse(script, ["--followups", "1"])
