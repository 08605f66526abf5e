"""Re-anchoring the retrieval cache and the chunk-mean index on CPU, every HIP op swapped for its oracle
restatement (cpu_ops; the two index ops are restated here): generation and sessions pass the retrieval budget, and what
comes out is still the target's own greedy continuation.  Host logic and the C ABI's argument checks only — the kernels are
checked in tests/test_gpu_reanchor.py."""
import ctypes

import pytest
import torch

from oracle import ref_ops as R
from tests import helpers as Hh

GREEDY = dict(top_k=-1, top_p=1e-9, temperature=1.0)           # --greedy: the only greedy the reference's sampler admits
GAP_TOL = 8e-3        # as tests/test_session_cpu.py: an emitted token may trail the target's argmax by ~2 fp16 spacings
# The seeds of the run that crosses the budget: small_gamma6's weights (tseed 201, dseed 202) and prompt seed 203 at
# prefill 128.  The plain loop (no re-anchoring, the parent's) keeps all but <= 2 of its first 60 tokens on the target's exact
# argmax for them (test_plain_loop_meets_the_argmax_condition_for_the_seed), so the cap of 2 below is a condition on the
# feature, not on the seed.
PSEED = 203
N = 48                # reanchor_at of every test here: 6 verify blocks of gamma + 2 = 8 rows


def _golden(**over):
    # retrieval budget 64 rows over a 128-row document: the generated tail reaches the budget after ~60 tokens
    return dict(Hh.load_golden("small_gamma6"), **dict(dict(prefill=128, budget=64, chunk=8, gen_len=300, pseed=PSEED), **over))


def _runner(g, ge=None, **kw):
    from triforce_amd.utils.decoding import TriForceRunner
    ge = ge or Hh.build_product(g, "cpu")
    return TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], **GREEDY, **kw)


def _question(g, n, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(3, g["tcfg"]["vocab_size"], (1, n), generator=gen)


def _steps(run, n):
    while run.n < n:
        run.step()
    return list(run.emitted)


def _follow(ar, stream):
    """Teacher-forced greedy check, worded as tests/test_session_cpu.py words DESIGN section 5's statement: ``ar`` is a
    runner over the same target whose pending token is stream[0]; it is stepped autoregressively over ``stream`` (one row per
    forward over its own full cache: no draft, no retrieval cache); every next token is within GAP_TOL of that forward's best
    logit, and exactly the best for all but <= 2 tokens."""
    assert ar.next_token == stream[0]
    gaps = []
    for i in range(len(stream) - 1):
        logits = ar.ge.decode_step(torch.tensor([[stream[i]]]))[0, -1]
        ar._fed.append(stream[i])
        gaps.append(float(logits.max() - logits[stream[i + 1]]))
    ar.next_token, ar.emitted = stream[-1], list(stream)
    print(f"teacher-forced gaps: max {max(gaps):.5f}, {sum(1 for x in gaps if x > 0.0)} of {len(gaps)} not the argmax")
    assert max(gaps) < GAP_TOL, f"token {gaps.index(max(gaps)) + 1} trails the target's argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x == 0.0) >= len(gaps) - 2


# ---- the two index ops, restated over the oracle (the product's are HIP kernels: csrc/retrieval.hip) ----
def _chunk_mean(k_layer, index_layer, c0, c1, chunk):
    """index[h, c] = fp16 mean of chunk c of K, c in [c0, c1): the means oracle.ref_ops.retrieval_scores forms."""
    assert 0 <= c0 <= c1 <= index_layer.shape[1] and c1 * chunk <= k_layer.shape[1]
    if c1 > c0:
        means = R.retrieval_chunk_means(k_layer.permute(1, 0, 2), c1 * chunk, chunk)          # (C, H, D)
        index_layer[:, c0:c1] = means[c0:c1].permute(1, 0, 2)


def _score_indexed(index_layer, q, chunks):
    kbar = index_layer[:, :chunks].permute(1, 0, 2).contiguous()                              # (C, H, D), as ref_ops holds it
    return torch.matmul(q.unsqueeze(1), kbar.permute(1, 2, 0)).squeeze(1)


@pytest.fixture
def index_ops(cpu_ops, monkeypatch):
    """cpu_ops plus the restated index ops; returns the list of (c0, c1) ranges chunk_mean was asked for."""
    asked = []

    def chunk_mean(k_layer, index_layer, c0, c1, chunk):
        asked.append((c0, c1))
        _chunk_mean(k_layer, index_layer, c0, c1, chunk)
    monkeypatch.setattr(cpu_ops, "chunk_mean", chunk_mean)
    monkeypatch.setattr(cpu_ops, "retrieval_score_indexed", _score_indexed)
    return asked


# ---- 1. crossing the budget ----
def test_plain_loop_meets_the_argmax_condition_for_the_seed(cpu_ops):
    """The condition the seed was picked by: without re-anchoring, the first 60 tokens are within the cap."""
    g = _golden()
    doc = Hh.prompt_of(g)
    spec, ar = _runner(g), _runner(g)
    spec.prefill(doc)
    ar.prefill(doc)
    _follow(ar, _steps(spec, 56)[:61])            # (56 tokens + one step's <= 7 more stay within the 64-row tail bound)


def test_generation_crosses_the_retrieval_budget(cpu_ops, monkeypatch):
    """200 generated tokens over a 64-row retrieval budget.  Without the feature this call fails: TriForce() takes no
    ``reanchor_at``, and the plain loop raises IndexError in _copy_tail once the tail passes the budget (that crash:
    test_reanchor_at_zero_is_the_plain_runner)."""
    from triforce_amd.utils import decoding as Dm
    g = _golden()
    gamma, doc = g["gamma"], Hh.prompt_of(g)
    real, runs = Dm.TriForceRunner.step, []

    def step(run):                                 # every step of the run below: the invariants that hold between steps
        out = real(run)
        kv, rc = run.eng.kv_cache, run.eng.graph_cache
        assert rc.prefill % 8 == 0 and rc.chunks == rc.prefill // 8
        assert kv.seq_len - rc.prefill + gamma + 2 <= 64
        runs[:] = [run]
        return out
    monkeypatch.setattr(Dm.TriForceRunner, "step", step)
    st = Dm.TriForce(Hh.FakeTokenizer(), Hh.build_product(g, "cpu"), doc, gamma=gamma, max_len=200, return_details=True,
                     reanchor_at=N, **GREEDY)
    run, = runs
    assert st["n"] >= 200 and len(st["tokens"]) == st["n"] + 1 and st["tokens"] == run.emitted
    rc = run.eng.graph_cache
    assert run.reanchors >= 3 and rc.prefill > rc.prefill0 == g["prefill"]
    ar = _runner(g)
    ar.prefill(doc)
    _follow(ar, run.emitted)
    assert run.eng.kv_cache.seq_len == g["prefill"] + len(run.emitted) - 1 == ar.eng.kv_cache.seq_len


# ---- 2. state after a re-anchor ----
def test_retrieval_cache_after_a_reanchor(cpu_ops):
    """The step that re-anchors re-selects once per layer, by the query of the verify's first row, over rows [0, P'): the
    selection is what init_graph_cache gives a fresh RetrievalCache(prefill=P') for that query, the selected slots hold the
    named chunks bit for bit, and the tail slots hold rows [P', seq_len)."""
    from triforce_amd.models.cache import RetrievalCache
    g = _golden()
    run = _runner(g, reanchor_at=N)
    run.prefill(Hh.prompt_of(g))
    kv, rc = run.eng.kv_cache, run.eng.graph_cache
    calls = []
    real = rc.init_graph_cache

    def spy(kv_cache, query_states, layer_idx):
        calls.append((layer_idx, query_states.clone(), rc.prefill))
        return real(kv_cache, query_states, layer_idx)
    rc.init_graph_cache = spy
    seen = 0
    while seen < 2:
        before, S = run.reanchors, kv.seq_len
        del calls[:]
        run.step()
        if run.reanchors == before:
            assert calls == []
            continue
        seen += 1
        P = (S // 8) * 8
        assert rc.prefill == P > g["prefill"] and [c[0] for c in calls] == list(range(rc.layers))
        assert all(c[2] == P and c[1].reshape(-1, rc.num_heads, rc.head_dim).shape[0] == 1 for c in calls)
        fresh = RetrievalCache(run.eng.model, max_budget=g["budget"], prefill=P, gamma=g["gamma"], chunk_size=8)
        B, tail = rc.max_budget, kv.seq_len - P
        assert 0 < tail <= 7 + g["gamma"] + 2
        for layer, query, _ in calls:
            fresh.init_graph_cache(kv, query, layer)
            assert torch.equal(rc.last_idx[layer], fresh.last_idx[layer])
            assert torch.equal(rc.last_scores[layer], fresh.last_scores[layer]) and rc.last_scores[layer].shape[1] == P // 8
            rows = (rc.last_idx[layer].long().unsqueeze(-1) * 8 + torch.arange(8)).reshape(rc.num_heads, B)
            for h in range(rc.num_heads):
                assert torch.equal(rc.k[layer, h, :B - tail], kv.k[layer, h, rows[h, :B - tail]])
                assert torch.equal(rc.v[layer, h, :B - tail], kv.v[layer, h, rows[h, :B - tail]])
            assert torch.equal(rc.k[layer, :, B - tail:B], kv.k[layer, :, P:kv.seq_len])
            assert torch.equal(rc.v[layer, :, B - tail:B], kv.v[layer, :, P:kv.seq_len])


# ---- 3. reanchor_at = 0 ----
def _refusals(run, g):
    """The message of every extend() refusal this runner gives (tests/test_session_cpu.py's list)."""
    P, S, gamma = g["prefill"], run.eng.kv_cache.seq_len, g["gamma"]
    fits = run.eng.graph_cache.max_budget - (gamma + 2)
    cap = run.eng.kv_cache.max_budget
    out = []
    for ids, keep in ((_question(g, 4, 1), P - 1), (_question(g, 4, 1), S + 1), (torch.zeros((1, 0), dtype=torch.long), P),
                      ([], None), (_question(g, fits + 1, 2), P), (_question(g, fits - (S - P), 2), None),
                      (_question(g, cap - P - (gamma + 2) + 1, 4), P)):
        with pytest.raises(ValueError) as e:
            run.extend(ids, keep=keep)
        out.append(str(e.value))
    return out


def test_reanchor_at_zero_is_the_plain_runner(cpu_ops):
    g = _golden()
    doc = Hh.prompt_of(g)
    plain, zero = _runner(g), _runner(g, reanchor_at=0)
    for run in (plain, zero):
        with pytest.raises(ValueError, match="prefill"):
            run.extend(_question(g, 4, 1), keep=g["prefill"])
        run.prefill(doc)
        _steps(run, 30)
    assert (plain.emitted, plain.counts, plain.rng.pos) == (zero.emitted, zero.counts, zero.rng.pos)
    a, b = _refusals(plain, g), _refusals(zero, g)
    assert a == b and len(set(a)) >= 5
    assert any("the covered region [0, 128) is fixed when the engine is built" in m for m in a)
    assert (_steps(plain, 44), plain.counts) == (_steps(zero, 44), zero.counts)
    assert zero.reanchors == 0 and zero.eng.graph_cache.prefill == g["prefill"]
    with pytest.raises(IndexError, match="exceeds the retrieval budget"):
        _steps(zero, 200)


# ---- 4. extend across the bound ----
def test_chat_turns_cross_the_retrieval_budget(cpu_ops):
    """Three chat turns of 20, 70 and 20 rows (+ the pending token) with 14-token answers against a 64-row budget: the
    second cannot fit whatever the tail held, so extend() itself re-anchors, between the body rows and the last row."""
    g = _golden()
    doc = Hh.prompt_of(g)
    turns = [_question(g, n, 21 + i) for i, n in enumerate((20, 70, 20))]
    spec, ar, plain = _runner(g, reanchor_at=N), _runner(g, reanchor_at=N), _runner(g)
    for run in (spec, ar, plain):
        run.prefill(doc)
    _follow(ar, _steps(spec, 10))
    _steps(plain, 10)
    moved = 0
    for t in turns:
        before = spec.eng.kv_cache.seq_len
        spec.extend(t)
        ar.extend(t)
        rc = spec.eng.graph_cache
        assert spec.eng.kv_cache.seq_len == before + 1 + t.shape[1] == ar.eng.kv_cache.seq_len
        if t.shape[1] == 70:
            assert spec.reanchors == 1 and rc.prefill == ((spec.eng.kv_cache.seq_len - 1) // 8) * 8
        assert rc.prefill % 8 == 0 and spec.eng.kv_cache.seq_len - rc.prefill + g["gamma"] + 2 <= 64
        _follow(ar, _steps(spec, 14))
        moved += spec.reanchors
    assert moved >= 2 and spec.eng.kv_cache.seq_len > g["prefill"] + 64
    assert torch.equal(spec.history, ar.history) and spec._fed == ar._fed
    with pytest.raises(ValueError, match=r"retrieval budget max_budget=64: the covered region \[0, 128\) is fixed"):
        for t in turns:
            plain.extend(t)
            _steps(plain, 14)


def test_question_on_the_document_after_the_region_has_grown(cpu_ops):
    """ask(keep=document) once the covered region has grown into earlier answers re-anchors down to the document, and the
    answer equals — tokens and accept counts — that of asking the same question first (DESIGN section 18's check)."""
    from triforce_amd.utils.decoding import TriForceSession
    g = _golden()
    doc, q = Hh.prompt_of(g), _question(g, 12, 32)
    out = []
    for grown in (True, False):
        s = TriForceSession(Hh.FakeTokenizer(), Hh.build_product(g, "cpu"), g["gamma"], reanchor_at=N, **GREEDY)
        s.prefill(doc)
        s.generate(10)
        rc = s.run.eng.graph_cache
        if grown:
            s.turn(_question(g, 30, 31), 60)
            assert rc.prefill > g["prefill"] and s.document == g["prefill"]
            with pytest.raises(ValueError, match=rf"keep={g['prefill'] - 1} is outside \[{g['prefill']}, "):
                s.ask(q, 24, keep=g["prefill"] - 1)
        st = s.ask(q, 24)
        assert rc.prefill == g["prefill"] and st["n"] >= 24
        out.append((st["tokens"], st["counts"]))
    assert out[0] == out[1]


# ---- 5. refusals ----
def test_refusals_leave_the_runner_as_it_was(cpu_ops):
    from triforce_amd.models.cache import OffloadingFlashSimpleCache
    from triforce_amd.utils.decoding import TriForceRunner, _DistEngine
    g = _golden()
    gamma, doc = g["gamma"], Hh.prompt_of(g)
    run, twin = _runner(g, reanchor_at=N), _runner(g, reanchor_at=N)
    run.prefill(doc)
    twin.prefill(doc)
    _steps(run, 6)
    _steps(twin, 6)
    ge, kv, rc = run.ge, run.eng.kv_cache, run.eng.graph_cache
    state = (kv.seq_len, rc.prefill, rc.chunks, rc.k.clone())
    for bad in (gamma + 1, 65, -1):
        with pytest.raises(ValueError, match=rf"reanchor_at={bad} is outside \[gamma \+ 2, max_budget\] = \[8, 64\]"):
            TriForceRunner(Hh.FakeTokenizer(), ge, gamma, reanchor_at=bad, **GREEDY)
    for ok in (gamma + 2, 64):
        TriForceRunner(Hh.FakeTokenizer(), Hh.build_product(g, "cpu"), gamma, reanchor_at=ok, **GREEDY)
    with pytest.raises(ValueError, match="new_prefill=132 is not a multiple of chunk_size=8"):
        rc.reanchor(132)
    with pytest.raises(ValueError, match="new_prefill=120 is below prefill0=128"):
        rc.reanchor(120)
    with pytest.raises(ValueError, match="32769 chunks of 8 rows, more than the top-k's limit of 32768 chunks"):
        rc.reanchor(32769 * 8)
    run.eng.kv_cache = OffloadingFlashSimpleCache.__new__(OffloadingFlashSimpleCache)
    with pytest.raises(NotImplementedError, match="reanchor_at is implemented for the resident FlashSimpleCache"):
        TriForceRunner(Hh.FakeTokenizer(), ge, gamma, reanchor_at=N, **GREEDY)
    run.eng.kv_cache = kv
    dist = _DistEngine.__new__(_DistEngine)
    dist.engine = ge.engine
    with pytest.raises(NotImplementedError, match="reanchor_at is implemented for the single-GPU resident .* _DistEngine"):
        TriForceRunner(Hh.FakeTokenizer(), dist, gamma, reanchor_at=N, **GREEDY)
    with pytest.raises(NotImplementedError, match="single-GPU"):
        TriForceRunner(Hh.FakeTokenizer(), ge, gamma, reanchor_at=N, sync_record=lambda t: None, **GREEDY)
    assert (kv.seq_len, rc.prefill, rc.chunks) == state[:3] and torch.equal(rc.k, state[3])
    assert (_steps(run, 80), run.counts, run.reanchors) == (_steps(twin, 80), twin.counts, twin.reanchors)
    assert run.reanchors >= 1
    rc.reanchor(rc.prefill0)                                        # shrinking is legal, and exactly the chunk-count limit is
    rc.reanchor(32768 * 8)
    assert (rc.prefill, rc.chunks) == (32768 * 8, 32768)


def test_on_chip_reanchor_flag():
    from triforce_amd.utils import cli
    assert cli.parse("on_chip", []).reanchor_at == 0
    assert cli.parse("on_chip", ["--reanchor_at", "1024"]).reanchor_at == 1024
    assert "--reanchor_at" in [f[0] for f in cli.SCRIPT_OWN["on_chip"]]
    assert "--reanchor_at" not in [f[0] for f in cli.SCRIPTS["on_chip"]]       # the table compared with the reference's
    for script in ("offloading", "offloading_TP", "offloading_seqouia"):
        with pytest.raises(SystemExit):
            cli.parse(script, ["--reanchor_at", "8"])


# ---- 6. the chunk-mean index: host logic ----
def test_restated_index_ops_agree_with_the_oracle_scorer():
    gen = torch.Generator().manual_seed(5)
    k = torch.randn(2, 80, 64, generator=gen).half()
    q = torch.randn(2, 64, generator=gen).half()
    index = torch.full((2, 10, 64), 7.0, dtype=torch.float16)
    _chunk_mean(k, index, 0, 5, 8)
    _chunk_mean(k, index, 5, 9, 8)
    assert torch.equal(_score_indexed(index, q, 9), R.retrieval_scores(k.permute(1, 0, 2), q, 72, 8))
    assert bool((index[:, 9] == 7.0).all())


def test_index_on_and_off_select_the_same(index_ops, monkeypatch):
    """Two engines from the same seeds, one with the index: every build — the prompt's, each re-anchor's, extend's — gives
    identical scores and indices, the index grows only by the new chunks, and a downward re-anchor truncates it."""
    from triforce_amd.models import cache as C
    g = _golden()
    doc = Hh.prompt_of(g)
    off = _runner(g, reanchor_at=N)
    monkeypatch.setenv(C.RETRIEVAL_INDEX_ENV, "1")                  # read when the cache is constructed
    on = _runner(g, reanchor_at=N)
    monkeypatch.delenv(C.RETRIEVAL_INDEX_ENV)
    rc_on, rc_off = on.eng.graph_cache, off.eng.graph_cache
    assert rc_on.use_index and not rc_off.use_index and rc_on.index is None and rc_off.index is None
    L, kv = rc_on.layers, on.eng.kv_cache

    def same():
        for layer in range(L):
            assert torch.equal(rc_on.last_scores[layer], rc_off.last_scores[layer])
            assert torch.equal(rc_on.last_idx[layer], rc_off.last_idx[layer])
        assert torch.equal(rc_on.k, rc_off.k) and torch.equal(rc_on.v, rc_off.v)
    on.prefill(doc)
    off.prefill(doc)
    assert index_ops == [(0, 16)] * L and rc_on.indexed_chunks == [16] * L and rc_off.index is None
    assert tuple(rc_on.index.shape) == (L, rc_on.num_heads, kv.max_budget // 8, rc_on.head_dim)
    same()
    del index_ops[:]
    builds = 0
    while on.n < 120:
        before, done = on.reanchors, rc_on.indexed_chunks[0]
        on.step()
        off.step()
        if on.reanchors > before:
            builds += 1
            assert index_ops == [(done, rc_on.chunks)] * L and done < rc_on.chunks == rc_on.prefill // 8
            assert rc_on.indexed_chunks == [rc_on.chunks] * L
            same()
            del index_ops[:]
        assert index_ops == []
    assert builds >= 2 and (on.emitted, on.counts) == (off.emitted, off.counts)
    # the means are those of the rows they cover
    want = torch.zeros_like(rc_on.index[0])
    _chunk_mean(kv.k[0], want, 0, rc_on.chunks, 8)
    assert torch.equal(rc_on.index[0, :, :rc_on.chunks], want[:, :rc_on.chunks])
    # a question on the document: down to 16 chunks, nothing new to compute (rows [0, 128) never change)
    q = _question(g, 12, 32)
    on.extend(q, keep=g["prefill"])
    off.extend(q, keep=g["prefill"])
    assert rc_on.prefill == g["prefill"] and rc_on.indexed_chunks == [16] * L and index_ops == []
    same()
    assert (_steps(on, 70), on.counts) == (_steps(off, 70), off.counts)           # ... and up again over the NEW rows
    assert on.reanchors >= 1 and index_ops[:L] == [(16, index_ops[0][1])] * L and index_ops[0][1] > 16
    want = torch.zeros_like(rc_on.index[1])
    _chunk_mean(kv.k[1], want, 0, rc_on.chunks, 8)
    assert torch.equal(rc_on.index[1, :, :rc_on.chunks], want[:, :rc_on.chunks])
    # a new prompt starts the index over
    on.prefill(doc)
    assert rc_on.prefill == g["prefill"] and rc_on.indexed_chunks == [16] * L and index_ops[-L:] == [(0, 16)] * L


def test_index_keyword_and_environment(cpu_ops, monkeypatch):
    from triforce_amd.models import cache as C
    g = _golden()
    model = Hh.build_product(g, "cpu").engine.model
    kw = dict(max_budget=64, prefill=128, gamma=6, chunk_size=8)
    assert not C.RetrievalCache(model, **kw).use_index
    assert C.RetrievalCache(model, index=True, **kw).use_index
    monkeypatch.setenv(C.RETRIEVAL_INDEX_ENV, "1")
    assert C.RetrievalCache(model, **kw).use_index and not C.RetrievalCache(model, index=False, **kw).use_index
    monkeypatch.setenv(C.RETRIEVAL_INDEX_ENV, "yes")
    with pytest.raises(ValueError, match="TRIFORCE_RETRIEVAL_INDEX"):
        C.RetrievalCache(model, **kw)
    import inspect
    for cls in (C.DistributedRetrievalCache, C.DistributedRetrievalCache_Seqouia):
        assert "index" not in inspect.signature(cls.__init__).parameters


# ---- 7. the C ABI's argument checks (no device) ----
def test_index_entry_points_reject_bad_arguments():
    from triforce_amd import hip
    lib = hip.lib()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)               # (never dereferenced: every call below is refused)
    ok = dict(k=p, st=128, sh=128 * 64, index=p, ish=128 * 8, c0=0, c1=8, chunk=8, H=2, D=128)

    def mean(**over):
        a = dict(ok, **over)
        return lib.tf_chunk_mean(a["k"], a["st"], a["sh"], a["index"], a["ish"], a["c0"], a["c1"], a["chunk"], a["H"], a["D"], null)
    for bad in (dict(k=null), dict(index=null), dict(c0=3, c1=2), dict(c0=-1), dict(chunk=0), dict(D=96), dict(D=256), dict(H=0),
                dict(st=132), dict(ish=128 * 8 + 4), dict(ish=128 * 7)):
        assert mean(**bad) == -22, bad
    ok_s = dict(index=p, ish=128 * 8, q=p, scores=p, C=8, H=2, D=64)

    def score(**over):
        a = dict(ok_s, **over)
        return lib.tf_retrieval_score_indexed(a["index"], a["ish"], a["q"], a["scores"], a["C"], a["H"], a["D"], null)
    for bad in (dict(index=null), dict(q=null), dict(scores=null), dict(C=0), dict(H=0), dict(D=32), dict(ish=64 * 7),
                dict(ish=64 * 8 + 2)):
        assert score(**bad) == -22, bad
    assert mean(c0=5, c1=5) == 0                                    # an empty range is valid and launches nothing
