"""Repetition / frequency / presence penalties on the device: tf_penalize_logits bit for bit against the
torch fp32 restatement (tests/penalty_ref.py) on its vector and its scalar path, tf_penalty_commit against torch.bincount,
graph replay over live state, and the captured target verify / decode loops with penalties on."""
import pytest
import torch

from oracle import specs
from tests import helpers as Hh
from tests import logprobs_ref as LR
from tests import penalty_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP_TOL = 8e-3        # as tests/test_gpu_e2e.py: an emitted token may trail the target's argmax by ~2 fp16 spacings
PEN = (1.3, 0.2, 0.1)
PEN_KW = dict(repetition_penalty=PEN[0], frequency_penalty=PEN[1], presence_penalty=PEN[2])
PAD_TOKEN = 100


def _ops():
    from triforce_amd import ops
    return ops


def _pen(*a):
    from triforce_amd.utils.sampling import Penalties
    return Penalties(*a)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def _case(V, rows):
    """(logits, ids, gen_count, prompt_seen) on the CPU with every planted case: a token twice in the block, an id that is
    prompt-seen only, ids with gen_count > 0 (in and out of the prompt), logits 0.0 / -0.0 / -inf at penalised entries."""
    gen = torch.Generator().manual_seed(1000 * rows + V % 997)
    lg = torch.randn(rows, V, generator=gen) * 3.0
    gc = torch.zeros(V, dtype=torch.int32)
    ps = torch.zeros(V, dtype=torch.uint8)
    ps[torch.randint(0, V, (V // 5,), generator=gen)] = 1
    hot = torch.randint(0, V, (V // 9,), generator=gen)
    gc[hot] = torch.randint(1, 9, (hot.numel(),), generator=gen, dtype=torch.int32)
    ps[[1, 9, V - 1]] = 1
    gc[[1, 9]] = 0                                                     # prompt-seen only
    gc[3], ps[3] = 2, 0                                                # generated only
    gc[5], ps[5] = 1, 1                                                # both
    gc[V - 2] = 7
    gc[[11, 12]], ps[[11, 12]] = 0, 0
    ids = torch.randint(0, V, (rows,), generator=gen)
    ids[0] = 11                                                        # neither seen nor counted before this block
    if rows > 1:
        ids[1] = 13
    if rows > 2:
        ids[2] = 11                                                    # twice in the block
    if rows > 3:
        ids[3] = 9                                                     # a prompt-seen token drafted
    if rows > 4:
        ids[4] = V - 1                                                 # the last entry (a scalar tail at V = 1003)
    lg[:, 1] = 0.0
    lg[:, 9] = -0.0
    lg[:, 3] = float("-inf")
    lg[:, 5] = 2.5
    lg[0, 11] = 1.75
    lg[-1, V - 2] = -1.25
    return lg, ids, gc, ps


@pytest.mark.parametrize("rows", [1, 7, 8, 18, 64])
@pytest.mark.parametrize("V", [1003, 32000, 128256])
def test_penalize_logits_equals_the_reference_bit_for_bit_on_both_paths(V, rows):
    ops = _ops()
    lg, ids, gc, ps = _case(V, rows)
    st = ops.PenaltyState(V, DEV)
    st.gen_count.copy_(gc)
    st.prompt_seen.copy_(ps)
    d_ids = ids.to(DEV)
    raw = _bits(lg)

    def strided(t, stride, offset=0):
        """``t`` in a fresh device buffer with this row stride, ``offset`` floats behind a 16-byte boundary."""
        buf = torch.full((rows * stride + offset + 8,), 7.0, dtype=torch.float32, device=DEV)
        view = buf[offset:offset + rows * stride].view(rows, stride)[:, :V]
        view.copy_(t)
        return view

    # (input stride, output stride, input offset, output offset, ids, alias): 16-byte loads need V, both strides % 4 == 0 and
    # aligned bases — the first two, the NULL-ids one and the aliased one take them at V % 4 == 0; the rest are scalar
    variants = [("contiguous", V, V, 0, 0, True, False), ("padded x4", V + 4, V + 8, 0, 0, True, False),
                ("odd input stride", V + 1, V, 0, 0, True, False), ("odd output stride", V, V + 3, 0, 0, True, False),
                ("unaligned input base", V, V, 1, 0, True, False), ("unaligned output base", V + 4, V + 4, 0, 3, True, False),
                ("no ids", V, V, 0, 0, False, False), ("out == logits", V + 4, V + 4, 0, 0, True, True),
                ("out == logits, scalar", V + 1, V + 1, 0, 0, True, True)]
    for pen in ((1.3, 0.2, 0.1), (0.7, -0.3, 0.05)):                   # (repetition < 1 and a negative frequency among them)
        want = {use: PR.penalize(lg, ids if use else None, gc, ps, *pen) for use in (True, False)}
        c = {use: PR.counts(gc, ids if use else None, rows, V) for use in (True, False)}
        for name, ls, os_, off_in, off_out, use_ids, alias in variants:
            x = strided(lg, ls, off_in)
            out = x if alias else strided(torch.full((rows, V), -3.0), os_, off_out)
            assert (x.data_ptr() % 16 == 0) == (off_in % 4 == 0) and x.stride(0) == ls
            got = ops.penalize_logits(x, d_ids if use_ids else None, st, _pen(*pen), out=out)
            assert got is out
            got = got.cpu()
            w = want[use_ids]
            same = _bits(got) == _bits(w)
            assert bool(same.all()), (f"{name} pen={pen}: {int((~same).sum())} entries differ, first at "
                                      f"{(~same).nonzero()[0].tolist()}")
            if not alias:
                assert torch.equal(_bits(x.cpu()), raw), f"{name}: the input was written"
            untouched = (ps == 0).unsqueeze(0) & (c[use_ids] == 0)
            assert torch.equal(_bits(got)[untouched], raw[untouched]), f"{name}: an entry that is not seen changed"
            assert bool((got[:, 3] == float("-inf")).all())
        # the planted cases did bite, and row i never sees ids[j > i]
        y = want[True]
        assert int(c[True][0, 11]) == 1 and float(y[0, 11]) != float(lg[0, 11])
        if rows > 2:
            assert c[True][:, 11].tolist()[:3] == [1, 1, 2]
        assert torch.equal(_bits(want[False][:, 11]), _bits(lg[:, 11]))         # without ids 11 is untouched
        assert float(y[0, 5]) != 2.5 and float(want[False][0, 1]) == 0.0
        assert _bits(y[0, 9:10]).tolist() == _bits(torch.tensor([-0.0])).tolist()   # -0.0 * r = -0.0
    assert torch.equal(st.gen_count.cpu(), gc) and torch.equal(st.prompt_seen.cpu(), ps)       # the state is only read


def test_penalty_commit_equals_bincount():
    ops = _ops()
    V = 1003
    st = ops.PenaltyState(V, DEV)
    gen = torch.Generator().manual_seed(5)
    total = torch.zeros(V, dtype=torch.long)
    for n in (1, 7, 8, 64, 33):
        ids = torch.randint(0, V, (64,), generator=gen)
        ids[: n // 2] = 17                                             # duplicates accumulate
        if n > 3:
            ids[n - 1], ids[n - 2], ids[n - 3] = -1, V, V + PAD_TOKEN   # outside [0, V): skipped
        ops.penalty_commit(st, ids.to(DEV), n)
        head = ids[:n]
        total += torch.bincount(head[(head >= 0) & (head < V)], minlength=V)
        assert torch.equal(st.gen_count.cpu().long(), total), n
    before = st.gen_count.clone()
    ops.penalty_commit(st, torch.full((8,), 5, dtype=torch.long, device=DEV), 0)
    assert torch.equal(st.gen_count, before)                          # n = 0: a no-op
    small = ops.PenaltyState(64, DEV)
    ops.penalty_commit(small, torch.tensor([PAD_TOKEN, 3, 64, -1, 3], device=DEV), 5)       # PAD_TOKEN past a small vocabulary
    assert small.gen_count.cpu().tolist() == [0, 0, 0, 2] + [0] * 60
    st.reset(torch.tensor([[3, 3, 9, V + 5, -2]], device=DEV))
    assert int(st.gen_count.sum()) == 0 and st.prompt_seen.nonzero().view(-1).tolist() == [3, 9]


def test_twenty_launches_in_one_graph_read_the_live_state():
    """Pointers are baked into the graph, values are live: replay, commit, replay — the second replay reflects the new counts."""
    ops = _ops()
    V, rows = 32000, 7
    lg, ids, gc, ps = _case(V, rows)
    st = ops.PenaltyState(V, DEV)
    st.gen_count.copy_(gc)
    st.prompt_seen.copy_(ps)
    x, d_ids, pen = lg.to(DEV), ids.to(DEV), _pen(*PEN)
    ops.penalize_logits(x, d_ids, st, pen)
    torch.cuda.synchronize()
    outs = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(20):
            outs.append(ops.penalize_logits(x, d_ids if i % 2 == 0 else None, st, pen))
    commit = torch.tensor([11, 11, 4242, 9], device=DEV)
    for step in range(2):
        for o in outs:
            o.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        want = [PR.penalize(lg, ids if use else None, st.gen_count.cpu(), ps, *PEN) for use in (True, False)]
        for i, o in enumerate(outs):
            assert torch.equal(_bits(o.cpu()), _bits(want[i % 2])), f"replay {step}, launch {i}"
        if step == 0:
            first = want[1]
            ops.penalty_commit(st, commit, 4)
    assert float(want[1][0, 4242]) != float(first[0, 4242])           # the commit showed in the second replay


# ---- the engine ---------------------------------------------------------------------------------------------------------------
def _golden(large):
    if not large:
        return dict(Hh.load_golden("small_gamma6"), gen_len=100, budget=320)
    return dict(tcfg=specs.tiny_target_config(vocab_size=128256, max_pos=131072), dcfg=specs.draft_68m_config(vocab_size=128256),
                tseed=1, dseed=2, pseed=3, head_std=0.05, prefill=2048, gen_len=96, budget=256, chunk=8, gamma=6,
                temperature=0.6, top_p=0.9)


_WEIGHTS = {}


def _engine(large, graphs, penalties):
    """min_p = 1 at temperature 1, top-p 1: the target's distribution is the row maximum of the penalised logits."""
    g = _golden(large)
    if large not in _WEIGHTS:
        _WEIGHTS[large] = (specs.random_state_dict(g["tcfg"], g["tseed"], head_std=0.05),
                           specs.random_state_dict(g["dcfg"], g["dseed"], head_std=0.05))
    tsd, dsd = _WEIGHTS[large]
    return g, PR.build_engine(g, DEV, graphs, penalties, min_p=1.0, tsd=tsd, dsd=dsd)[0]


def _runner(g, ge, penalties, seed=41, **kw):
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.sampling import UniformSource
    return TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], top_p=1.0, temperature=1.0, min_p=1.0,
                          rng=UniformSource(DEV, values=Hh.fixed_uniforms(seed=seed)), repetition_penalty=penalties[0],
                          frequency_penalty=penalties[1], presence_penalty=penalties[2], **kw)


def _stream(g, ge, penalties, n, **kw):
    run = _runner(g, ge, penalties, **kw)
    run.prefill(Hh.prompt_of(g).to(DEV))
    while run.n < n:
        run.step()
    return run


def _check_state(ge, g, emitted):
    st = ge.penalty_state
    hist = torch.bincount(torch.tensor(emitted[:-1]), minlength=st.V)
    assert torch.equal(st.gen_count.cpu().long(), hist), "gen_count is not the histogram of emitted[:-1]"
    seen = torch.zeros(st.V, dtype=torch.uint8)
    seen[Hh.prompt_of(g).reshape(-1)] = 1
    assert torch.equal(st.prompt_seen.cpu(), seen)


def test_captured_verify_is_the_eager_penalty_and_normaliser_on_its_own_logits():
    from triforce_amd.utils.sampling import norm_logits
    ops = _ops()
    g, ge = _engine(False, True, PEN)
    gamma, pen = g["gamma"], _pen(*PEN)
    assert ge.target_penalties == pen and ge.penalty_state is not None and not any("penalt" in k for k in ge.sampling)
    run = _stream(g, ge, PEN, 12)
    assert run._device_sets() is not None and run._served()
    st = ge.penalty_state
    _check_state(ge, g, run.emitted)
    kv = ge.engine.kv_cache
    for q_len in (gamma + 1, gamma + 2):
        tg = ge.target_graphs[q_len]
        assert tg.pen_rows is not None and tg.pen_rows.data_ptr() != tg.logits.data_ptr()
        S0 = kv.seq_len
        ids = [run.next_token] + [run.emitted[0], 5, run.emitted[0], 9, 5, 11, 12][:q_len - 1]
        assert ge.verify_probs_ids(ids, 1.0, 1.0, min_p=1.0) is None                      # a caller without penalties is not served
        assert ge.verify_probs_ids(ids, 1.0, 1.0, min_p=1.0, penalties=_pen(1.3, 0.2, 0.0)) is None and kv.seq_len == S0
        fast = ge.verify_probs_ids(ids, 1.0, 1.0, min_p=1.0, penalties=pen)
        assert fast is not None and fast[0] is tg.out_probs and fast[1].view(-1).tolist() == ids
        kv.seq_len = S0                                               # (the probe's rows are dropped again)
        rows = ops.penalize_logits(tg.logits[0], tg.ids[0], st, pen)
        assert torch.equal(_bits(rows), _bits(tg.pen_rows)), f"q_len={q_len}: the graph's penalised rows differ from the eager ones"
        want = norm_logits(rows, **ge.target_filters.kw())
        assert torch.equal(_bits(tg.out_probs), _bits(want)), f"q_len={q_len}: the captured probabilities differ"
        # tg.logits holds the RAW rows: the (strictly monotone) map of it is pen_rows, and it is not pen_rows itself
        ref = PR.penalize(tg.logits[0].cpu(), ids, st.gen_count, st.prompt_seen, *PEN)
        assert torch.equal(_bits(ref), _bits(tg.pen_rows.cpu()))
        changed = (_bits(tg.logits[0]) != _bits(tg.pen_rows)).sum(-1)
        assert int(changed.min()) > 0 and ge.last_logits is tg.logits
    ge.dev_len = None


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_presence_penalty_makes_every_emitted_token_distinct_on_device(graphs):
    g, ge = _engine(False, graphs, (1.0, 0.0, 1e4))
    run = _stream(g, ge, (1.0, 0.0, 1e4), 48)
    assert (run._device_sets() is not None) == graphs
    toks = list(run.emitted)
    assert len(set(toks)) == len(toks), f"a token was emitted twice: {toks}"
    assert run.resample_count > 0
    _check_state(ge, g, toks)


def _check_penalised_stream(g, run, plain, what):
    stream = list(run.emitted)
    gaps = PR.teacher_forced_penalised_gaps(g, stream, PEN, Hh.build_oracle, Hh.prompt_of(g))
    Hh.note(f"penalties {PEN} {what} (V={g['tcfg']['vocab_size']}): {len(stream)} tokens, max penalised teacher-forced gap "
            f"{max(gaps):.5f}, {sum(1 for x in gaps if x != 0.0)} not the argmax, {run.resample_count} resampled, "
            f"acceptance {run.accepted_count / max(run.draft_count, 1):.3f}")
    assert max(gaps) <= GAP_TOL * PEN[0], f"token {gaps.index(max(gaps))} trails the penalised argmax by {max(gaps):.4f}"
    if plain is not None:
        assert stream != plain[:len(stream)], "the penalised stream is the unpenalised one"


@pytest.mark.parametrize("route", ["eager", "graphs", "no-target-graph", "tiny-v128k"])
def test_penalised_stream_is_the_penalised_argmax_of_the_oracle_on_device(route, monkeypatch):
    large = route == "tiny-v128k"
    if route == "no-target-graph":
        monkeypatch.setenv("TRIFORCE_TARGET_GRAPH", "0")
    g, ge = _engine(large, route != "eager", PEN)
    assert bool(ge.target_graphs) == (route in ("graphs", "tiny-v128k"))
    n = 24 if large else 48
    run = _stream(g, ge, PEN, n)
    assert (run._device_sets() is not None) == bool(ge.target_graphs)
    _check_state(ge, g, run.emitted)
    # the same engine under a runner WITHOUT penalties: not served, the eager route, the unpenalised stream
    off = _runner(g, ge, (1.0, 0.0, 0.0))
    assert off._served() is False
    off.prefill(Hh.prompt_of(g).to(DEV))
    while off.n < n:
        off.step()
    _check_penalised_stream(g, run, list(off.emitted), route)
    if route == "graphs":
        from triforce_amd.utils.decoding import Autoregressive
        from triforce_amd.utils.sampling import UniformSource
        _, ids = Autoregressive(Hh.FakeTokenizer(), ge, Hh.prompt_of(g).to(DEV), max_len=24, top_p=1.0, temperature=1.0, min_p=1.0,
                                rng=UniformSource(DEV, values=Hh.fixed_uniforms(seed=5)), return_tokens=True, **PEN_KW)
        gaps = PR.teacher_forced_penalised_gaps(g, ids, PEN, Hh.build_oracle, Hh.prompt_of(g))
        assert max(gaps) <= GAP_TOL * PEN[0], f"Autoregressive: token {gaps.index(max(gaps))} trails by {max(gaps):.4f}"
        _check_state(ge, g, ids)


def test_accepted_drafts_count_inside_the_block_on_device():
    """Aligned weights (the random ones never accept a draft at temperature 1): rows i > 0 of the captured verify — whose counts
    include the drafted ids[1 .. i] — decide tokens and several ids are committed per step, on the device-side step set-up;
    the stream is the Autoregressive one under the same penalties (both are the penalised argmax walk of one model)."""
    run, ge, counts, ar = PR.aligned_streams(DEV, True, PEN)
    assert run._device_sets() is not None and run._served()
    assert run.accepted_count >= 10 and max(run.counts) >= 2, (run.accepted_count, run.counts)
    hist = torch.bincount(torch.tensor(run.emitted[:-1]), minlength=ge.penalty_state.V)
    assert torch.equal(counts.cpu().long(), hist)
    Hh.note(f"penalties {PEN} aligned weights: {len(run.emitted)} tokens, {run.accepted_count} drafts accepted, counts "
            f"{run.counts[:12]}, common prefix with Autoregressive {Hh.common_prefix(ar, run.emitted)}")
    assert ar == run.emitted, f"the streams part at token {Hh.common_prefix(ar, run.emitted)} of {len(ar)}"


def test_logprobs_with_penalties_score_the_raw_logits():
    g, ge = _engine(False, True, PEN)
    run = _stream(g, ge, PEN, 40, logprobs=True)
    st = run.stats(1.0)
    stream = list(run.emitted)
    want, bounds = LR.teacher_forced_reference(g, Hh.prompt_of(g), stream)
    LR.check(st["logprobs"], want, bounds, "logprobs under penalties (raw logits)")
    _check_state(ge, g, stream)
