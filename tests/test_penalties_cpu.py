"""Repetition / frequency / presence penalties on the target tier, the parts that need no GPU: the C ABI
and every argument gate of tf_penalize_logits / tf_penalty_commit, the Penalties value, the torch route of ``penalize``
against tests/penalty_ref.py, the routing through GraphInferenceEngine and the runner, the decode loops on the CPU backend
(cpu_ops) and the command line.  The kernels are checked in tests/test_gpu_penalties.py."""
import ctypes
import os
import re
import types

import pytest
import torch

from tests import helpers as Hh
from tests import penalty_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP_TOL = 8e-3        # as tests/test_topk_cpu.py: an emitted token may trail the target's argmax by ~2 fp16 spacings
EINVAL = -22
PEN = (1.3, 0.2, 0.1)
PEN_KW = dict(repetition_penalty=PEN[0], frequency_penalty=PEN[1], presence_penalty=PEN[2])


def test_entry_points_are_declared_bound_exported_and_gate_every_argument_before_launching():
    from triforce_amd import build, hip, ops
    src = open(os.path.join(ROOT, "include", "triforce_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = hip.lib()
    for name in ("tf_penalize_logits", "tf_penalty_commit"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", decl), f"include/triforce_hip.h does not declare {name}"
        assert name in hip.SIGNATURES
        assert hasattr(lib, name), f"libtriforce_hip.so does not export {name}"
    assert len(hip.SIGNATURES["tf_penalize_logits"][1]) == 13 and len(hip.SIGNATURES["tf_penalty_commit"][1]) == 5
    assert "penalties.hip" in build.SOURCES
    assert callable(ops.penalize_logits) and callable(ops.penalty_commit)

    # no device is touched below: host buffers stand in for device pointers, every call must return before any launch
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15)
    null = ctypes.c_void_p(0)

    def pen(lg=p, ls=8, out=p, os_=8, ids=p, gc=p, ps=p, rows=1, V=8, r=1.3, f=0.2, pr=0.1):
        return lib.tf_penalize_logits(lg, ls, out, os_, ids, gc, ps, rows, V, r, f, pr, null)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(lg=null), dict(out=null), dict(gc=null), dict(ps=null), dict(rows=0), dict(rows=-1), dict(rows=65),
               dict(V=0), dict(V=-3), dict(ls=7), dict(os_=7), dict(ls=0), dict(os_=-8), dict(r=0.0), dict(r=-1.0), dict(r=nan),
               dict(r=inf), dict(f=nan), dict(f=inf), dict(f=-inf), dict(pr=nan), dict(pr=inf), dict(pr=-inf)):
        assert pen(**kw) == EINVAL, kw
        assert pen(**dict(kw, ids=null)) == EINVAL, kw                 # (NULL ids alone is legal: every other gate still holds)
    assert pen(lg=null, out=null, ids=null, gc=null, ps=null) == EINVAL

    def commit(gc=p, ids=p, n=1, V=8):
        return lib.tf_penalty_commit(gc, ids, n, V, null)

    for kw in (dict(gc=null), dict(ids=null), dict(n=-1), dict(n=65), dict(V=0), dict(gc=null, n=0), dict(ids=null, n=0),
               dict(gc=null, ids=null, n=0)):
        assert commit(**kw) == EINVAL, kw
    assert commit(n=0) == 0                                            # the documented no-op: nothing is launched


def test_ops_refuse_cpu_tensors():
    from triforce_amd import hip, ops
    from triforce_amd.utils.sampling import Penalties
    st = ops.PenaltyState(16, "cpu")
    with pytest.raises(hip.TriforceHipError):
        ops.penalize_logits(torch.zeros(2, 16), torch.zeros(2, dtype=torch.long), st, Penalties(1.3))
    with pytest.raises(hip.TriforceHipError):
        ops.penalty_commit(st, torch.zeros(2, dtype=torch.long), 1)


def test_penalties_validate_compare_and_hash():
    from triforce_amd.utils.sampling import Penalties
    off = Penalties()
    assert (off.repetition, off.frequency, off.presence) == (1.0, 0.0, 0.0) and not off.on
    assert Penalties(1, 0, 0) == off and hash(Penalties(1, 0, 0)) == hash(off) and len({off, Penalties(1.0, 0.0, -0.0)}) == 1
    for kw in (dict(repetition=1.3), dict(frequency=0.2), dict(presence=0.1), dict(frequency=-0.5), dict(presence=-1.0),
               dict(repetition=0.8)):
        assert Penalties(**kw).on and Penalties(**kw) != off, kw
    assert Penalties(1.3, 0.2, 0.1) == Penalties(1.3, 0.2, 0.1) != Penalties(1.3, 0.2, 0.0)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(repetition=0.0), dict(repetition=-1.0), dict(repetition=nan), dict(repetition=inf), dict(frequency=nan),
               dict(frequency=inf), dict(frequency=-inf), dict(presence=nan), dict(presence=inf), dict(repetition=None),
               dict(frequency="1")):
        with pytest.raises(ValueError):
            Penalties(**kw)
    with pytest.raises(Exception):
        off.repetition = 2.0                                           # frozen


def _case(V, rows, seed):
    """Logits with every planted case of the contract, a state and a block of ids -> (logits, ids, state)."""
    from triforce_amd import ops
    gen = torch.Generator().manual_seed(seed)
    lg = torch.randn(rows, V, generator=gen) * 3.0
    st = ops.PenaltyState(V, "cpu")
    st.reset(torch.tensor([[1, 5, 5, 9, V - 1]]))                      # prompt-seen only: 1, 9; 5 twice in the prompt
    st.gen_count[3] = 2                                                # generated before, not in the prompt
    st.gen_count[5] = 1                                                # both
    st.gen_count[V - 2] = 7
    ids = torch.randint(0, V, (rows,), generator=gen)
    ids[0] = 11
    if rows > 2:
        ids[2] = 11                                                    # a token twice in the block
    if rows > 3:
        ids[3] = 9                                                     # a prompt-seen token drafted
    lg[:, 1] = 0.0
    lg[:, 9] = -0.0
    lg[:, 3] = float("-inf")
    lg[0, 11] = 2.5
    lg[-1, 5] = -1.25
    return lg, ids, st


@pytest.mark.parametrize("pen", [(1.3, 0.2, 0.1), (0.7, 0.0, 0.0), (1.0, -0.3, 0.0), (1.0, 0.0, 1e4), (1.1, 0.25, -0.5)])
def test_penalize_torch_route_equals_the_reference_bit_for_bit(pen):
    from triforce_amd.utils.sampling import Penalties, penalize
    for V, rows in [(37, 1), (64, 7), (101, 18)]:
        lg, ids, st = _case(V, rows, 3 + rows)
        raw = lg.clone()
        for block in (ids, None):
            got = penalize(lg, block, st, Penalties(*pen))
            want = PR.penalize(lg, block, st.gen_count, st.prompt_seen, *pen)
            assert got.dtype == torch.float32 and got.shape == lg.shape
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (V, rows, pen, block is None)
            assert torch.equal(lg.view(torch.int32), raw.view(torch.int32))        # out of place
            c = PR.counts(st.gen_count, block, rows, V)
            untouched = (st.prompt_seen == 0).unsqueeze(0) & (c == 0)
            assert torch.equal(got.view(torch.int32)[untouched], raw.view(torch.int32)[untouched])
            assert bool((got[:, 3] == float("-inf")).all())
        if rows > 2:                                                   # row i never sees ids[j > i]: 11 is counted once, then twice
            c = PR.counts(st.gen_count, ids, rows, V)
            assert int(c[0, 11]) == 1 and int(c[1, 11]) == 1 and int(c[2, 11]) == 2
            later = int(ids[-1])
            if later not in ids[:-1].tolist() and st.gen_count[later] == 0 and st.prompt_seen[later] == 0:
                got = penalize(lg, ids, st, Penalties(*pen))
                assert torch.equal(got[:-1, later].view(torch.int32), raw[:-1, later].view(torch.int32))


def test_the_penalty_map_is_piecewise_linear_with_slopes_one_over_r_one_and_r():
    """What the end-to-end tolerance rests on: for a fixed state the map x -> y is continuous and its slopes lie in
    {1 / r, 1, r}, so two logits that differ by d map to values that differ by at most max(r, 1 / r) * d."""
    r = 1.3
    x = torch.linspace(-4.0, 4.0, 4001, dtype=torch.float64)
    d = 1e-3
    for seen, c in [(0, 0), (1, 0), (0, 2)]:
        def f(v):
            return PR.penalize(v.float().reshape(1, -1), None, torch.full((v.numel(),), c, dtype=torch.int32),
                               torch.full((v.numel(),), seen, dtype=torch.uint8), r, 0.2, 0.1)[0].double()
        slope = (f(x + d) - f(x)) / d
        lo, hi = (1.0, 1.0) if (not seen and c == 0) else (1 / r, r)
        assert float(slope.min()) >= lo - 1e-3 and float(slope.max()) <= hi + 1e-3
        away = x.abs() > 2 * d                                          # (a step across 0 mixes the two slopes)
        s = slope[away]
        near = lambda k: (s - k).abs() < 1e-3                           # noqa: E731
        assert bool((near(1 / r) | near(1.0) | near(r)).all())


def _cpu_engine(g, penalties=(1.0, 0.0, 0.0), min_p=1.0):
    return PR.build_engine(g, "cpu", graphs=False, penalties=penalties, min_p=min_p)


def _run(ge, g, seed=41, **kw):
    from triforce_amd.utils.decoding import TriForce
    from triforce_amd.utils.sampling import UniformSource
    return TriForce(Hh.FakeTokenizer(), ge, Hh.prompt_of(g), gamma=g["gamma"], max_len=g["gen_len"], top_p=1.0, temperature=1.0,
                    min_p=1.0, rng=UniformSource("cpu", values=Hh.fixed_uniforms(seed=seed)), return_details=True, **kw)


def test_defaults_call_no_penalty_function_and_allocate_nothing(cpu_ops, monkeypatch):
    from triforce_amd import ops
    from triforce_amd.utils import sampling
    g = Hh.load_golden("small_gamma6")
    ge, _, _ = _cpu_engine(g)
    assert ge.penalty_state is None and not ge.target_penalties.on
    plain = _run(ge, g)["tokens"]
    calls = []
    for mod, name in ((ops, "penalize_logits"), (ops, "penalty_commit"), (sampling, "penalize"), (sampling, "commit_penalties")):
        monkeypatch.setattr(mod, name, lambda *a, _n=name, **k: calls.append(_n))
    monkeypatch.setattr(ops, "PenaltyState", lambda *a, **k: calls.append("PenaltyState"))
    ge.initialize_eager(g["gamma"], probs=True, temperature=1.0, top_p=1.0, min_p=1.0, repetition_penalty=1.0,
                        frequency_penalty=0.0, presence_penalty=0.0)
    again = _run(ge, g, repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)["tokens"]
    assert calls == [] and ge.penalty_state is None
    assert again == plain


def test_serves_rule_over_runner_and_engine_penalties(cpu_ops):
    from triforce_amd.utils.decoding import Autoregressive, TriForceRunner
    from triforce_amd.utils.sampling import Filters, Penalties
    g = Hh.load_golden("small_gamma6")
    gamma = g["gamma"]
    ge, _, _ = _cpu_engine(g)
    f = Filters(1.0, 1.0, -1, 1.0)
    off = (1.0, 0.0, 0.0)
    for runner_p, engine_p, match in [(PEN, PEN, True), (off, PEN, False), (PEN, (1.3, 0.2, 0.0), False), (off, off, True),
                                      ((1.0, 0.0, 0.5), (1.0, 0.0, 0.5), True), ((1.1, 0.0, 0.0), (1.2, 0.0, 0.0), False)]:
        ge.initialize_eager(gamma, probs=True, temperature=1.0, top_p=1.0, min_p=1.0, repetition_penalty=engine_p[0],
                            frequency_penalty=engine_p[1], presence_penalty=engine_p[2])
        assert ge.target_penalties == Penalties(*engine_p) and (ge.penalty_state is not None) == Penalties(*engine_p).on
        assert not any("penalt" in k for k in ge.sampling)            # the draft tiers' capture arguments never see them
        run = TriForceRunner(Hh.FakeTokenizer(), ge, gamma, top_p=1.0, temperature=1.0, min_p=1.0, repetition_penalty=runner_p[0],
                             frequency_penalty=runner_p[1], presence_penalty=runner_p[2])
        assert run._served() is match, (runner_p, engine_p)
        assert ge.serves(f, Penalties(*runner_p)) is match
        assert ge.serves(f) is (not Penalties(*engine_p).on)          # callers that pass no penalties mean "off"
        assert ge.serves(f, None) is (not Penalties(*engine_p).on)
        assert ge.serves(Filters(1.0, 1.0, -1, 0.5), Penalties(*runner_p)) is False
    # a runner that asks for penalties over an engine initialised without them: refused before anything runs
    ge.initialize_eager(gamma, probs=True, temperature=1.0, top_p=1.0, min_p=1.0)
    with pytest.raises(NotImplementedError, match="penalt"):
        TriForceRunner(Hh.FakeTokenizer(), ge, gamma, top_p=1.0, temperature=1.0, min_p=1.0, **PEN_KW)
    with pytest.raises(NotImplementedError, match="penalt"):
        Autoregressive(Hh.FakeTokenizer(), ge, Hh.prompt_of(g), max_len=2, top_p=1.0, temperature=1.0, **PEN_KW)
    with pytest.raises(ValueError):
        TriForceRunner(Hh.FakeTokenizer(), ge, gamma, repetition_penalty=0.0)
    with pytest.raises(ValueError):
        ge.initialize_eager(gamma, frequency_penalty=float("nan"))

    # an engine without ``serves`` (stubs) captured without penalties
    class Bare:
        engine = ge.engine
        sampling = ge.sampling
    ge.initialize_eager(gamma, probs=True, temperature=1.0, top_p=1.0, **PEN_KW)
    run = TriForceRunner(Hh.FakeTokenizer(), ge, gamma, top_p=1.0, temperature=1.0, **PEN_KW)
    run.ge = Bare()
    assert run._served() is False
    run.penalties = Penalties()
    assert run._served() is True


def test_dist_engine_refuses_penalties_before_anything_is_captured():
    from triforce_amd.utils.decoding import TriForceRunner, _DistEngine

    class Llm:
        temperature, top_p, device, draft = 0.6, 0.9, "cpu", None
        config = types.SimpleNamespace(model_config=types.SimpleNamespace(vocab_size=64))
        kv_cache = retrieval_cache = draft_cache = None

        def __getattr__(self, name):
            raise AssertionError(f"the llm was touched: {name}")
    ge = _DistEngine(Llm())
    for kw in (dict(repetition_penalty=1.2), dict(frequency_penalty=0.1), dict(presence_penalty=-0.1)):
        with pytest.raises(NotImplementedError, match="penalt"):
            TriForceRunner(Hh.FakeTokenizer(), ge, 4, **kw)


def test_only_on_chip_takes_the_penalty_flags():
    from triforce_amd.utils import cli
    flags = ("--repetition_penalty", "--frequency_penalty", "--presence_penalty")
    for flag in flags:
        assert any(row[0] == flag for row in cli.SCRIPT_OWN["on_chip"]), flag
        for script, rows in cli.SCRIPTS.items():
            assert all(row[0] != flag for row in rows), (script, flag)
        for script in ("offloading", "offloading_TP", "offloading_seqouia"):
            with pytest.raises(SystemExit):
                cli.parse(script, [flag, "1.1"])
        assert flag in open(os.path.join(ROOT, "README.md")).read()
    a = cli.parse("on_chip", [])
    assert (a.repetition_penalty, a.frequency_penalty, a.presence_penalty) == (1.0, 0.0, 0.0)
    a = cli.parse("on_chip", ["--repetition_penalty", "1.1", "--frequency_penalty", "0.2", "--presence_penalty", "-0.1"])
    assert (a.repetition_penalty, a.frequency_penalty, a.presence_penalty) == (1.1, 0.2, -0.1)
    src = open(os.path.join(ROOT, "test", "on_chip.py")).read()
    for flag in flags:
        assert "args." + flag[2:] in src


@pytest.fixture(scope="module")
def golden():
    return Hh.load_golden("small_gamma6")


def test_presence_penalty_makes_every_emitted_token_distinct(cpu_ops, golden):
    """(a) temperature 1, top-p 1, min_p = 1: the target's distribution is the row maximum of the PENALISED logits while the
    drafts keep sampling unpenalised.  presence = 1e4 sinks every token of the answer so far, so no token is emitted twice; a
    prompt token stays free to appear (once): presence acts on the output only."""
    g = golden
    ge, _, _ = _cpu_engine(g, (1.0, 0.0, 1e4))
    res = _run(ge, g, presence_penalty=1e4)
    toks = res["tokens"]
    assert len(toks) > g["gamma"] and len(set(toks)) == len(toks), f"a token was emitted twice: {toks}"
    assert res["resampled"] > 0                                       # the drafts did propose something else, and it was corrected
    hist = torch.bincount(torch.tensor(toks[:-1]), minlength=ge.penalty_state.V)
    assert torch.equal(ge.penalty_state.gen_count.long(), hist)      # everything emitted but the pending token
    seen = torch.zeros(ge.penalty_state.V, dtype=torch.uint8)
    seen[Hh.prompt_of(g).reshape(-1)] = 1
    assert torch.equal(ge.penalty_state.prompt_seen, seen)


def test_penalised_stream_is_the_penalised_argmax_of_the_oracle(cpu_ops, golden):
    """(b), (c), (d): with (1.3, 0.2, 0.1) every emitted token's penalised oracle logit is within GAP_TOL * 1.3 of the best
    (the penalty map's slopes are at most r = 1.3), the stream differs from the unpenalised one, and Autoregressive passes
    the same check."""
    from triforce_amd.utils.decoding import Autoregressive
    from triforce_amd.utils.sampling import UniformSource
    g = golden
    plain = _run(_cpu_engine(g)[0], g)["tokens"]
    ge, _, _ = _cpu_engine(g, PEN)
    res = _run(ge, g, **PEN_KW)
    gaps = PR.teacher_forced_penalised_gaps(g, res["tokens"], PEN, Hh.build_oracle, Hh.prompt_of(g))
    print(f"TriForce: penalised teacher-forced gaps max {max(gaps):.5f}, {sum(1 for x in gaps if x > 0)} of {len(gaps)} not "
          f"the argmax; acceptance {res['acceptance_rate']:.3f}, resampled {res['resampled']}")
    assert max(gaps) <= GAP_TOL * PEN[0], f"token {gaps.index(max(gaps))} trails the penalised argmax by {max(gaps):.4f}"
    assert res["tokens"] != plain
    raw_gaps = Hh.teacher_forced_gaps(g, res["tokens"])
    assert max(raw_gaps) > GAP_TOL                                    # (and it is NOT the unpenalised greedy stream)
    _, ids = Autoregressive(Hh.FakeTokenizer(), ge, Hh.prompt_of(g), max_len=g["gen_len"], top_p=1.0, temperature=1.0, min_p=1.0,
                            rng=UniformSource("cpu", values=Hh.fixed_uniforms(seed=5)), return_tokens=True, **PEN_KW)
    gaps = PR.teacher_forced_penalised_gaps(g, ids, PEN, Hh.build_oracle, Hh.prompt_of(g))
    print(f"Autoregressive: penalised teacher-forced gaps max {max(gaps):.5f}")
    assert max(gaps) <= GAP_TOL * PEN[0]
    hist = torch.bincount(torch.tensor(ids[:-1]), minlength=ge.penalty_state.V)
    assert torch.equal(ge.penalty_state.gen_count.long(), hist)


def test_accepted_drafts_count_inside_the_block_and_the_stream_is_the_autoregressive_one(cpu_ops):
    """Random weights never accept a draft at temperature 1; aligned weights do, so rows i > 0 of a verify block — whose counts
    include the drafted ids[1 .. i] — decide tokens, and several ids are committed per step."""
    run, ge, counts, ar = PR.aligned_streams("cpu", False, PEN)
    assert run.accepted_count >= 10 and max(run.counts) >= 2, (run.accepted_count, run.counts)
    hist = torch.bincount(torch.tensor(run.emitted[:-1]), minlength=ge.penalty_state.V)
    assert torch.equal(counts.long(), hist)
    assert ar == run.emitted, f"the streams part at token {Hh.common_prefix(ar, run.emitted)} of {len(ar)}"


def test_extend_resets_the_state_to_the_new_history(cpu_ops, golden):
    """(e) after extend() the counts are zero and prompt_seen is the set of the whole new history — kept rows, the pending
    token of a chat turn, the new input."""
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.sampling import UniformSource
    g = golden
    ge, _, _ = _cpu_engine(g, PEN)
    run = TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], top_p=1.0, temperature=1.0, min_p=1.0,
                         rng=UniformSource("cpu", values=Hh.fixed_uniforms(seed=41)), **PEN_KW)
    run.prefill(Hh.prompt_of(g))
    for _ in range(2):
        run.step()
    st = ge.penalty_state
    assert int(st.gen_count.sum()) == len(run.emitted) - 1 > 0
    pending = run.next_token
    question = torch.tensor([[7, 8, 9, 7]])
    run.extend(question, keep=None)
    hist = run.history.reshape(-1)
    assert int(st.gen_count.sum()) == 0
    seen = torch.zeros(st.V, dtype=torch.uint8)
    seen[hist] = 1
    assert torch.equal(st.prompt_seen, seen)
    assert pending in hist.tolist() and all(t in hist.tolist() for t in (7, 8, 9))
    assert len(run.emitted) == 1
    run.step()                                                        # and the next answer counts from zero
    assert int(st.gen_count.sum()) == len(run.emitted) - 1
