"""Top-N alternatives and token ranks on the device: tf_token_top_logprobs against the definition (exact)
and against tf_token_logprobs (bit for bit), its argument gates, and ``top_logprobs=5`` end to end against the CPU oracle."""
import ctypes

import pytest
import torch

from tests import helpers as Hh
from tests import logprobs_ref as LR
from tests.test_gpu_logprobs import _bound, _device_view, small_blocks  # noqa: F401  (small_blocks: a fixture)
from tests.test_logprobs_cpu import SAMPLED, NoEosTokenizer
from tests.test_top_logprobs_cpu import KINDS, definition, rows_of_every_kind

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GREEDY = dict(top_k=-1, top_p=1e-9, temperature=1.0)


@pytest.mark.parametrize("N", [1, 5, 20])
@pytest.mark.parametrize("V", [1, 19, 20, 21, 64, 1000, 4097, 32000, 128256])
@pytest.mark.parametrize("rows", [1, 7, 32])
def test_kernel_matches_the_definition(rows, V, N):
    """ids and ranks equal the definition's; every value equals tf_token_logprobs' for that row and id bit for bit and lies
    within test_gpu_logprobs._bound of the float64 log_softmax; ``out`` equals tf_token_logprobs'.  A row of -inf alone (the
    -inf kind at N = 1) is outside tf_token_logprobs' contract (it gives NaN): there the ids and ranks are checked and the
    values must be -inf."""
    from triforce_amd import ops
    gen = torch.Generator().manual_seed(100000 * N + 1000 * rows + V)
    for shift in range(KINDS if rows < KINDS else 1):
        x, t = rows_of_every_kind(rows, V, N, shift, gen)
        ids, vals, rank = definition(x, t, N)
        ref = ops.token_top_logprobs_ref(x, t, N)
        assert torch.equal(ref[0], ids) and torch.equal(ref[2], rank)
        live = torch.isfinite(x.max(dim=1).values)                   # rows inside tf_token_logprobs' contract
        bound = _bound(x)[:, None].expand(-1, N)
        for layout in ("contiguous", "strided", "offset"):
            xd, what = _device_view(x, layout), f"{rows}x{V} N={N} {layout} shift {shift}"
            single = ops.token_logprobs(xd, t.to(DEV)).cpu()
            for targets in (t.to(DEV), t.tolist()):
                out = torch.full((rows,), 7.0, device=DEV)
                got_ids, got_lp, got_rank = (a.cpu() for a in ops.token_top_logprobs(xd, targets, N, out=out))
                assert torch.equal(got_ids, ids), f"{what}: ids of row {int((got_ids != ids).any(dim=1).nonzero()[0])}"
                assert torch.equal(got_rank, rank), f"{what}: ranks {got_rank.tolist()} != {rank.tolist()}"
                assert torch.equal(out.cpu()[live], single[live]), f"{what}: out"
                for r in range(rows):                                # rank <= N  <=>  the target sits at place rank - 1
                    k = int(rank[r])                                 # (0: no target)
                    assert k == 0 or ((k <= N) == (int(t[r]) in got_ids[r].tolist()) and (k > N or got_ids[r, k - 1] == t[r]))
            inf = torch.isinf(vals)
            assert torch.equal(got_lp.double()[inf], vals[inf]), f"{what}: -inf values and pads"
            used = (got_lp.double() - vals).abs()[~inf] / bound[~inf]
            assert used.numel() == 0 or float(used.max()) <= 1.0, f"{what}: {float(used.max()):.2f} of the bound"
            for j in range(min(N, V)):                               # bit for bit the single-value kernel's value
                one = ops.token_logprobs(xd, ids[:, j].long().to(DEV)).cpu()
                assert torch.equal(got_lp[live, j], one[live]), f"{what}: place {j} differs from tf_token_logprobs"
            assert ops.token_top_logprobs(xd, None, N)[2] is None and torch.equal(ops.token_top_logprobs(xd, None, N)[0].cpu(), ids)
    torch.cuda.synchronize()


def test_entry_points_reject_bad_arguments_and_write_nothing():
    from triforce_amd import hip
    lib = hip.lib()
    x, t = torch.zeros(2, 8, device=DEV), torch.zeros(2, dtype=torch.long, device=DEV)
    outs = [torch.full((2, 5), 9, dtype=torch.int32, device=DEV), torch.full((2, 5), 9.0, device=DEV),
            torch.full((2,), 9, dtype=torch.int32, device=DEV), torch.full((2,), 9.0, device=DEV)]
    host = (ctypes.c_int64 * 32)()
    p, tt, null = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(0)
    i, v, k, o = (ctypes.c_void_p(b.data_ptr()) for b in outs)
    f, g = lib.tf_token_top_logprobs, lib.tf_token_top_logprobs_ids
    for args in ((null, 8, tt, 2, 8, 5, i, v, k, o), (p, 8, tt, 2, 8, 5, null, v, k, o), (p, 8, tt, 2, 8, 5, i, null, k, o),
                 (p, 8, tt, 2, 8, 5, i, v, null, o), (p, 8, null, 2, 8, 5, i, v, k, null), (p, 8, null, 2, 8, 5, i, v, null, o),
                 (p, 8, tt, 2, 8, 0, i, v, k, o), (p, 8, tt, 2, 8, 21, i, v, k, o), (p, 8, tt, 2, 0, 5, i, v, k, o),
                 (p, 7, tt, 2, 8, 5, i, v, k, o), (p, 8, tt, 0, 8, 5, i, v, k, o)):
        assert f(*args, null) == -22, args
    for args in ((null, 8, host, 2, 8, 5, i, v, k, o), (p, 8, null, 2, 8, 5, i, v, k, o), (p, 8, host, 2, 8, 5, null, v, k, o),
                 (p, 8, host, 2, 8, 5, i, null, k, o), (p, 8, host, 2, 8, 5, i, v, null, o), (p, 8, host, 2, 8, 0, i, v, k, o),
                 (p, 8, host, 2, 8, 21, i, v, k, o), (p, 8, host, 2, 0, 5, i, v, k, o), (p, 7, host, 2, 8, 5, i, v, k, o),
                 (p, 8, host, 0, 8, 5, i, v, k, o), (p, 8, host, 33, 8, 5, i, v, k, o)):
        assert g(*args, null) == -22, args
    torch.cuda.synchronize()
    assert all(bool((b == 9).all()) for b in outs)                    # nothing was launched or written


# ---- end to end on small_gamma6 --------------------------------------------------------------------------------------------
def _oracle_rows(g, context, stream):
    """The oracle's float64 log_softmax rows that score ``stream`` behind ``context``, walked as
    logprobs_ref.teacher_forced_reference walks them (whose per-row bounds are used beside these)."""
    eng, _, _ = Hh.build_oracle(g)
    eng.kv_cache.reset()
    rows = [eng.inference(context)[0, -1]]
    for tok in stream[:-1]:
        rows.append(eng.model.forward(torch.tensor([[tok]]), eng.kv_cache, None)[0, -1])
    return torch.log_softmax(torch.stack(rows).double(), dim=-1)


def _check_stream(g, context, tokens, logprobs, top, ranks, what):
    V = g["tcfg"]["vocab_size"]
    assert len(top) == len(ranks) == len(tokens) == len(logprobs)
    want, bounds = LR.teacher_forced_reference(g, context, tokens)
    rows = _oracle_rows(g, context, tokens)
    for n, (tok, lp, pairs, rank) in enumerate(zip(tokens, logprobs, top, ranks)):
        ids, vals = [i for i, _ in pairs], [v for _, v in pairs]
        assert len(pairs) == 5 and len(set(ids)) == 5 and all(0 <= i < V for i in ids), f"{what}: token {n} ids {ids}"
        assert all(a >= b for a, b in zip(vals, vals[1:])), f"{what}: token {n} values increase"
        assert rank >= 1 and (rank <= 5) == (tok in ids) and (rank > 5 or pairs[rank - 1] == (tok, lp)), f"{what}: token {n}"
        b = float(bounds[n])
        assert all(abs(v - float(rows[n, i])) <= b for i, v in pairs), f"{what}: token {n} values off the oracle's"
        assert float(rows[n].topk(5).values[4]) <= vals[4] + b, f"{what}: token {n}: the oracle's 5th is above the 5th listed"
    assert float((torch.tensor(logprobs, dtype=torch.float64) - want).abs().div(bounds).max()) < 1.0


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_triforce_top_logprobs(small_blocks, mode, graphs):  # noqa: F811
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.sampling import UniformSource
    g, sampling = Hh.load_golden("small_gamma6"), GREEDY if mode == "greedy" else SAMPLED
    prompt, stats = Hh.prompt_of(g), []
    for top in (0, 5):
        ge = Hh.build_product(g, DEV, temperature=sampling["temperature"], top_p=sampling["top_p"], graphs=graphs)
        run = TriForceRunner(NoEosTokenizer(), ge, g["gamma"], rng=UniformSource(DEV, values=Hh.fixed_uniforms()),
                             logprobs=True, top_logprobs=top, **sampling)
        run.prefill(prompt.to(DEV))
        while run.n < 32:
            run.step()
        stats.append(run.stats(1.0))
    off, on = stats
    assert "top_logprobs" not in off and "ranks" not in off
    assert on["tokens"] == off["tokens"] and on["logprobs"] == off["logprobs"]
    _check_stream(g, prompt, on["tokens"], on["logprobs"], on["top_logprobs"], on["ranks"], f"TriForce {mode} graphs={graphs}")


def test_autoregressive_and_session_followup(small_blocks):  # noqa: F811
    from triforce_amd.utils.decoding import Autoregressive, TriForceSession
    from triforce_amd.utils.sampling import UniformSource
    g = dict(Hh.load_golden("small_gamma6"), gen_len=120, budget=320)
    doc = Hh.prompt_of(g)
    rng = lambda: UniformSource(DEV, values=Hh.fixed_uniforms())        # noqa: E731
    ge = Hh.build_product(g, DEV, temperature=SAMPLED["temperature"], top_p=SAMPLED["top_p"], graphs=True)
    base = Autoregressive(NoEosTokenizer(), ge, doc.to(DEV), max_len=16, rng=rng(), logprobs=True, **SAMPLED)
    out = Autoregressive(NoEosTokenizer(), ge, doc.to(DEV), max_len=16, rng=rng(), top_logprobs=5, **SAMPLED)
    assert len(out) == 5 and out[1] == base[1] and out[2] == base[2]
    _check_stream(g, doc, out[1], out[2], out[3], out[4], "Autoregressive")
    ge = Hh.build_product(g, DEV, temperature=SAMPLED["temperature"], top_p=SAMPLED["top_p"], graphs=True)   # (a fresh engine)
    s = TriForceSession(NoEosTokenizer(), ge, g["gamma"], rng=rng(), top_logprobs=5, **SAMPLED)
    s.prefill(doc.to(DEV))
    s.generate(12)
    q = torch.randint(3, g["tcfg"]["vocab_size"], (1, 9), generator=torch.Generator().manual_seed(5))
    st = s.ask(q.to(DEV), 16)
    context = torch.cat([doc[:, :s.document], q], dim=1)
    _check_stream(g, context, st["tokens"], st["logprobs"], st["top_logprobs"], st["ranks"], "session follow-up")
