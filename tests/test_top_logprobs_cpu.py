"""Top-N alternatives and token ranks without a device: ops.token_top_logprobs_ref against a float64
restatement, the ``top_logprobs`` keyword's range check and refusals, and the decode loop's bookkeeping over that restatement."""
import types

import pytest
import torch

from tests import helpers as Hh
from tests.test_logprobs_cpu import SAMPLED, NoEosTokenizer, lp_ops, token_logprobs_cpu  # noqa: F401  (lp_ops: a fixture)

KINDS = 7


def rows_of_every_kind(rows, V, N, shift, gen):
    """(fp32 logits, targets): row r is of kind (r + shift) % 7 — N(0, 1); N(0, 30); all equal; one entry at +80; multiples of
    0.5 (ties everywhere); a plateau of 2N equal maxima at ids that cross 4-, 64- and 256-entry boundaries, one at V - 1;
    -inf everywhere except min(V, N - 1) entries.  Targets cycle through 0, V - 1, -1, V, random, one inside the plateau."""
    x = torch.randn(rows, V, generator=gen)
    t = torch.randint(0, V, (rows,), generator=gen)
    for r in range(rows):
        kind = (r + shift) % KINDS
        plateau = torch.unique(torch.tensor([V - 1] + [(p + 61 * r) % V for p in (3, 4, 63, 64, 255, 256, 257)]
                                            + [(67 * j + r) % V for j in range(2 * N)]))[-2 * N:]
        if kind == 1:
            x[r] *= 30.0
        elif kind == 2:
            x[r] = 0.37
        elif kind == 3:
            x[r, (7 * r + 3) % V] = 80.0
        elif kind == 4:
            x[r] = torch.round(2.0 * x[r]) / 2.0
        elif kind == 5:
            x[r, plateau] = 9.25
        elif kind == 6:
            keep = torch.randperm(V, generator=gen)[:min(V, N - 1)]
            vals = x[r, keep].clone()
            x[r] = -float("inf")
            x[r, keep] = vals
        t[r] = (0, V - 1, -1, V, int(t[r]), int(plateau[len(plateau) // 2]))[(r + shift) % 6]
    return x, t


def definition(x, t, N):
    """The contract on fp32 inputs: stable descending sort, the counting formula; values from a float64 log_softmax."""
    rows, V = x.shape
    k = min(N, V)
    ids = torch.full((rows, N), -1, dtype=torch.int32)
    ids[:, :k] = torch.sort(x, dim=1, descending=True, stable=True).indices[:, :k].to(torch.int32)
    ls = torch.log_softmax(x.double(), dim=1)
    vals = torch.full((rows, N), -float("inf"), dtype=torch.float64)
    vals[:, :k] = ls.gather(1, ids[:, :k].long())
    vals[torch.isinf(x.gather(1, ids.clamp(min=0).long())) | (ids < 0)] = -float("inf")        # (a row of -inf alone: not NaN)
    rank = torch.zeros(rows, dtype=torch.int32)
    for r in range(rows):
        if 0 <= int(t[r]) < V:
            xt = x[r, t[r]]
            rank[r] = 1 + int((x[r] > xt).sum()) + int((x[r, :t[r]] == xt).sum())
    return ids, vals, rank


@pytest.mark.parametrize("V", [1, 19, 20, 21, 64, 1000])
@pytest.mark.parametrize("N", [1, 5, 20])
def test_ref_matches_the_definition(V, N):
    from tests.test_gpu_logprobs import _bound
    from triforce_amd import ops
    gen = torch.Generator().manual_seed(100 * V + N)
    x, t = rows_of_every_kind(2 * KINDS, V, N, 0, gen)
    ids, vals, rank = definition(x, t, N)
    got_ids, got_lp, got_rank = ops.token_top_logprobs_ref(x, t, N)
    assert torch.equal(got_ids, ids) and torch.equal(got_rank, rank)
    inf = torch.isinf(vals)
    assert torch.equal(got_lp.double()[inf], vals[inf])
    assert bool(((got_lp.double() - vals).abs()[~inf] <= _bound(x)[:, None].expand(-1, N)[~inf]).all())
    assert ops.token_top_logprobs_ref(x, None, N)[2] is None


def test_range_check_and_refusals_come_before_anything_is_built(cpu_ops):
    from triforce_amd.models.cache import OffloadingFlashSimpleCache
    from triforce_amd.utils import decoding as D
    from triforce_amd.utils.SpecTree_TP import SpecTree
    tok, g = Hh.FakeTokenizer(), Hh.load_golden("small_gamma6")
    ge, ids = Hh.build_product(g, "cpu"), torch.zeros(1, 8, dtype=torch.long)
    for bad in (-1, 21, 2.5):
        with pytest.raises(ValueError, match="top_logprobs"):
            D.TriForceRunner(tok, ge, g["gamma"], top_logprobs=bad)
        with pytest.raises(ValueError, match="top_logprobs"):
            D.Autoregressive(tok, ge, ids, max_len=4, top_logprobs=bad)
    llm = types.SimpleNamespace(temperature=0.6, top_p=0.9)
    for call in (lambda: D.TriForce_Dist(tok, llm, ids, top_logprobs=5), lambda: D._DistEngine(llm, top_logprobs=5),
                 lambda: SpecTree(None, top_logprobs=5), lambda: D.Baseline_Dist(tok, llm, ids, top_logprobs=5),
                 lambda: D.TriForceRunner(tok, types.SimpleNamespace(engine=ge.engine), g["gamma"], top_logprobs=5)):
        with pytest.raises(NotImplementedError, match="top_logprobs"):
            call()
    ge.engine.kv_cache = OffloadingFlashSimpleCache.__new__(OffloadingFlashSimpleCache)
    for call in (lambda: D.TriForceRunner(tok, ge, g["gamma"], top_logprobs=5),
                 lambda: D.TriForceSession(tok, ge, g["gamma"], top_logprobs=5),
                 lambda: D.Autoregressive(tok, ge, ids, max_len=4, top_logprobs=5)):
        with pytest.raises(NotImplementedError, match="top_logprobs.*OffloadingFlashSimpleCache"):
            call()


def test_keyword_off_adds_nothing_and_on_keeps_tokens_and_logprobs(lp_ops, monkeypatch):
    """The loop's bookkeeping with the device op restated on the host: no new key or op call with the keyword off; with it on
    the same tokens and ``logprobs``, and one (N pairs, rank) per emitted token."""
    from triforce_amd.utils import decoding as D
    from triforce_amd.utils.sampling import UniformSource
    calls = []

    def top_cpu(logits, targets, n, top_ids=None, top_lp=None, rank=None, out=None):
        calls.append(n)
        ids, lp, rk = lp_ops.token_top_logprobs_ref(logits, targets, n)
        top_ids.copy_(ids), top_lp.copy_(lp), rank.copy_(rk)
        token_logprobs_cpu(logits, targets, out=out)

    monkeypatch.setattr(lp_ops, "token_top_logprobs", top_cpu)
    g = Hh.load_golden("small_gamma6")
    prompt, tok = Hh.prompt_of(g), NoEosTokenizer()
    run = lambda **kw: D.TriForce(tok, Hh.build_product(g, "cpu", temperature=0.6, top_p=0.9), prompt, gamma=g["gamma"],  # noqa: E731
                                  max_len=24, return_details=True, rng=UniformSource("cpu", values=Hh.fixed_uniforms()),
                                  **SAMPLED, **kw)
    off = run(logprobs=True)
    assert not calls and "top_logprobs" not in off and "ranks" not in off
    on = run(top_logprobs=5)
    assert calls and set(calls) == {5}
    assert on["tokens"] == off["tokens"] and on["logprobs"] == off["logprobs"]
    assert len(on["top_logprobs"]) == len(on["ranks"]) == len(on["tokens"]) and all(len(p) == 5 for p in on["top_logprobs"])
    assert all((r <= 5) == (t in [i for i, _ in p]) for t, p, r in zip(on["tokens"], on["top_logprobs"], on["ranks"]))
