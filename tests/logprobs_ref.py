"""Oracle-side references shared by tests/test_logprobs_cpu.py and tests/test_gpu_logprobs.py: the CPU
oracle's log-probabilities of a prompt and of a teacher-forced stream, each computed once per (golden, ids) and cached."""
import math

import torch

from tests import helpers as Hh

LOGIT_BAR = 1e-3          # the suite's logit bar: max(1e-3, 2 fp16 spacings at the largest |logit| of the row)


def fp16_spacing(x):
    """Distance between neighbouring fp16 numbers at magnitude x (normal range)."""
    return 2.0 ** (math.floor(math.log2(max(float(x), 6.2e-5))) - 10)


def row_bound(row):
    """2 x the logit bar on one oracle logits row: lp is a logit minus a log-sum-exp, and the log-sum-exp moves by at most
    the largest logit deviation."""
    return 2.0 * max(LOGIT_BAR, 2.0 * fp16_spacing(row.abs().max()))


def _lp(row, t):
    return float(torch.log_softmax(row.double(), dim=-1)[t])


_cache = {}


def _key(g, *ids):
    return (g["tseed"], g["prefill"], g["pseed"]) + tuple(tuple(int(t) for t in torch.as_tensor(i).reshape(-1)) for i in ids)


def prompt_reference(g, prompt):
    """(values, bounds): log p(prompt[i + 1] | prompt[:i + 1]) for i = 0 .. n - 2 from the oracle's logits over the whole
    prompt (its own 128-row chunks), and the per-position bound."""
    key = ("prompt",) + _key(g, prompt)
    if key not in _cache:
        eng, _, _ = Hh.build_oracle(g)
        eng.kv_cache.reset()
        ids = prompt[:, :-1]
        rows = torch.cat([eng.model.forward(ids[:, c:c + 128], eng.kv_cache, None)[0] for c in range(0, ids.shape[1], 128)])
        nxt = prompt[0, 1:]
        want = torch.log_softmax(rows.double(), dim=-1).gather(1, nxt[:, None])[:, 0]
        _cache[key] = (want, torch.tensor([row_bound(r) for r in rows], dtype=torch.float64))
    return _cache[key]


def teacher_forced_reference(g, context, stream):
    """(values, bounds) of ``stream`` fed through the oracle's autoregressive forward behind ``context`` (1, n), as
    helpers.teacher_forced_gaps walks it: stream[0] is scored from the context's last row, stream[i + 1] from the row of
    stream[i]."""
    key = ("stream",) + _key(g, context, stream)
    if key not in _cache:
        eng, _, _ = Hh.build_oracle(g)
        eng.kv_cache.reset()
        row = eng.inference(context)[0, -1]
        vals, bounds = [_lp(row, stream[0])], [row_bound(row)]
        for i in range(len(stream) - 1):
            row = eng.model.forward(torch.tensor([[stream[i]]]), eng.kv_cache, None)[0, -1]
            vals.append(_lp(row, stream[i + 1]))
            bounds.append(row_bound(row))
        _cache[key] = (torch.tensor(vals, dtype=torch.float64), torch.tensor(bounds, dtype=torch.float64))
    return _cache[key]


def check(got, want, bounds, what):
    """max |got - want| / bound per value < 1 and the mean deviation below 2 x the logit bar; both put on record."""
    got = torch.as_tensor(got, dtype=torch.float64).reshape(-1)
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} values, expected {tuple(want.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite log-probabilities"
    d = (got - want).abs()
    used, mean = float((d / bounds).max()), float(d.mean())
    print(f"[logprobs] {what}: max |d| {float(d.max()):.3e} ({used:.3f} of its bound), mean |d| {mean:.3e} "
          f"(bar {2 * LOGIT_BAR:.1e}), {got.numel()} values", flush=True)
    Hh.record("logprobs_max", used, what=what, max_abs=float(d.max()), n=int(got.numel()))
    Hh.record("logprobs_mean", mean / (2 * LOGIT_BAR), what=what, mean_abs=mean)
    assert used < 1.0, f"{what}: position {int((d / bounds).argmax())} is {float(d.max()):.3e} off, {used:.2f} of its bound"
    assert mean < 2 * LOGIT_BAR, f"{what}: mean deviation {mean:.3e}"
