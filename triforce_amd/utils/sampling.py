"""Sampling helpers — mirror of the reference's utils/sampling.py (norm_logits :43-60,
top_k_top_p_filter :5-27, sample :63-66, max_fn :68-75), device-agnostic torch (plumbing that
runs inside the captured hipGraphs), plus the explicit uniform stream that feeds the device-side
sampler / accept kernels.

Tie rule: the reference sorts with torch.sort(descending=True), whose order among equal logits is
implementation-defined; here the sort is *stable* (lowest token id first among equals) so greedy
emulation (temperature=1, top_p->0) is deterministic on every device.
"""
import dataclasses
import math

import torch
from torch.nn import functional as F

from .. import ops


def top_k_top_p_filter(logits: torch.Tensor, top_k: int = 0, top_p: float = 0.0):
    if top_k > 0:
        kth = torch.topk(logits, min(top_k, logits.size(-1)))[0][:, [-1]]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    if top_p > 0.0:
        sorted_logits, sorted_indices = torch.sort(logits, descending=True, stable=True)
        cumulative = torch.cumsum(F.softmax(sorted_logits, dim=-1), dim=-1)
        # drop a sorted position when the mass BEFORE it already exceeds top_p (rank 0 always stays)
        drop_sorted = torch.zeros_like(cumulative, dtype=torch.bool)
        drop_sorted[..., 1:] = cumulative[..., :-1] > top_p
        drop = torch.zeros_like(drop_sorted).scatter(1, sorted_indices, drop_sorted)
        logits = logits.masked_fill(drop, float("-inf"))
    return logits


@dataclasses.dataclass(frozen=True)
class Filters:
    """The sampling settings of one distribution, as one comparable value.  Every top_k <= 0 means "no top-k" and is kept as
    -1, every min_p <= 0 means "no min-p" and is kept as 0.0 (reference utils/sampling.py:16), so two values are equal exactly
    when they normalise alike: the rule by which an engine's captured target verify may stand in for a runner's own
    (``serves``: DESIGN section 28)."""
    temperature: float
    top_p: float
    top_k: int = -1
    min_p: float = 0.0

    def __post_init__(self):
        if self.top_k <= 0:
            object.__setattr__(self, "top_k", -1)
        if self.min_p <= 0:
            object.__setattr__(self, "min_p", 0.0)

    @property
    def target_only(self):
        """Top-k or min-p is on: the filters of the TARGET's distribution that the two draft tiers never see."""
        return self.top_k > 0 or self.min_p > 0

    def kw(self):
        """The keywords of norm_logits (and of the engines' verify entry points); ``min_p`` only when it is on: without it the
        call is the one made before min-p existed."""
        kw = dict(temperature=self.temperature, top_k=self.top_k, top_p=self.top_p)
        if self.min_p > 0:
            kw["min_p"] = self.min_p
        return kw


@dataclasses.dataclass(frozen=True)
class Penalties:
    """The stateful settings of the TARGET's distribution as one comparable value: ``repetition`` (HF's
    rule over prompt and output, 1 = off), ``frequency`` and ``presence`` (OpenAI's, over the output only, 0 = off; negative
    values are legal).  Kept apart from Filters: they act on the logits before the normaliser and need the engine's state."""
    repetition: float = 1.0
    frequency: float = 0.0
    presence: float = 0.0

    def __post_init__(self):
        for name in ("repetition", "frequency", "presence"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"{name}_penalty={v!r} is not a finite number")
            object.__setattr__(self, name, float(v))
        if not self.repetition > 0.0:
            raise ValueError(f"repetition_penalty={self.repetition} must be > 0 (1 = off)")

    @property
    def on(self):
        return self.repetition != 1.0 or self.frequency != 0.0 or self.presence != 0.0


def _penalize_torch(logits, ids, state, penalties):
    """The formula of include/triforce_hip.h "SAMPLING PENALTIES" in torch: fp32, one operation per statement."""
    rows, V = logits.shape
    dev = logits.device
    x = logits.float()
    c = state.gen_count.to(device=dev, dtype=torch.int32).unsqueeze(0).repeat(rows, 1)
    if ids is not None:
        block = ids.reshape(-1)[:rows].to(dev)
        hit = torch.zeros(rows, V, dtype=torch.int32, device=dev)
        ok = (block >= 0) & (block < V)
        hit[torch.arange(rows, device=dev)[ok], block[ok]] = 1
        c = c + torch.cumsum(hit, dim=0, dtype=torch.int32)            # row i counts ids[0 .. i]
    seen = (state.prompt_seen.to(dev) != 0).unsqueeze(0) | (c > 0)
    r = torch.tensor(penalties.repetition, dtype=torch.float32, device=dev)
    f = torch.tensor(penalties.frequency, dtype=torch.float32, device=dev)
    p = torch.tensor(penalties.presence, dtype=torch.float32, device=dev)
    y = x
    if float(r) != 1.0:
        divided = x / r
        multiplied = x * r
        y = torch.where(seen, torch.where(x > 0, divided, multiplied), x)
    fc = f * c.to(torch.float32)
    less = y - fc
    less = less - p
    return torch.where(c > 0, less, y)


def penalize(logits, ids, state, penalties, out=None):
    """(rows, V) logits of the target -> the penalised rows: row i counts ``state.gen_count`` plus the
    block's input tokens ids[0 .. i] (``ids`` None: none).  Out of place, the state is only read.  fp32 device logits go to
    the kernel (ops.penalize_logits), anything else takes the torch restatement."""
    assert logits.dim() == 2
    if logits.is_cuda and logits.dtype == torch.float32:
        return ops.penalize_logits(logits, ids, state, penalties, out=out)
    return _penalize_torch(logits, ids, state, penalties)


def commit_penalties(state, ids_row, n):
    """state.gen_count[ids_row[j]] += 1 for j < n: the tokens a step left in the full cache.  One launch on the device
    (ops.penalty_commit), torch elsewhere; nothing is read back."""
    if state.gen_count.is_cuda:
        return ops.penalty_commit(state, ids_row, n)
    row = ids_row.reshape(-1)[:n]
    row = row[(row >= 0) & (row < state.V)]
    state.gen_count.index_add_(0, row, torch.ones_like(row, dtype=torch.int32))


# route of ops.topp_route -> the ops wrappers without top-k and min-p, with top-k, with min-p
_KERNELS = {"fused": ("topp_probs", "topk_topp_probs", "minp_probs"),
            "large": ("topp_probs_large", "topk_topp_probs_large", "minp_probs_large")}


def norm_logits(logits: torch.Tensor, temperature=0.6, top_k=-1, top_p=0.9, min_p=0.0) -> torch.Tensor:
    """(rows, vocab) fp32 logits -> probabilities after temperature / top-k / top-p / min-p (HF order; a token passes min-p only
    if its probability is at least min_p times the most likely token's: DESIGN section 27).  ops.topp_route names the form —
    one fused kernel with the row in LDS, the same select with the row streamed through a workspace, or the torch restatement
    — and the filters that are on name the kernel."""
    assert logits.dim() == 2
    route = ops.topp_route(logits.shape[-1], top_p, logits.is_cuda, logits.dtype)
    if route == "torch":
        probs = F.softmax(top_k_top_p_filter(logits / temperature, top_k=top_k, top_p=top_p), dim=-1)
        if min_p > 0.0:
            probs = probs.masked_fill(probs < min_p * probs.amax(dim=-1, keepdim=True), 0.0)
            probs = probs / probs.sum(dim=-1, keepdim=True)
        return probs
    plain, with_top_k, with_min_p = _KERNELS[route]         # (looked up on ops per call: tests and tools replace them by name)
    if min_p > 0.0:
        return getattr(ops, with_min_p)(logits.contiguous(), temperature, top_k, top_p, min_p)
    if top_k > 0:
        return getattr(ops, with_top_k)(logits.contiguous(), temperature, top_k, top_p)
    return getattr(ops, plain)(logits.contiguous(), temperature, top_p)


def max_fn(x):
    """norm(max(x, 0)) — the residual distribution of speculative sampling."""
    x_max = torch.where(x > 0, x, torch.zeros_like(x))
    return x_max / torch.sum(x_max, dim=-1, keepdim=True)


class UniformSource:
    """Device-resident stream of U[0,1) numbers consumed by the sampling / accept kernels.

    ``take(n)`` exposes the next n numbers (a device view) without consuming them; ``advance(k)``
    consumes k.  The reference draws lazily with torch.rand(1)/multinomial per decision
    (decoding.py:97,192); a stream with explicit consumption reproduces that order with zero host
    syncs.  ``values`` injects a fixed sequence (cycled) for parity tests.
    """

    MAX_TAKE = 256        # most numbers one kernel may look at (the Sequoia tree walk: one per examined child)

    def __init__(self, device, seed=None, values=None, block=1 << 16):
        self.device = torch.device(device)
        self.block = block
        self.pos = 0
        self._fixed = values is not None
        # Round 5: the buffer is allocated ONCE and refilled in place, and ``cursor`` is a device-resident int64 copy of
        # ``pos`` — kernels captured inside a hipGraph read their numbers as buf[cursor + k] and the kernel that closes a
        # decision advances the cursor itself (ops.*_cur); the host mirrors it with advance().  ``device_cursor`` says
        # whether the device copy is current: the plain take() / advance() users (eager kernels that get a pointer) leave it
        # stale, cursor_tensor() brings it up to date with one fill when it is.
        self.cursor = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.device_cursor = True
        if self._fixed:
            v = torch.as_tensor(values, dtype=torch.float32).flatten()
            reps = (block + self.MAX_TAKE + v.numel() - 1) // v.numel() + 1
            self._period = v.numel()
            self.buf = v.repeat(reps).to(self.device)
        else:
            self.gen = torch.Generator(device=self.device)
            if seed is not None:
                self.gen.manual_seed(seed)
            else:
                self.gen.seed()
            self.buf = torch.rand(block + self.MAX_TAKE, generator=self.gen, device=self.device)

    def _room(self, n):
        """Make sure buf[pos : pos + n] exists (refill / wrap, in place: captured graphs keep the buffer's address)."""
        assert n <= self.MAX_TAKE
        if self.pos + n > self.block:
            if self._fixed:
                self.pos %= self._period
            else:
                self.buf.copy_(torch.rand(self.block + self.MAX_TAKE, generator=self.gen, device=self.device))
                self.pos = 0
            self.device_cursor = False

    def take(self, n):
        self._room(n)
        return self.buf[self.pos:self.pos + n]

    def advance(self, k):
        """Consume k numbers on the host side only (an eager kernel got them through take())."""
        self.pos += int(k)
        self.device_cursor = False

    def cursor_tensor(self, n):
        """The device cursor, current and with room for n numbers: for kernels that read buf[cursor + k] (ops.*_cur)."""
        self._room(n)
        if not self.device_cursor:
            self.cursor.fill_(self.pos)
            self.device_cursor = True
        return self.cursor

    def advanced_on_device(self, k, at=None):
        """A *_cur kernel consumed k numbers and advanced the device cursor itself; ``at``: the cursor value it reported."""
        if at is not None and int(at) != self.pos:
            raise RuntimeError(f"uniform stream out of step: device cursor {int(at)} != host position {self.pos}")
        self.pos += int(k)


def sample(probs: torch.Tensor, num_samples=1, rng: UniformSource = None):
    """Draw one token id from ``probs`` ((V,) or (1,V)) -> int64 tensor of shape (1,1) on the device.
    Replaces torch.multinomial (sampling.py:63-66) by inverse-CDF sampling with an explicit uniform."""
    assert num_samples == 1
    p = probs.reshape(-1).contiguous()
    if rng is None:
        rng = _default_rng(p.device)
    out = torch.empty(1, dtype=torch.int64, device=p.device)
    ops.sample_inverse_cdf(p, rng.take(1), out)
    rng.advance(1)
    return out.view(1, 1)


_rngs = {}


def _default_rng(device):
    key = str(device)
    if key not in _rngs:
        _rngs[key] = UniformSource(device)
    return _rngs[key]
