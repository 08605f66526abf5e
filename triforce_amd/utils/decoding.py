"""Decode algorithms of the TriForce path — same entry points as the reference's utils/decoding.py:
Autoregressive (:14-37), TriForce (:41-160), Middle_Spec (:163-223) (+ the TP variants in
decoding_dist.py).  Same algorithm, same quirks, different execution:

  * every accept/reject decision, residual resample and bonus sample runs on the device
    (tf_accept_chain / tf_middle_accept / tf_sample_inverse_cdf); the host reads back ONE small int64
    record per inner step and ONE per outer step instead of >= gamma+2 blocking ``.item()`` /
    ``if r < ...`` syncs (decoding.py:97-121,190-193);
  * randomness comes from an explicit uniform stream (utils.sampling.UniformSource) consumed in
    the reference's decision order, so a run is reproducible and comparable across devices;
  * timing brackets the decode loop with device synchronisation (the reference omits it on-chip).
"""
import time

import numpy as np
import torch

from .. import ops
from . import sampling as _sampling
from .misc import log_csv, spec_stream
from .sampling import Filters, Penalties, UniformSource, norm_logits, sample

PAD_TOKEN = 100            # filler id of verify_tokens / pass_tokens (decoding.py:94,177)


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)


def _eos(tokenizer):
    e = getattr(tokenizer, "eos_token_id", None)
    return -1 if e is None else int(e)


@torch.inference_mode()
def Autoregressive(tokenizer, graph_engine, input_ids, max_len=256, top_k=-1, top_p=0.9, temperature=0.6, verbose=False,
                   rng=None, return_tokens=False, logprobs=False, min_p=0.0, repetition_penalty=1.0, frequency_penalty=0.0,
                   presence_penalty=0.0):
    """``min_p`` > 0: min-p behind top-k / top-p.  ``logprobs``: also the log-probability (temperature 1, unfiltered: DESIGN section 23) of every emitted token, scored
    on the device from the step's own logits -> (tokens / s, ids, logprobs).  The three penalties: every
    step's row is penalised with the engine's state and its own input token, which is then committed — on the device, no
    host sync in the loop; the log-probabilities stay those of the raw logits."""
    eng = graph_engine.engine
    device = eng.model.device
    pen = Penalties(repetition_penalty, frequency_penalty, presence_penalty)
    state = _penalty_state(graph_engine, pen)
    lp = None
    if logprobs:
        refusal = _logprobs_refusal(graph_engine, "logprobs")
        if refusal is not None:
            raise NotImplementedError(refusal)
        lp = torch.empty(max_len + 1, dtype=torch.float32, device=device)
    rng = rng or UniformSource(device)
    kw = Filters(temperature, top_p, top_k, min_p).kw()
    eng.kv_cache.reset()
    logits = graph_engine.inference(input_ids=input_ids)
    row = logits[:, -1, :]
    if pen.on:
        state.reset(input_ids)
        row = _sampling.penalize(row, None, state, pen)
    next_token = sample(norm_logits(row, **kw), rng=rng)
    if lp is not None:
        ops.token_logprobs(logits[:, -1, :], next_token.view(-1), out=lp[0:1])
    toks = [next_token]
    n = 0
    _sync(device)
    time1 = time.time()
    step = getattr(graph_engine, "decode_step", None) or \
        (lambda t: eng.model(input_ids=t, kv_cache=eng.kv_cache, graph_cache=None).logits)
    while n < max_len:      # no host sync inside the loop: the sampled token never leaves the device
        logits = step(next_token)
        if pen.on:                          # the row counts its own input token, which then joins the counts
            row = _sampling.penalize(logits[:, -1, :], next_token.view(-1), state, pen)
            _sampling.commit_penalties(state, next_token.view(-1), 1)
            next_token = sample(norm_logits(row, **kw), rng=rng)
        else:
            next_token = sample(norm_logits(logits[:, -1, :], **kw), rng=rng)
        toks.append(next_token)
        n += 1
        if lp is not None:                  # device targets, the step's own logits (a graph's static buffer until its next replay)
            ops.token_logprobs(logits[:, -1, :], next_token.view(-1), out=lp[n:n + 1])
    _sync(device)
    time2 = time.time()
    if verbose or return_tokens or logprobs:
        ids = torch.cat(toks, dim=1)[0].tolist()
        if verbose:
            for t in ids:
                spec_stream(t, tokenizer, "cyan")
        if logprobs:
            return n / (time2 - time1), ids, lp[:n + 1].tolist()
        if return_tokens:
            return n / (time2 - time1), ids
    return n / (time2 - time1)


def _penalty_state(graph_engine, penalties):
    """The engine's ops.PenaltyState for ``penalties`` (None when they are off: nothing is touched).  Refused before anything
    is captured or allocated over an engine that has none — the tensor-parallel and Sequoia engines, or a
    GraphInferenceEngine initialised without penalties."""
    if not penalties.on:
        return None
    state = getattr(graph_engine, "penalty_state", None)
    if state is None:
        raise NotImplementedError(
            f"repetition / frequency / presence penalties need the single-GPU GraphInferenceEngine initialised with them "
            f"(initialize_cuda_graph / initialize_eager(repetition_penalty=..., frequency_penalty=..., presence_penalty=...)); "
            f"{type(graph_engine).__name__} holds no penalty state")
    return state


def _logprobs_refusal(graph_engine, what):
    """Why ``logprobs`` / ``prompt_logprobs`` cannot be served over this engine (None: they can) — DESIGN section 23: the
    single-GPU GraphInferenceEngine over a resident FlashSimpleCache (fp16 or FP8) and a RetrievalCache."""
    from ..models.cache import FlashSimpleCache, RetrievalCache
    from .graph_infer import GraphInferenceEngine
    if not isinstance(graph_engine, GraphInferenceEngine):
        return (f"{what} is implemented for the single-GPU resident GraphInferenceEngine only, not for "
                f"{type(graph_engine).__name__} (tensor-parallel loop)")
    eng = graph_engine.engine
    if type(eng.kv_cache) is not FlashSimpleCache or type(eng.graph_cache) is not RetrievalCache:
        return (f"{what} is implemented for the resident FlashSimpleCache + RetrievalCache only, not for "
                f"{type(eng.kv_cache).__name__} + {type(eng.graph_cache).__name__}")
    return None


class _Record:
    """A small int64 decision record written by a kernel and read by the host once per (inner / outer) step.
    mailbox=True: the record lives in PINNED HOST memory that the kernel writes directly (unified addressing); the host
    arms it with a sentinel before the launch and polls — no device-to-host copy, no stream synchronisation (~20 us of
    idle GPU per read otherwise, 5 reads per step).  Else: a device tensor read with .tolist() (what TP needs: the
    record is broadcast over RCCL first)."""

    SENTINEL = -(1 << 62)

    def __init__(self, device, n, mailbox):
        self.n = n
        self.mailbox = bool(mailbox) and torch.device(device).type == "cuda"
        if self.mailbox:
            self.tensor = torch.zeros(n, dtype=torch.int64).pin_memory()
            self._np = self.tensor.numpy()
        else:
            self.tensor = torch.zeros(n, dtype=torch.int64, device=device)

    def arm(self, k):
        if self.mailbox:
            self._np[:k] = self.SENTINEL

    def read(self, k):
        if not self.mailbox:
            return self.tensor[:k].tolist()
        view, s, spins = self._np[:k], self.SENTINEL, 0
        while (view == s).any():
            spins += 1
            if spins > 50_000_000:
                raise RuntimeError("decision record never arrived (kernel failed?)")
        return view.tolist()


# One hipGraph per inner iteration (draft step, draw, retrieval verify, accept test: utils/graph_infer._InnerGraphs) instead
# of two replays + two eager kernels.  TRIFORCE_INNER_GRAPH=0: rounds 2-4's four launches.
# (Round 5 also built the two-stream form the round-4 trace suggested — every chain of launches between two record reads on
#  alternating streams, ordered by the record alone — and measured it on the same box against this form: +150..200 us per step
#  (profiles/r05_inner_loop_ab.jsonl: a launch into the OTHER hardware queue starts later than one behind the still-completing
#  accept kernel); it is also unsound without an explicit acquire at the head of every chain — the runtime knows nothing of an
#  ordering that goes through host memory.  Removed)
INNER_GRAPH = __import__("os").environ.get("TRIFORCE_INNER_GRAPH", "1") != "0"


class LookaheadPolicy:
    """When the inner loop replays the lookahead form of an iteration.  A lookahead replay costs two draft
    steps more than a plain one and saves a whole retrieval verify when its guess hits, so it pays while the hit rate stays
    above ``break_even`` (measured at capture: utils/graph_infer._InnerGraphs).  Over the last WINDOW lookahead replays: a hit
    rate below break_even switches to the plain graphs for the next REST logical iterations, then the form is probed again.
    The policy sees only decisions of the token path, so a run is reproducible; and it changes no token either way."""

    WINDOW, REST = 32, 128

    def __init__(self, break_even):
        self.break_even = float(break_even)
        self.recent, self.rest = [], 0
        self.switched_off = 0                      # times a window fell below break_even

    def on(self):
        return self.rest == 0

    def replayed(self, hit):
        """A lookahead replay was issued; ``hit``: it decided two iterations."""
        self.recent.append(1 if hit else 0)
        if len(self.recent) > self.WINDOW:
            self.recent.pop(0)
        if len(self.recent) == self.WINDOW and sum(self.recent) / self.WINDOW < self.break_even:
            self.rest, self.recent = self.REST, []
            self.switched_off += 1

    def passed(self, iterations):
        """``iterations`` logical inner iterations ran on the plain graphs while the policy was off."""
        self.rest = max(0, self.rest - int(iterations))


class LookaheadDepthPolicy:
    """Depth 3 against depth 2.  A depth-3 replay costs two draft steps more than a depth-2 one and saves
    a further retrieval verify when it decides a THIRD iteration, so it pays while the rate of third decisions per depth-3
    replay stays above ``break_even`` (the marginal cost measured at capture, as a fraction of a plain replay).  Over the last
    WINDOW depth-3 replays: a rate below break_even drops to depth 2 for the next REST logical iterations, then depth 3 is
    probed again.  Like LookaheadPolicy it sees only decisions of the token path and changes no token."""

    WINDOW, REST = 32, 128

    def __init__(self, break_even):
        self.break_even = float(break_even)
        self.recent, self.rest = [], 0
        self.switched_down = 0                     # times a window fell below break_even

    def on(self):
        return self.rest == 0

    def replayed(self, third):
        """A depth-3 replay was issued; ``third``: it decided three iterations."""
        self.recent.append(1 if third else 0)
        if len(self.recent) > self.WINDOW:
            self.recent.pop(0)
        if len(self.recent) == self.WINDOW and sum(self.recent) / self.WINDOW < self.break_even:
            self.rest, self.recent = self.REST, []
            self.switched_down += 1

    def passed(self, iterations):
        """``iterations`` logical inner iterations were decided by replays of depth <= 2."""
        self.rest = max(0, self.rest - int(iterations))


class _Lookahead:
    """What Middle_Spec keeps about the lookahead form between calls: the policies and the replay counters (on _SpecBuffers)."""

    def __init__(self, break_even, break_even3=None):
        self.policy = LookaheadPolicy(break_even)
        self.depth_policy = LookaheadDepthPolicy(break_even3) if break_even3 is not None else None
        self.verify_replays = self.lookahead_replays = self.lookahead_hits = self.lookahead_third = 0
        self.depth3_replays = 0


def lookahead_fits(rng, depth=2):
    """The lookahead form reads the uniforms of ``depth`` iterations behind the cursor.  The plain path would refill the
    stream's block between two iterations when the second one's three numbers did not fit (UniformSource._room): reading
    ahead across that point would take other numbers than the plain path, and with them other tokens.  So: only when all
    3 * depth numbers lie inside the current block."""
    return rng.pos + 3 * depth <= rng.block


_MAILBOX_OK = {}


def _mailbox_supported(device):
    """One-off probe per device: a kernel writes a pinned host record and the host sees it without any synchronisation
    (coherent pinned memory).  TRIFORCE_MAILBOX=0 forces the copy-back path."""
    import os
    key = str(torch.device(device))
    if key not in _MAILBOX_OK:
        ok = False
        if torch.device(device).type == "cuda" and os.environ.get("TRIFORCE_MAILBOX", "1") != "0":
            try:
                rec = _Record(device, 4, True)
                probs = torch.zeros(64, dtype=torch.float32, device=device)
                probs[5] = 1.0
                rec.arm(1)
                ops.sample_inverse_cdf(probs, torch.full((1,), 0.5, device=device), rec.tensor[:1])
                t0 = time.time()
                while int(rec._np[0]) == rec.SENTINEL and time.time() - t0 < 0.25:
                    pass
                ok = int(rec._np[0]) == 5
                torch.cuda.synchronize(device)
            except Exception:
                ok = False
        _MAILBOX_OK[key] = ok
    return _MAILBOX_OK[key]


class _SpecBuffers:
    """Per-engine device scratch reused across iterations (allocated once)."""

    def __init__(self, device, gamma, vocab, graph_engine=None, mailbox=False):
        tok_buf = getattr(graph_engine, "tok_buf", None)
        self.shared_inputs = tok_buf is not None and tok_buf.shape[1] >= gamma + 1
        if self.shared_inputs:
            # the engine's graphs read their tokens / positions from these very buffers: no input copies per replay
            self.verify_tokens = tok_buf[:, :gamma + 1]
            self.positions = graph_engine.pos_buf
        else:
            self.verify_tokens = torch.full((1, gamma + 1), PAD_TOKEN, dtype=torch.long, device=device)
            self.positions = torch.zeros((1, gamma + 1), dtype=torch.long, device=device)
        self.start_plan = self.pass_plan = None      # ops.SetTokensPlan of Middle_Spec's first launch / of the pass tokens
        self.inner_for = None                        # (inner-iteration graphs, the uniform stream they were captured for)
        self.spec_rows = torch.empty(gamma + 2, vocab, dtype=torch.float32, device=device)
        self.rows_generation = None                # lifetime token of static (un-copied) retrieval-verify rows
        mailbox = bool(mailbox) and _mailbox_supported(device)
        self.mid_out = _Record(device, ops.MID3_RECORD, mailbox)      # 4 entries of a plain iteration, 8 / 11 of a lookahead one
        self.lookahead = None                      # _Lookahead of the runner whose inner graphs have the lookahead form
        self.chain_out = _Record(device, 4, mailbox)
        self.pos_base = torch.arange(gamma + 1, dtype=torch.long, device=device).unsqueeze(0)
        # host -> device token lists go through one pinned staging row (a pageable source makes the copy synchronous)
        cuda = torch.device(device).type == "cuda"
        self.stage = torch.zeros(2, gamma + 4, dtype=torch.long, pin_memory=cuda)
        self.dev_tokens = torch.zeros(2, gamma + 4, dtype=torch.long, device=device)
        self._flip = 0

    def to_device(self, ids):
        """(1, len(ids)) int64 device tensor holding the python list ``ids``.  Two (staging, device) row pairs
        alternate: the row handed out by the previous call stays intact while this one is filled, and a staging row is
        rewritten only after a host sync (every decode step reads a decision record between two calls) has retired the
        copy that read it."""
        n = len(ids)
        self._flip ^= 1
        row = self.dev_tokens[self._flip, :n]
        if row.is_cuda and n <= 32:
            ops.set_tokens(row, ids, PAD_TOKEN)                # ids as kernel arguments: no staging copy, no H2D copy
            return row.unsqueeze(0)
        stage = self.stage[self._flip, :n]
        stage.copy_(torch.tensor(ids, dtype=torch.long))
        row.copy_(stage, non_blocking=True)
        return row.unsqueeze(0)


def _buffers(graph_engine, gamma, vocab, device, mailbox=False):
    b = getattr(graph_engine, "_tf_spec_buffers", None)
    stale = b is not None and getattr(graph_engine, "tok_buf", None) is not None \
        and b.verify_tokens.data_ptr() != graph_engine.tok_buf.data_ptr()        # graphs were re-captured
    if b is None or stale or b.verify_tokens.shape[1] != gamma + 1 or b.spec_rows.shape[1] != vocab \
            or b.mid_out.mailbox != (bool(mailbox) and _mailbox_supported(device)):
        b = _SpecBuffers(device, gamma, vocab, graph_engine, mailbox)
        graph_engine._tf_spec_buffers = b
    return b


@torch.inference_mode()
def Middle_Spec(next_token, graph_engine, gamma, verbose, tokenizer, rng=None, buffers=None, sync_record=None,
                health=None):
    """Inner loop: the 68M drafts one token at a time for the retrieval-cache model (decoding.py:163-223).
    Returns (ids [next, t1..t_g2], rows = device (g2, V) view of the retrieval-model prob rows, acceptance)."""
    eng = graph_engine.engine
    device = eng.model.device
    rng = rng or UniformSource(device)
    if buffers is None:
        buffers = _buffers(graph_engine, gamma, eng.model.config.vocab_size, device, mailbox=sync_record is None)
    inner = None
    if INNER_GRAPH and sync_record is None and buffers.mid_out.mailbox and buffers.shared_inputs:
        cached = getattr(buffers, "inner_for", None)           # (graphs, rng) the runner captured for exactly this stream
        if cached is not None and cached[1] is rng and cached[0].key[0] == gamma:
            inner = cached[0]
        elif hasattr(graph_engine, "inner_graphs"):
            inner = graph_engine.inner_graphs(gamma, rng, buffers.mid_out.tensor, capture=False)
    S = eng.kv_cache.seq_len
    n = accepted = drafted = 0
    ids = [int(next_token)]
    vt = buffers.verify_tokens
    # [next, PAD...] and the gamma + 1 positions S, S + 1, ... in one launch (the token id travels as a kernel argument)
    if vt.numel() <= 32 and buffers.positions.numel() <= 64:      # (tf_set_tokens' limits)
        position_ids = buffers.positions
        if vt.is_cuda:
            if buffers.start_plan is None:
                buffers.start_plan = ops.SetTokensPlan(vt.view(-1), position_ids)
            buffers.start_plan(ids, PAD_TOKEN, pos0=S)
        else:
            ops.set_tokens(vt, ids, PAD_TOKEN, pos=position_ids, pos0=S)
    else:
        vt.fill_(PAD_TOKEN)
        vt[0, 0] = ids[0]
        position_ids = torch.add(buffers.pos_base, S, out=buffers.positions)
    # the engines' graph replays can hand out their static output buffers (valid until the same graph replays again):
    # q_d and p are consumed by tf_middle_accept / the spec_rows copies before the next iteration asks for new ones
    noclone = dict(clone=False) if getattr(graph_engine, "static_outputs", False) else {}
    # the draft / verify graphs read vt itself: replay without looking at the inputs (this call sits between the host's
    # read of the previous accept record and the next launch — the one place where host time is GPU idle time)
    replay_draft = getattr(graph_engine, "replay_draft", None) if (noclone and buffers.shared_inputs) else None
    flat = vt.view(-1)
    look = buffers.lookahead if (inner is not None and inner.look) else None
    while inner is not None and n < gamma:
        # one launch, one read: [draft step n, draw, retrieval verify, accept test + follow-up draw] is ONE hipGraph whose
        # kernels take their three uniforms from the stream's device cursor and advance it
        rec = buffers.mid_out
        # the lookahead form (DESIGN sections 24, 25): this replay also decides the NEXT iteration(s) while its guesses of b are
        # right.  The largest depth whose rows and uniforms fit, then the two policies.
        depth = 1
        if look is not None and n in inner.look and lookahead_fits(rng) and look.policy.on():
            depth = 2
            if n in inner.look3 and lookahead_fits(rng, 3) and look.depth_policy.on():
                depth = 3
        if depth > 1:
            k = ops.mid_record_len(depth)
            rng.cursor_tensor(3 * depth)
            rec.arm(k)
            p = inner.replay(n, lookahead=depth)
            r = rec.read(k)                                                   # the one host read of these one to three steps
            ran = 1 + r[4]
            rng.advanced_on_device(3 * ran, r[3])
            decided = (tuple(r[0:3]),) + tuple(tuple(r[5 + 3 * s:8 + 3 * s]) for s in range(ran - 1))
            look.lookahead_replays += 1
            look.lookahead_hits += 1 if ran >= 2 else 0
            look.policy.replayed(ran >= 2)
            if depth == 3:
                look.depth3_replays += 1
                look.lookahead_third += 1 if ran == 3 else 0
                look.depth_policy.replayed(ran == 3)
        else:
            rng.cursor_tensor(3)
            rec.arm(4)
            p = inner.replay(n)
            acc, b, d, at = rec.read(4)                                       # the one host read of this step
            rng.advanced_on_device(3, at)
            decided = ((acc, b, d),)
            if look is not None:
                look.policy.passed(1)
        if depth < 3 and look is not None and look.depth_policy is not None:
            look.depth_policy.passed(len(decided))
        if look is not None:
            look.verify_replays += 1
        for acc, b, d in decided:                  # each one exactly an iteration of the plain loop
            drafted += 1
            if acc:                                                           # decoding.py:193-209
                ids += [d, b]
                accepted += 1
                n += 2
            else:                                                             # decoding.py:211-220
                ids.append(b)
                n += 1
            if verbose:
                for t, colour in (((d, "green"), (b, "blue")) if acc else ((b, "red"),)):
                    spec_stream(t, tokenizer, colour)
    if inner is not None:
        # row i of the LAST replay's static output is the retrieval model's distribution after tokens 0..i (see below)
        buffers.rows_generation = graph_engine.verify_generation()
        return ids, p[:len(ids) - 1], accepted / drafted
    while n < gamma:
        if replay_draft is not None:
            q_d = replay_draft(n)
        else:
            q_d = graph_engine.graph_draft_inference(input_ids=vt[:, :n + 1], gamma_offset=n, **noclone)
        u = rng.take(3)
        ops.sample_inverse_cdf(q_d, u[0:1], flat[n + 1:n + 2])               # d ~ q_d, written into verify_tokens
        if sync_record is not None:           # TP: rank 0's draft token is everyone's BEFORE the all-reduced verify runs
            sync_record(flat[n + 1:n + 2])    # on it (the reference's sample_dist, decoding.py:230-239,452)
        p = graph_engine.graph_verify(input_ids=vt, position_ids=position_ids, **noclone)
        rec = buffers.mid_out
        rec.arm(3)
        ops.middle_accept(p, q_d, flat, u[1:3], n, gamma, rec.tensor)         # accept test + follow-up sample
        if sync_record is not None:                                           # TP: rank 0's decision wins
            sync_record(rec.tensor)
            if n + 1 < flat.numel() and not _single_rank():                   # (one rank: the record IS the kernel's own)
                if flat.is_cuda:
                    ops.mid_record_tokens(rec.tensor, flat, n)               # one launch (the torch form below: six)
                else:
                    flat[n + 1:n + 3].copy_(_mid_tokens(rec.tensor, n, gamma, flat))
        acc, b, d = rec.read(3)                                               # the one host read of this step
        if health is not None:                # TP: a timed-out exchange NaN-filled p — stop before its tokens are used
            health()
        rng.advance(3)
        drafted += 1
        g = len(ids) - 1                                                      # == n: verify_tokens holds exactly ids
        if not noclone:
            buffers.spec_rows[g].copy_(p[n])                                  # decoding.py:193-220: q row(s) of this step
            if acc:
                buffers.spec_rows[g + 1].copy_(p[n + 1])
        if acc:                                                               # decoding.py:193-209
            ids += [d, b]
            accepted += 1
            n += 2
            if verbose:
                spec_stream(d, tokenizer, "green")
                spec_stream(b, tokenizer, "blue")
        else:                                                                 # decoding.py:211-220
            ids.append(b)
            n += 1
            if verbose:
                spec_stream(b, tokenizer, "red")
    if noclone:
        # Static verify output: row i of the LAST replay is the retrieval model's distribution after tokens 0..i —
        # the very row an earlier replay produced when position i was decided (same graph, same tokens <= i, same
        # cache; the kernels are deterministic), so the rows need not be copied out step by step.  The rows stay valid
        # only until the verify graph replays again: the caller checks ``rows_generation`` before consuming them.
        gen = getattr(graph_engine, "verify_generation", None)
        buffers.rows_generation = gen() if gen is not None else None
        return ids, p[:len(ids) - 1], accepted / drafted
    buffers.rows_generation = None
    return ids, buffers.spec_rows[:len(ids) - 1], accepted / drafted


def _single_rank():
    import torch.distributed as _d
    return not (_d.is_available() and _d.is_initialized() and _d.get_world_size() > 1)


def _mid_tokens(rec, n, gamma, flat):
    """verify_tokens[n+1 : n+3] implied by a (possibly broadcast) middle_accept record (acc, b, d)."""
    acc, b, d = rec[0], rec[1], rec[2]
    cur = flat[n + 1:n + 3].clone()
    first = torch.where(acc > 0, d, b)                 # accepted: d stays at n+1, b goes to n+2; rejected: b at n+1
    cur[0] = first
    if cur.numel() > 1:
        cur[1] = torch.where(acc > 0, b, cur[1])
    return cur


class TriForceRunner:
    """The TriForce outer loop (decoding.py:41-160) as prefill() + step(): ``TriForce`` below drives it to
    ``max_len`` tokens, bench.py drives it for an exact number of steps."""

    def __init__(self, tokenizer, graph_engine, gamma, top_k=-1, top_p=0.9, temperature=0.6, verbose=False, rng=None,
                 inclusive_accept=False, sync_record=None, rebuild_every=0, reanchor_at=0, logprobs=False,
                 prompt_logprobs=False, min_p=0.0, repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0):
        # filters: what the TARGET's distribution (first token, target verify) is normalised with.  top_k > 0 and min_p > 0 (a
        #              token stays only if its probability is at least min_p times the most likely token's, behind top-k / top-p:
        #              DESIGN section 27) apply to it alone; the draft tiers stay unfiltered
        self.filters = Filters(temperature, top_p, top_k, min_p)
        # penalties: repetition / frequency / presence on the TARGET's logits, in front of the normaliser;
        #              the draft tiers stay unpenalised, so decoding is lossless for the penalised target distribution.  The
        #              state lives with the engine (refused here, before anything is captured, over an engine without one)
        self.penalties = Penalties(repetition_penalty, frequency_penalty, presence_penalty)
        self.penalty_state = _penalty_state(graph_engine, self.penalties)
        # logprobs: keep the log-probability (temperature 1, unfiltered: DESIGN section 23) of every emitted token, scored on the
        #              device from the logits of the verify that produced it — one launch per step, no host read before stats()
        # prompt_logprobs: prefill() also scores the prompt, log p(input_ids[i + 1] | input_ids[:i + 1]) for i = 0 .. n - 2
        self.logprobs, self.want_prompt_logprobs = bool(logprobs), bool(prompt_logprobs)
        self._lp, self._lp_n, self.prompt_logprobs = None, 0, None
        # rebuild_every: N > 0 re-selects the retrieval cache's prefill chunks during every N-th target verify
        #                (SURVEY 8f row 4); 0 = the reference's behaviour, one build per prompt
        self.rebuild_every, self.rebuilds = int(rebuild_every), 0
        # reanchor_at: N > 0 re-anchors the retrieval cache at the top of a step whose verify block would
        #                take the generated tail past N rows: the confirmed rows are folded into the covered region
        #                (RetrievalCache.reanchor), this step's verify re-selects over it and the tail starts again, so
        #                generation and extend() may pass the retrieval budget; 0 = the covered region is fixed
        self.reanchor_at, self.reanchors = int(reanchor_at), 0
        # eager_every: N > 0 runs every N-th target verify eagerly instead of replaying its hipGraph, so that
        #              bench.py can bracket individual attention launches with HIP events inside the timed region
        self.eager_every = 0
        # inclusive_accept: marks the TP outer loop — it tests ``r <=`` (decoding.py:347) where on-chip tests ``r <``
        #              (:99), and it ends at an eos that closes the accept scan (:382-383) where on-chip keeps going
        # sync_record: optional callable applied to each device decision record before it is read (TP: broadcast
        #              from rank 0, the role of sample_dist / the r broadcast, decoding.py:230-239,345-346)
        self.inclusive_accept, self.sync_record = inclusive_accept, sync_record
        # health: optional callable run once per outer step right after the step's host read (TP: raises when the
        #              one-shot all-reduce has timed out — its outputs are NaN-filled from then on, csrc/allreduce.hip)
        self.health = None
        self.tokenizer, self.ge, self.eng = tokenizer, graph_engine, graph_engine.engine
        self.gamma, self.verbose = gamma, verbose
        if self.logprobs or self.want_prompt_logprobs:  # (refused before anything is captured or allocated)
            refusal = self._extend_refusal("logprobs / prompt_logprobs")
            if refusal is not None:
                raise NotImplementedError(refusal)
        if self.reanchor_at != 0:                      # (refused before anything is captured or allocated)
            refusal = self._extend_refusal("reanchor_at")
            if refusal is not None:
                raise NotImplementedError(refusal)
            if not gamma + 2 <= self.reanchor_at <= self.eng.graph_cache.max_budget:
                raise ValueError(f"reanchor_at={self.reanchor_at} is outside [gamma + 2, max_budget] = [{gamma + 2}, "
                                 f"{self.eng.graph_cache.max_budget}]: one verify block must fit below it, and it below the "
                                 "retrieval budget")
        self.device = self.eng.model.device
        self.rng = rng or UniformSource(self.device)
        self.eos = _eos(tokenizer)
        self.bufs = _buffers(graph_engine, gamma, self.eng.model.config.vocab_size, self.device,
                             mailbox=sync_record is None)
        self.inner = None
        if INNER_GRAPH and sync_record is None and self.bufs.mid_out.mailbox and self.bufs.shared_inputs \
                and hasattr(graph_engine, "inner_graphs"):
            self.inner = graph_engine.inner_graphs(gamma, self.rng, self.bufs.mid_out.tensor)   # captured here, not in a step
            self.bufs.inner_for = (self.inner, self.rng) if self.inner is not None else None
        # the lookahead form of the inner iterations: policy + counters live with the buffers Middle_Spec is handed
        self.bufs.lookahead = _Lookahead(self.inner.break_even, self.inner.break_even3) \
            if (self.inner is not None and self.inner.look) else None
        self.resample_count = self.accepted_count = self.target_sample_count = self.draft_count = 0
        self.n = 0
        self.inner_iters = 0          # LOGICAL Middle_Spec iterations (decisions); the lookahead form decides up to two per
        #                               retrieval-verify replay: stats()['verify_replays'] counts the replays
        self.emitted, self.counts, self.acc_rate_middle_list = [], [], []
        self.next_token, self.last_reason = None, None
        # extend(): the ids of the full cache's rows — ``history`` (1, n) as of the last prefill() / extend(), ``_fed`` the rows
        # the steps appended since — and, with ``time_extend``, the split of the last extend() in seconds
        self.history, self._fed = None, []
        self.time_extend, self.extend_seconds = False, None
        # the prompt-lookup n-gram draft tier: its NgramCache, whose history every step appends the rows it
        # leaves in the full cache to; None over the 68M tier, where nothing below changes
        from ..models.ngram_draft import NgramCache
        dc = getattr(self.eng, "draft_cache", None)
        self.ngram = dc if isinstance(dc, NgramCache) else None

    @torch.inference_mode()
    def prefill(self, input_ids, prompt_logprobs=None):
        """``prompt_logprobs`` (None: the runner's setting): score the prompt in the same pass — ``self.prompt_logprobs`` is the
        (n - 1,) fp32 device tensor of log p(input_ids[i + 1] | input_ids[:i + 1]), handed out by stats()."""
        eng, ge = self.eng, self.ge
        score = self.want_prompt_logprobs if prompt_logprobs is None else bool(prompt_logprobs)
        if score and not self.want_prompt_logprobs:
            refusal = self._extend_refusal("prompt_logprobs")
            if refusal is not None:
                raise NotImplementedError(refusal)
        eng.kv_cache.reset()
        eng.graph_cache.reset()
        eng.draft_cache.reset()
        self.prompt_logprobs = None
        if score:
            self.prompt_logprobs = ge.inference(input_ids=input_ids[:, :-1], next_ids=input_ids[0, 1:].contiguous())[1]
        else:
            ge.inference(input_ids=input_ids[:, :-1])
        logits = ge.inference(input_ids=input_ids[:, -1:])         # q_len==1 -> the retrieval cache is built here
        ge.graph_draft_prefill(input_ids=input_ids)
        if self.verbose:
            eng.kv_cache.print_status()
            eng.graph_cache.print_status()
            eng.draft_cache.print_status()
        self.calibrate_aligned()
        if self.penalties.on:
            self.penalty_state.reset(input_ids)            # the context is the prompt; nothing generated yet
        self.start(logits)
        self.history, self._fed = input_ids, []

    def _extend_refusal(self, what="extend()"):
        """Why extend() — or re-anchoring, the same gate — cannot run over this engine (None: it can)."""
        from ..models.cache import FlashSimpleCache, RetrievalCache
        from .graph_infer import GraphInferenceEngine
        if not isinstance(self.ge, GraphInferenceEngine) or self.sync_record is not None or self.inclusive_accept:
            return (f"{what} is implemented for the single-GPU resident GraphInferenceEngine only, not for "
                    f"{type(self.ge).__name__} (tensor-parallel loop)")
        if type(self.eng.kv_cache) is not FlashSimpleCache or type(self.eng.graph_cache) is not RetrievalCache:
            return (f"{what} is implemented for the resident FlashSimpleCache + RetrievalCache only, not for "
                    f"{type(self.eng.kv_cache).__name__} + {type(self.eng.graph_cache).__name__}")
        return None

    @torch.inference_mode()
    def extend(self, input_ids, keep=None):
        """Continue from a prefilled runner without touching rows [0, keep) of the full cache.

        keep=None: a chat turn — everything generated so far stays and the rows fed are [pending next_token] + input_ids (the
        pending token was emitted, its K/V is not in the cache yet).  keep=k: a new question on the same document — the full
        cache is rolled back to k rows (retrieval.prefill <= k <= seq_len), then input_ids are fed.  All rows but the last go
        through the engine's prefill (> 64 rows) or verify (2..64 rows) route, one row through the autoregressive step; the
        last row is fed alone and re-selects the retrieval cache for its query; the draft's StreamingLLM cache is refilled
        over the whole token history.  Every bound is checked before any state changes (ValueError names the limit).

        On a runner with ``reanchor_at`` > 0 the retrieval tail is no bound: a turn that would cross it
        re-anchors the retrieval cache to the chunk boundary below the last row fed, between the body rows and the last
        row's forward; and keep=k may lie below the covered region once that has grown (prefill0 <= k): the cache is
        re-anchored down to the chunk boundary below k first."""
        from ..models.cache import TOPK_MAX_CHUNKS
        eng, ge, gamma = self.eng, self.ge, self.gamma
        refusal = self._extend_refusal()
        if refusal is not None:
            raise NotImplementedError(refusal)
        kv, rc, dc = eng.kv_cache, eng.graph_cache, eng.draft_cache
        if self.history is None or self.next_token is None:
            raise ValueError("extend() continues a prefilled runner: call prefill() first")
        ids = torch.as_tensor(input_ids, dtype=torch.long, device=self.device).reshape(1, -1)
        if ids.shape[1] == 0:
            raise ValueError("extend() needs at least one input token")
        S, P = kv.seq_len, rc.prefill
        moving, chunk = self.reanchor_at > 0, rc.chunk_size
        known = self.history.shape[1] + len(self._fed)
        if keep is None:
            k, rows = S, ids.shape[1] + 1
        else:
            k, rows = int(keep), ids.shape[1]
            if moving and not rc.prefill0 <= k <= S:
                raise ValueError(f"keep={k} is outside [{rc.prefill0}, {S}]: the retrieval cache covers rows [0, "
                                 f"{rc.prefill0}) at the least and the full cache holds {S} rows")
            if not moving and not P <= k <= S:
                raise ValueError(f"keep={k} is outside [{P}, {S}]: the retrieval cache covers rows [0, {P}) and the full "
                                 f"cache holds {S} rows")
        # the covered region while the body rows are fed (below P: rows of it are about to be rewritten) and for the last row
        P_feed = P if k >= P else (k // chunk) * chunk
        P_last = P_feed
        if known < k:
            raise ValueError(f"the runner knows the ids of {known} cache rows, keep needs {k} (the cache length was changed "
                             "behind the runner)")
        room = gamma + 2                                   # one decode step's verify block
        if k + rows - P_feed + room > rc.max_budget:
            if not moving:
                raise ValueError(f"retrieval tail {k} + {rows} - {P} rows + {room} rows for one decode step exceeds the "
                                 f"retrieval budget max_budget={rc.max_budget}: the covered region [0, {P}) is fixed when the "
                                 "engine is built")
            P_last = ((k + rows - 1) // chunk) * chunk
            if P_last // chunk > TOPK_MAX_CHUNKS:
                raise ValueError(f"{k} + {rows} rows need the retrieval cache to cover {P_last // chunk} chunks of {chunk} rows, "
                                 f"more than the top-k's limit of {TOPK_MAX_CHUNKS} chunks")
        if k + rows + room > kv.max_budget:
            raise ValueError(f"{k} + {rows} rows + {room} rows for one decode step exceeds the full cache's capacity "
                             f"max_budget={kv.max_budget}")
        if k + rows <= 64:
            raise ValueError(f"a token history of {k + rows} rows is too short for the draft's prefill route (> 64 rows)")

        # ---- state changes from here ----
        t = [self._extend_mark()]
        hist = self.history
        if self._fed:
            hist = torch.cat([hist, torch.tensor(self._fed, dtype=torch.long, device=self.device).unsqueeze(0)], dim=1)
        new = ids if keep is not None else torch.cat([torch.tensor([[self.next_token]], dtype=torch.long, device=self.device),
                                                      ids], dim=1)
        hist = torch.cat([hist[:, :k], new], dim=1)
        kv.seq_len = k                                     # rows [0, k) stay as they are, the rest is overwritten
        moved = 0
        if P_feed != P:
            rc.reanchor(P_feed)
            moved += 1
        body = new[:, :-1]
        if body.shape[1] == 1:                             # (q_len == 1 through inference() would build the retrieval cache)
            ge.decode_step(body)
        elif body.shape[1] > 1:
            ge.inference(input_ids=body)
        t.append(self._extend_mark())
        if P_last != P_feed:                               # every row below P_last is in the full cache now
            rc.reanchor(P_last)
            moved += 1
        logits = ge.inference(input_ids=new[:, -1:], rebuild_retrieval=True)   # selection for THIS query over [0, P) + tail
        ge.update_graph_cache()                            # (the last layer's tail copy ran before seq_len advanced)
        t.append(self._extend_mark())
        dc.reset()
        dc.seq_len = 0                                     # a clean refill: the window a first prompt of these ids leaves
        ge.graph_draft_prefill(input_ids=hist)
        t.append(self._extend_mark())
        assert kv.seq_len == k + rows == hist.shape[1]
        self.history, self._fed = hist, []
        ge.dev_len = None                                  # the verify graphs' device scalars: re-synchronised by the next step
        self.bufs.rows_generation = None
        self.resample_count = self.accepted_count = self.target_sample_count = self.draft_count = 0
        self.n = self.inner_iters = self.rebuilds = 0
        self.reanchors = moved
        self.counts, self.acc_rate_middle_list, self.last_reason = [], [], None
        if self.penalties.on:
            self.penalty_state.reset(hist)                 # a fresh request whose prompt is the conversation so far
        self.start(logits)                                 # (take + advance: the uniform stream's device cursor is re-written
        if self.time_extend:                               #  before its next reader)
            self.extend_seconds = dict(target_feed=t[1] - t[0], retrieval_rebuild=t[2] - t[1], draft_refill=t[3] - t[2],
                                       rows=rows, keep=k)

    def _extend_mark(self):
        if not self.time_extend:
            return 0.0
        _sync(self.device)
        return time.time()

    def calibrate_aligned(self):
        """Aligned synthetic weights (models/aligned.py) need one calibration of the lm_head's attention read-out once
        a prompt's full and retrieval caches exist; real or random weights: no-op."""
        info = getattr(getattr(getattr(self.eng, "model", None), "weights", None), "aligned", None)
        if info is None or info.get("role") != "target" or "calibration" in info:
            return None
        from ..models import aligned
        return aligned.calibrate_engine(self.ge, self.gamma, self.filters.temperature, self.filters.top_p)

    @torch.inference_mode()
    def start(self, logits):
        row = logits[:, -1, :]
        if self.penalties.on:                          # the first token: no block ids, the state as prefill() / extend() left it
            row = _sampling.penalize(row, None, self.penalty_state, self.penalties)
        probs = norm_logits(row, **self.filters.kw())
        self.next_token = int(sample(probs, rng=self.rng))
        if self.verbose:
            spec_stream(self.next_token, self.tokenizer, "cyan")
        self.emitted = [self.next_token]
        if self.logprobs:
            self._lp_n = 0                             # (a new answer: extend() starts here too)
            self._score(logits[0, -1:], [self.next_token])

    def _score(self, logits, ids):
        """Append the log-probabilities of ``ids`` under rows 0 .. len(ids) - 1 of the (rows, V) fp32 ``logits`` to the device
        buffer, in emission order: one launch, the ids as kernel arguments, nothing read back."""
        k, n = len(ids), self._lp_n
        if k == 0:
            return
        if self._lp is None or n + k > self._lp.numel():
            grown = torch.empty(max(1024, 2 * (n + k)), dtype=torch.float32, device=self.device)
            if n:
                grown[:n].copy_(self._lp[:n])
            self._lp = grown
        ops.token_logprobs(logits[:k], list(ids), out=self._lp[n:n + k])
        self._lp_n = n + k

    def _device_sets(self):
        """The captured verify graphs' device scalars (``ge.verify_sets``) when this runner sets its steps up on the device, else
        None.  Then the outer accept kernel (tf_accept_chain_step) writes the catch-up draft's pass tokens and the next verify's
        positions / slot / key count, and the verify reads its tokens from the shared token buffer, where the inner graphs left
        [next, t_1 .. t_g2]: the chain behind the last inner record is one graph replay, no set-up launch.  An eager or rebuild
        step still sets its verify up from the host."""
        if self.inner is None or self.sync_record is not None or self.inclusive_accept or not self._served():
            return None
        return self.ge.verify_sets(self.gamma)

    def _served(self):
        """The engine's captured target verify was normalised with exactly THIS runner's filters (``serves``: DESIGN section 28)
        behind exactly its penalties, so its probabilities may be used: what every fast verify route asks.
        An engine without ``serves`` captured without top-k, min-p and penalties."""
        serves = getattr(self.ge, "serves", None)
        if serves is None:
            return not self.filters.target_only and not self.penalties.on
        return serves(self.filters, self.penalties) if self.penalties.on else serves(self.filters)

    def _pen_kw(self):
        """``penalties`` for the engines' verify entry points, only when they are on: without it the call is the one made
        before penalties existed."""
        return dict(penalties=self.penalties) if self.penalties.on else {}

    @torch.inference_mode()
    def step(self):
        """One outer iteration: Middle_Spec drafting, target verify over the full KV, device-side
        accept/rollback, cache fix-ups.  Returns the number of tokens emitted."""
        eng, ge, gamma, device, bufs, rng = self.eng, self.ge, self.gamma, self.device, self.bufs, self.rng
        tokenizer, verbose = self.tokenizer, self.verbose
        next_token = self.next_token
        n0 = self.n
        # re-anchor: between steps seq_len is the rolled-back length, so rows [0, seq_len) are confirmed.
        # Only the bound moves here (nothing the drafting below reads); this step's verify re-selects over the new region and
        # the tail copy behind it starts at the new bound
        reanchor = False
        if self.reanchor_at > 0:
            kv, rc = eng.kv_cache, eng.graph_cache
            if kv.seq_len - rc.prefill + gamma + 2 > self.reanchor_at:
                rc.reanchor((kv.seq_len // rc.chunk_size) * rc.chunk_size)
                self.reanchors += 1
                reanchor = True
        # health (TP): a plain load of the pinned mirror of the exchange's error word after EVERY inner record read — after a
        # timed-out exchange the probabilities are NaN-filled, and without the check up to gamma more iterations would draft,
        # append draft KV and write token ids from them before the outer step noticed
        ids, spec_rows, acc_mid = Middle_Spec(next_token, ge, gamma, False, tokenizer, rng=rng, buffers=bufs,
                                              sync_record=self.sync_record, health=self.health)
        self.acc_rate_middle_list.append(acc_mid)
        generated = ids[1:]
        g2 = len(generated)
        self.draft_count += g2
        self.inner_iters += int(round(g2 / (1.0 + acc_mid)))        # g2 = iterations + accepted drafts

        # target model verifies [next, t1..t_g2] against the full KV cache
        rebuild = self.rebuild_every > 0 and (len(self.counts) + 1) % self.rebuild_every == 0
        self.rebuilds += int(rebuild)
        rebuild = rebuild or reanchor                                  # (one rebuild serves both)
        eager = self.eager_every > 0 and (len(self.counts) + 1) % self.eager_every == 0
        served = self._served()
        sets = self._device_sets()
        on_device = sets is not None and not rebuild and not eager
        logits = None                                                  # (set by the last route below only)
        if on_device:
            if not ge.verify_lengths_current(gamma):
                ge.sync_verify_lengths(gamma)                          # stale (first step, after an eager / rebuild step): one launch each
            tg = ge.target_graphs[len(ids)]
            probs, verify_tokens = tg.replay_in_place(), tg.ids
        elif served and not rebuild and not eager and hasattr(ge, "verify_probs_ids") and len(ids) <= 32 \
                and (fast := ge.verify_probs_ids(ids, **self.filters.kw(), **self._pen_kw())) is not None:
            # captured forward + temperature / top-p: ids, positions and lengths set by ONE launch (ids as kernel arguments)
            probs, verify_tokens = fast
        else:
            verify_tokens = bufs.to_device(ids)
            if served and hasattr(ge, "verify_probs"):                 # one hipGraph: forward + temperature / top-k / top-p
                probs = ge.verify_probs(verify_tokens, rebuild_retrieval=rebuild, eager=eager, **self.filters.kw(),
                                        **self._pen_kw())
            else:
                logits = ge.inference(input_ids=verify_tokens, rebuild_retrieval=True) if rebuild \
                    else (ge.inference(input_ids=verify_tokens, eager=True) if eager else ge.inference(input_ids=verify_tokens))
                rows = logits[0]
                if self.penalties.on:                                  # out of place: ``logits`` stays raw (logprobs below)
                    rows = _sampling.penalize(rows, verify_tokens.view(-1), self.penalty_state, self.penalties)
                probs = norm_logits(rows, **self.filters.kw())
        if getattr(bufs, "rows_generation", None) is not None:
            # spec_rows is a view of the retrieval-verify graph's static output: nothing may have replayed that graph
            # between Middle_Spec's return and this read (the target verify above is a different graph)
            assert ge.verify_generation() == bufs.rows_generation, "retrieval-verify graph replayed before its rows were consumed"
        rec = bufs.chain_out
        rec.arm(4)
        on_cursor = self.inner is not None and self.sync_record is None
        if on_device:
            # the accept kernel also leaves the pass tokens in the token buffer and the NEXT verify's scalars (rolled-back
            # length) on the device
            ops.accept_chain_step(probs, spec_rows, ge.tok_buf.view(-1), rng.buf, rng.cursor_tensor(g2 + 1), g2, False, self.eos,
                                  PAD_TOKEN, ge.target_graphs[len(ids)].slot, sets, rec.tensor)
        elif on_cursor:
            # the uniform stream's device cursor is live (the inner-iteration graphs advance it): the chain reads its numbers
            # behind it and advances it by what it consumed, so no step ever has to re-synchronise the device copy
            ops.accept_chain_cur(probs, spec_rows, verify_tokens.view(-1)[1:], rng.buf, rng.cursor_tensor(g2 + 1), g2,
                                 self.inclusive_accept, self.eos, rec.tensor)
        else:
            ops.accept_chain(probs, spec_rows, verify_tokens.view(-1)[1:], rng.take(g2 + 1), g2, self.inclusive_accept,
                             self.eos, rec.tensor)
        if self.sync_record is not None:
            self.sync_record(rec.tensor)
        count, pred, reason, consumed = rec.read(4)                      # the one host read of the outer step
        if self.penalties.on:
            # the pass tokens [next_token] + generated[:count] join the counts: they are the head of the verify block's own
            # device row in every route (the accept kernel writes behind them).  One launch, outside every graph; the
            # resampled / bonus token stays pending and is counted by the next block's row 0
            _sampling.commit_penalties(self.penalty_state, verify_tokens.view(-1), count + 1)
        if self.ngram is not None:
            # the same head of the verify block's device row — the rows this step leaves in the full cache (``_fed`` below) —
            # joins the n-gram draft's history: one launch, outside every graph, confirmed tokens only
            self.ngram.commit(verify_tokens.view(-1), count + 1)
        if self.health is not None:
            self.health()
        dp = getattr(getattr(eng, "draft", None), "_persist", None)                        # one-launch draft forward: pinned mirror of its error word
        if dp is not None:
            dp.check()
        dev_consumed = consumed
        if self.inclusive_accept and reason == 1 and generated[g2 - 1] == self.eos:
            # TP loop only: an eos accepted as the LAST drafted token ends the loop before the bonus sample
            # (decoding.py:357-360,382-383); the on-chip loop — and tf_accept_chain — go on to the bonus token (:127)
            reason, pred, consumed = 2, self.eos, consumed - 1
        if on_cursor:
            rng.advanced_on_device(dev_consumed)
            if consumed != dev_consumed:                                 # the kernel drew a bonus number the loop does not consume:
                rng.pos -= dev_consumed - consumed                       # step the host position back; the device cursor is
                rng.device_cursor = False                                # re-written before its next reader
        else:
            rng.advance(consumed)
        self.last_reason = reason          # 0 rejection + resample, 1 everything accepted (bonus token), 2 accepted eos
        if self.logprobs:
            # rows 0 .. count of the verify that just ran are the target's distributions for generated[:count] and for the
            # resampled / bonus token: scored HERE, before any later launch of this step can touch a static logits buffer
            if on_device:
                vlogits = ge.target_graphs[len(ids)].logits
            else:                                      # verify_probs_ids / verify_probs leave theirs with the engine
                vlogits = ge.last_logits if logits is None else logits
            self._score(vlogits[0], generated[:count] + ([pred] if reason != 2 else []))

        pass_tokens = [next_token] + generated[:count] + [PAD_TOKEN] * (g2 + 1 - count)
        self._fed += pass_tokens[:count + 1]          # the rows this step leaves in the full cache (extend)
        if reason != 2:
            pass_tokens[count + 1] = pred             # the resampled (:111-118) or the bonus (:127-134) token

        # Launch order (not the reference's statement order; the three pieces touch disjoint buffers): the 68M catch-up
        # forward (:137-139) goes FIRST — ~120 us of device work behind which the host issues the tail copies, the window
        # shift and the next iteration's first launches; issued last, each of those short launches was a host-bound gap
        # (profiles/r04_gap_analysis_decode_steps.txt).
        # The pass tokens go straight into the draft graphs' static input when they fit (the next Middle_Spec re-initialises
        # it): one launch, no copies.
        tok_buf = getattr(ge, "tok_buf", None)
        in_tok_buf = tok_buf is not None and tok_buf.shape[0] == 1 and tok_buf.shape[1] >= len(pass_tokens) and tok_buf.is_cuda \
            and len(pass_tokens) <= 32
        if self.ngram is not None:
            # the n-gram tier has no catch-up forward: its state is the history the commit above appended to
            if on_device:
                ge.dev_len = eng.kv_cache.seq_len - (g2 - count)
        elif on_device:
            ge.dev_len = eng.kv_cache.seq_len - (g2 - count)            # what the accept kernel wrote: the rolled-back length
            ge.replay_draft(g2 + 1)                                      # the pass tokens are in the token buffer already
        elif in_tok_buf and hasattr(ge, "replay_draft") and getattr(ge, "static_outputs", False) and tok_buf.numel() <= 32:
            if bufs.pass_plan is None:
                bufs.pass_plan = ops.SetTokensPlan(tok_buf.view(-1))
            bufs.pass_plan(pass_tokens, PAD_TOKEN, n_dst=len(pass_tokens))
            ge.replay_draft(g2 + 1)                                       # (the graph reads tok_buf itself: no input checks)
        elif in_tok_buf:
            row = tok_buf[:, :len(pass_tokens)]
            ops.set_tokens(row, pass_tokens, PAD_TOKEN)
            ge.graph_draft_inference(input_ids=row, gamma_offset=g2 + 1)
        else:
            ge.graph_draft_inference(input_ids=bufs.to_device(pass_tokens), gamma_offset=g2 + 1)

        eng.kv_cache.seq_len -= (g2 - count)                              # rollback (:124)
        if sets is not None and not on_device:
            # this step set its verify up from the host (eager / rebuild step): bring the device scalars to the rolled-back
            # length HERE, behind the catch-up draft forward, not at the head of the next step's verify chain
            ge.sync_verify_lengths(gamma)
        ge.update_graph_cache()                                           # refresh the retrieval tail (:125)

        self.accepted_count += count
        self.n += count
        self.emitted += generated[:count]
        if verbose:
            for t in generated[:count]:
                spec_stream(t, tokenizer, "green")
        if reason == 0:                                                   # rejection -> residual resample (:111-118)
            self.resample_count += 1
            self.n += 1
            self.emitted.append(pred)
            if verbose:
                spec_stream(pred, tokenizer, "red")
        elif reason == 2:                                                 # accepted eos (:108-110)
            self.draft_count -= g2 - count
        else:                                                             # everything accepted -> bonus token (:127-134)
            self.target_sample_count += 1
            self.n += 1
            self.emitted.append(pred)
            if verbose:
                spec_stream(pred, tokenizer, "blue")
            count += 1
        self.counts.append(count)

        dc = eng.draft_cache
        dc.evict_for_spec(dc.start_size + dc.recent_size + count)
        self.next_token = pred
        return self.n - n0

    def stats(self, seconds):
        acceptance_rate = self.accepted_count / max(self.draft_count, 1)
        extra = {}
        if self.logprobs:                              # the one device-to-host read of the values
            extra["logprobs"] = self._lp[:self._lp_n].tolist()
            assert len(extra["logprobs"]) == len(self.emitted)
        if self.prompt_logprobs is not None:
            extra["prompt_logprobs"] = self.prompt_logprobs.float().cpu()
        look = self.bufs.lookahead
        # retrieval-verify replays the inner loop issued (0 when it does not run on the inner-iteration graphs' lookahead
        # form: then every inner iteration is one replay), how many carried the lookahead, how many of those decided two
        extra.update(verify_replays=look.verify_replays if look else 0, lookahead_replays=look.lookahead_replays if look else 0,
                     lookahead_hits=look.lookahead_hits if look else 0,
                     # depth 3: replays of that form, and how many of them decided a third iteration
                     lookahead_depth3_replays=look.depth3_replays if look else 0,
                     lookahead_third=look.lookahead_third if look else 0)
        return dict(**extra, acceptance_rate=acceptance_rate, tokens_per_s=self.n / seconds, tokens=self.emitted, n=self.n,
                    counts=self.counts, accepted=self.accepted_count, drafted=self.draft_count,
                    avg_tokens=acceptance_rate * self.gamma, resampled=self.resample_count,
                    bonus=self.target_sample_count, seconds=seconds, outer_steps=len(self.counts),
                    acc_rate_middle=float(np.mean(self.acc_rate_middle_list)) if self.acc_rate_middle_list else 0.0)


@torch.inference_mode()
def TriForce(tokenizer, graph_engine, input_ids, gamma=4, max_len=256, top_k=-1, top_p=0.9, temperature=0.6, verbose=False,
             file_path=None, dataset=None, spec_args=None, rng=None, return_details=False, rebuild_every=0, reanchor_at=0,
             logprobs=False, prompt_logprobs=False, min_p=0.0, repetition_penalty=1.0, frequency_penalty=0.0,
             presence_penalty=0.0):
    """``min_p`` > 0: min-p on the target tier.
    ``repetition_penalty`` / ``frequency_penalty`` / ``presence_penalty``: penalties on the target tier.
    ``logprobs`` / ``prompt_logprobs``: ``return_details`` then carries ``logprobs`` — a list aligned
    with ``tokens`` — and ``prompt_logprobs`` — an fp32 host tensor of n - 1 values."""
    run = TriForceRunner(tokenizer, graph_engine, gamma, top_k, top_p, temperature, verbose, rng,
                         rebuild_every=rebuild_every, reanchor_at=reanchor_at, logprobs=logprobs,
                         prompt_logprobs=prompt_logprobs, min_p=min_p, repetition_penalty=repetition_penalty,
                         frequency_penalty=frequency_penalty, presence_penalty=presence_penalty)
    run.prefill(input_ids)
    eng, device = run.eng, run.device
    _sync(device)
    time1 = time.time()
    while run.n < max_len:
        run.step()
    _sync(device)
    time2 = time.time()
    st = run.stats(time2 - time1)
    n, acceptance_rate, avg_tokens = st["n"], st["acceptance_rate"], st["avg_tokens"]
    if verbose:
        print(f"Use {time2 - time1} sec to generate {n} tokens (now {eng.kv_cache.seq_len} tokens), "
              f"Tokens/s: {n / (time2 - time1)}", flush=True)
        print(f"accepted rate {acceptance_rate}, avg generated tokens {avg_tokens}")
    if file_path is not None:
        header = "target,acceptance_rate,token/s,avg_tokens,prefill,gen_len,dataset,acc_rate_middle,latency\n"
        entry = (f"{eng.model.config._name_or_path},{acceptance_rate},{n / (time2 - time1)},{avg_tokens},"
                 f"{input_ids.shape[1]},{n},{dataset},{st['acc_rate_middle']},{(time2 - time1) / n}\n")
        if spec_args is not None:
            for k, v in spec_args.items():
                header = header.replace("\n", f",{k}\n")
                entry = entry.replace("\n", f",{v}\n")
        log_csv(file_path, header, entry)
    if return_details:
        return st
    return acceptance_rate, n / (time2 - time1)


class TriForceSession:
    """One long document, several answers: prefill once, then ``ask`` follow-up questions against the same document or
    take chat ``turn``s, each starting from the KV already on the device (TriForceRunner.extend).
    Every answer returns the runner's stats plus ``ttft`` — the seconds from the call to the first token of the answer."""

    def __init__(self, tokenizer, graph_engine, gamma=4, top_k=-1, top_p=0.9, temperature=0.6, verbose=False, rng=None,
                 rebuild_every=0, reanchor_at=0, logprobs=False, prompt_logprobs=False, min_p=0.0, repetition_penalty=1.0,
                 frequency_penalty=0.0, presence_penalty=0.0):
        self.run = TriForceRunner(tokenizer, graph_engine, gamma, top_k, top_p, temperature, verbose, rng,
                                  rebuild_every=rebuild_every, reanchor_at=reanchor_at, logprobs=logprobs,
                                  prompt_logprobs=prompt_logprobs, min_p=min_p, repetition_penalty=repetition_penalty,
                                  frequency_penalty=frequency_penalty, presence_penalty=presence_penalty)
        self.ttft = None

    @property
    def document(self):
        """Rows of the full cache that a follow-up question keeps by default: the region the retrieval cache was built over
        (re-anchoring moves ``prefill``, not this)."""
        rc = self.run.eng.graph_cache
        return getattr(rc, "prefill0", rc.prefill)

    def _first_token(self, fn, *a, **kw):
        device = self.run.device
        _sync(device)
        t0 = time.time()
        fn(*a, **kw)
        _sync(device)
        self.ttft = time.time() - t0

    def prefill(self, input_ids):
        self._first_token(self.run.prefill, input_ids)

    @torch.inference_mode()
    def generate(self, max_len=256):
        run = self.run
        _sync(run.device)
        t0 = time.time()
        while run.n < max_len:
            run.step()
        _sync(run.device)
        st = run.stats(time.time() - t0)
        st["ttft"] = self.ttft
        return st

    def ask(self, input_ids, max_len=256, keep=None):
        """A new question on the same document: the cache is rolled back to ``keep`` rows (default: the document)."""
        self._first_token(self.run.extend, input_ids, keep=self.document if keep is None else keep)
        return self.generate(max_len)

    def turn(self, input_ids, max_len=256):
        """A chat turn: everything generated so far stays in the context."""
        self._first_token(self.run.extend, input_ids, keep=None)
        return self.generate(max_len)


################### Dist Spec (TP + offloading) ####################
import types

import torch.distributed as dist


def _bcast_record(t):
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.broadcast(t, src=0)


# Who decides.  The reference broadcasts rank 0's samples and its accept draws (decoding.py:230-239, 345-346) because every
# rank draws from its own generator.  Here every rank holds the SAME uniform stream (same seed, explicit numbers) and, behind
# each exchange, bit-identical activations (every rank adds the same partials in the same order: csrc/allreduce.hip, the
# replicated lm_head and draft model do the rest), so every rank reaches rank 0's decision on its own — the path has no
# exchange step for decisions.  TRIFORCE_TP_REPLICATED_DECISIONS=1 runs TriForce_Dist / Middle_Spec_Dist that way (the autoregressive
# baseline and the tree loop keep their one broadcast per token / per level): no broadcast (two per inner
# iteration + one per outer step otherwise), and with the broadcasts the blocking device-to-host reads go — the records travel
# through the pinned mailbox like the single-GPU loop's.  A digest of the emitted stream is compared across the ranks every
# TRIFORCE_TP_REPLICA_CHECK_EVERY outer steps and when a loop ends (ReplicaCheck): a rank that left the common stream raises
# on every rank.  Default off: the broadcast form is the reference's, and neither form has met a second device yet.
# Round 6: the DEFAULT is "auto" — replicate when this group's forwards have been SHOWN bit-identical on every rank at start-up
# (DistributedLlama.replica_litmus: the retrieval forward with all its exchanges on a fixed probe, digests compared across
# the ranks), else broadcast.  "1" forces replicated, "0" forces the broadcast form (the reference's).  Evidence behind the
# default: tests/test_gpu_tp_offload.py — a two-process soak of 2 000+ tokens at T = 1.0 / top-p 0.95 in both exchange forms emits
# the broadcast form's stream on both ranks, and a rank whose uniform stream is knocked out of step fails LOUDLY (stream digest
# or exchange time-out) within the check interval instead of emitting another stream.
TP_REPLICATED_DECISIONS = __import__("os").environ.get("TRIFORCE_TP_REPLICATED_DECISIONS", "auto") == "1"      # (import-time view; see below)
TP_REPLICA_CHECK_EVERY = max(1, int(__import__("os").environ.get("TRIFORCE_TP_REPLICA_CHECK_EVERY", "32")))


def tp_decision_mode():
    v = __import__("os").environ.get("TRIFORCE_TP_REPLICATED_DECISIONS", "auto")
    return {"1": "replicated", "0": "broadcast"}.get(v, "auto")


def tp_sync_record(llm=None):
    """The `sync_record` of the tensor-parallel loops: rank 0's record broadcast, or None when the ranks replicate decisions.
    COLLECTIVE in "auto" mode the first time it sees an engine (the litmus runs one probe forward on every rank)."""
    mode = tp_decision_mode()
    if mode == "replicated":
        return None
    if mode == "broadcast" or llm is None:
        return _bcast_record
    base = getattr(llm, "llm", llm)                           # (a _DistEngine wraps the engine)
    ok = getattr(base, "replica_ok", None)
    if ok is None and hasattr(base, "replica_litmus"):
        ok = base.replica_litmus()
    return None if ok else _bcast_record


class ReplicaCheck:
    """Replicated decisions only: every rank folds the tokens it emitted into a 61-bit digest; every `every` outer steps
    (and on `force`) ONE 4-word MAX all-reduce of (digest, -digest, n, -n) tells every rank whether all ranks hold the same
    stream.  The call sites are functions of the outer step count alone, so ranks that agree meet in the collective; ranks whose
    forwards fell out of step never get here — their exchanges time out first (RuntimeError from `health`)."""

    MOD = (1 << 61) - 1

    def __init__(self, device, every=None):
        self.device, self.every = device, int(every or TP_REPLICA_CHECK_EVERY)
        self.seen = self.digest = self.checks = self.last_step = 0

    def fold(self, tokens):
        d = self.digest
        for t in tokens[self.seen:]:
            d = (d * 1_000_003 + int(t) + 1) % self.MOD
        self.digest, self.seen = d, len(tokens)

    def __call__(self, run, force=False):
        steps = len(run.counts)
        if not (force or steps - self.last_step >= self.every):
            return
        self.last_step = steps
        self.fold(run.emitted)
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        t = torch.tensor([self.digest, -self.digest, run.n, -run.n], dtype=torch.int64, device=self.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        hi, lo, n_hi, n_lo = t.tolist()
        self.checks += 1
        if hi != -lo or n_hi != -n_lo:
            raise RuntimeError(f"tensor-parallel ranks left the common token stream (rank {dist.get_rank()}: {run.n} tokens, digest "
                               f"{self.digest:#x}; across ranks n in [{-n_lo}, {n_hi}]): replicated decisions need identical "
                               "uniform streams and bit-identical exchanges — unset TRIFORCE_TP_REPLICATED_DECISIONS to broadcast rank 0's")


def sample_dist(probs, rng=None):
    """Rank 0 samples, everyone gets the token (reference decoding.py:230-239) — one 8-byte broadcast, no barrier."""
    tok = sample(probs, rng=rng)
    _bcast_record(tok)
    return tok


class _DistEngine:
    """Presents a DistributedLlama through the GraphInferenceEngine surface the decode loops drive."""

    def __init__(self, llm, logprobs=False, prompt_logprobs=False):
        if logprobs or prompt_logprobs:                # (refused before anything is captured: DESIGN section 23)
            raise NotImplementedError("logprobs / prompt_logprobs are implemented for the single-GPU resident "
                                      "GraphInferenceEngine only, not for _DistEngine (tensor-parallel loop)")
        self.llm = llm
        self._inner = {}
        self.sampling = dict(probs=True, temperature=llm.temperature, top_p=llm.top_p)

        def draft_run(input_ids, gamma_offset=0, probs=True, temperature=0.6, top_p=0.9):
            return llm._draft_run_eager(input_ids, gamma_offset, True, 0.6, 0.9)      # 0.6 / 0.9 hard-wired

        def model_verify(input_ids, position_ids, probs=True, temperature=None, top_p=None):
            # the retrieval-verify forward, issued eagerly (inside a capture: utils/graph_infer._InnerGraphs) — it reads the
            # shared token / position buffers itself; exchanges included, in the order of the whole-forward graph
            return llm._verify_cap["run_all"]()

        self.engine = types.SimpleNamespace(
            model=types.SimpleNamespace(device=llm.device, config=llm.config.model_config),
            kv_cache=llm.kv_cache, graph_cache=llm.retrieval_cache, draft_cache=llm.draft_cache, draft=getattr(llm, "draft", None),
            draft_run=draft_run, model_verify=model_verify)

    # -- round 6: the single-GPU loop's launch structure over the tensor-parallel engine's captured forwards ------------------
    # (what the loops look for on a graph engine: shared static inputs, replay-only draft steps, the one-graph inner iteration,
    #  a target verify that takes its ids as kernel arguments.  All of it needs whole-forward graphs — with segment graphs the
    #  exchanges run eagerly between the stages — and replicated decisions: a broadcast in the middle of an iteration cannot sit
    #  inside its graph.)
    def _whole(self):
        cap = getattr(self.llm, "_verify_cap", None)
        return cap is not None and cap.get("form") == "whole" and "run_all" in cap and bool(getattr(self.llm, "_draft_graphs", None))

    @property
    def tok_buf(self):
        return getattr(self.llm, "tok_buf", None) if self._whole() else None

    @property
    def pos_buf(self):
        return getattr(self.llm, "pos_buf", None) if self._whole() else None

    def replay_draft(self, gamma_offset):
        return self.llm.replay_draft(gamma_offset)

    def serves(self, filters):
        """The verify is normalised eagerly at whatever temperature and top-p it is handed; it has no top-k or min-p."""
        return not filters.target_only

    def verify_probs_ids(self, ids, temperature, top_p, top_k=-1, min_p=0.0):
        if not self.serves(Filters(temperature, top_p, top_k, min_p)):
            return None
        return self.llm.verify_probs_ids(ids, temperature, top_p)

    @torch.inference_mode()
    def inner_graphs(self, gamma, rng, record, capture=True):
        """The per-position inner-iteration graphs (graph_infer._InnerGraphs: draft step -> draw -> retrieval verify with its
        exchanges -> accept test, ONE hipGraph per position) over this engine; None when it cannot provide them."""
        import os
        from .graph_infer import _InnerGraphs
        tok = self.tok_buf
        if os.environ.get("TRIFORCE_INNER_GRAPH", "1") == "0" or tok is None or not tok.is_cuda or tok.shape[1] < gamma + 3 \
                or record.numel() < 4 or record.is_cuda or torch.cuda.is_current_stream_capturing():
            return None
        key = _InnerGraphs.key_of(self, gamma, rng, record)
        got = self._inner.get(key)
        if got is None and capture:
            if len(self._inner) >= 2:
                self._inner.pop(next(iter(self._inner)))
            got = self._inner[key] = _InnerGraphs(self, gamma, rng, record)
        return got

    @property
    def static_outputs(self):
        """The captured draft / retrieval-verify forwards can hand out their static output buffers (valid until the same graph
        replays again — what the decode loops need: no 0.9 MB clone and no per-position row copies per inner iteration)."""
        return getattr(self.llm, "_verify_cap", None) is not None and bool(getattr(self.llm, "_draft_graphs", None))

    def graph_draft_inference(self, input_ids, gamma_offset=0, clone=True):
        return self.llm.draft_run(input_ids=input_ids, gamma_offset=gamma_offset, clone=clone)   # 0.6/0.9 hard-wired

    def graph_verify(self, input_ids, position_ids, clone=True):
        return self.llm.retrieval_verify(input_ids=input_ids, position_ids=position_ids,
                                         temperature=self.llm.temperature, top_p=self.llm.top_p, clone=clone)

    def verify_generation(self):
        if getattr(self.llm, "_verify_cap", None) is None:
            return None
        return getattr(self.llm, "_verify_gen", 0) + sum(g.generation for g in self._inner.values())

    def inference(self, input_ids, eager=False):
        return self.llm.inference(input_ids=input_ids, eager=eager)

    def update_graph_cache(self):
        self.llm.retrieval_cache.update_graph_cache(self.llm.kv_cache)

    def health(self):
        check = getattr(self.llm, "check_exchange", None)
        if check is not None:
            check("decode step")


@torch.inference_mode()
def Baseline_Dist(tokenizer, graph_engine, input_ids, max_len=256, top_k=-1, top_p=0.9, temperature=0.6, verbose=False,
                  local_rank=0, rng=None, logprobs=False):
    """Autoregressive TP baseline (reference decoding.py:243-287): returns (ms per token, generated ids)."""
    if logprobs:
        raise NotImplementedError("logprobs is implemented for the single-GPU resident GraphInferenceEngine only, not for "
                                  "Baseline_Dist (tensor-parallel loop)")
    llm = graph_engine
    rng = rng or UniformSource(llm.device, seed=1)
    kw = Filters(temperature, top_p, top_k).kw()
    llm.reset()
    logits = llm.prefill(input_ids=input_ids)
    next_token = sample_dist(norm_logits(logits[:, -1, :], **kw), rng)
    gen_tokens = torch.zeros((input_ids.size(0), max_len), dtype=torch.long, device=input_ids.device)
    n = 0
    check = getattr(llm, "check_exchange", None)
    _sync(llm.device)
    time1 = time.time()
    while n < max_len:
        logits = llm.inference(input_ids=next_token)
        next_token = sample_dist(norm_logits(logits[:, -1, :], **kw), rng)
        gen_tokens[:, n] = next_token.squeeze()
        n += 1
        if check is not None and n % 32 == 0:          # a timed-out exchange NaN-fills its outputs: stop, don't emit
            check("autoregressive step")
    _sync(llm.device)
    time2 = time.time()
    if check is not None:
        check("autoregressive loop")
    return 1000 * (time2 - time1) / n, gen_tokens


@torch.inference_mode()
def Middle_Spec_Dist(next_token, llm, gamma, verbose, tokenizer, rng=None):
    """Reference decoding.py:432-495."""
    ge = llm if isinstance(llm, _DistEngine) else _DistEngine(llm)
    sync = tp_sync_record(ge)
    if sync is None and rng is None:
        # replicated decisions: every rank must hold the SAME uniform stream — an unseeded one differs per rank and the ranks
        # would drift apart silently (in the broadcast form rank 0's draw is everyone's, so None did no harm there).  One
        # seeded stream per engine, continued across calls (advisor, round 5).
        base = ge.llm
        rng = getattr(base, "_replicated_rng", None)
        if rng is None:
            rng = base._replicated_rng = UniformSource(base.device, seed=1)
    return Middle_Spec(next_token, ge, gamma, verbose, tokenizer, rng=rng, sync_record=sync)


@torch.inference_mode()
def TriForce_Dist(tokenizer, llm, input_ids, gamma=4, max_len=256, top_k=-1, top_p=0.9, temperature=0.6, verbose=False,
                  file_path=None, dataset=None, spec_args=None, rng=None, return_details=False, logprobs=False,
                  prompt_logprobs=False):
    """Reference decoding.py:291-428: returns (avg accepted tokens, seconds per token)."""
    if logprobs or prompt_logprobs:                    # (refused before the engine wrapper or anything else is built)
        raise NotImplementedError("logprobs / prompt_logprobs are implemented for the single-GPU resident "
                                  "GraphInferenceEngine only, not for TriForce_Dist (tensor-parallel loop)")
    ge = _DistEngine(llm)
    rng = rng or UniformSource(llm.device, seed=1)          # same seed on every rank: identical uniform streams
    run = TriForceRunner(tokenizer, ge, gamma, top_k, top_p, temperature, verbose, rng, inclusive_accept=True,
                         sync_record=tp_sync_record(llm))
    run.health = ge.health
    replicas = ReplicaCheck(llm.device) if run.sync_record is None else None
    llm.reset()
    if input_ids.shape[1] != llm.prefill_len:
        # the retrieval cache's chunk grid and the device mirror of the generated rows are laid out for exactly this
        # prompt length (the entry scripts clip / generate prompts to --prefill)
        raise ValueError(f"prompt length {input_ids.shape[1]} != the engine's prefill length {llm.prefill_len}")
    llm.prefill(input_ids=input_ids[:, :-1])
    logits = llm.build_retrieval_cache(input_ids=input_ids[:, -1:])
    info = getattr(llm.weights, "aligned", None)
    if info is not None and "calibration" not in info:        # aligned synthetic weights: one-off read-out calibration
        from ..models import aligned
        aligned.calibrate_llm(llm, gamma, temperature, top_p)
    run.start(logits)
    llm.draft_run(input_ids=input_ids)
    eos = run.eos
    _sync(llm.device)
    time1 = time.time()
    knock = __import__("os").environ.get("TF_TEST_TP_KNOCK_RANK_AT")       # tests only: "rank,step" — that rank skips one uniform there
    while run.n < max_len:
        if knock and [llm.local_rank, len(run.counts)] == [int(x) for x in knock.split(",")]:
            rng.advance(1)
        run.step()
        if replicas is not None:
            replicas(run)
        # the TP loop stops when the token that closed the accept scan — accepted or resampled — is eos
        # (decoding.py:382-383); a bonus token is sampled after that check and never ends the loop
        if run.next_token == eos and run.last_reason != 1:
            break
    if replicas is not None:
        replicas(run, force=True)
    _sync(llm.device)
    time2 = time.time()
    st = run.stats(time2 - time1)
    st["decisions"] = "broadcast" if replicas is None else "replicated"
    st["replica_checks"] = 0 if replicas is None else replicas.checks
    st["inner_graphs"] = run.inner is not None           # one hipGraph per inner iteration (whole-forward graphs + replicated decisions)
    if return_details:
        return st
    return st["avg_tokens"], (time2 - time1) / max(run.n, 1)
