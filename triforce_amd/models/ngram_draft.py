"""Prompt-lookup n-gram draft tier: the bottom tier without a checkpoint.  ``NgramDraft`` stands where the
68M model stands in ``InferenceEngine(model, cache, graph_cache, draft, draft_cache)`` and ``NgramCache`` where its
StreamingLLM cache stands; the decode loops, the draw and the accept kernels are the 68M tier's, called exactly as for it.

The proposal is the token that followed the most recent, longest earlier occurrence of the context's last ``ngram_max``
tokens (include/triforce_hip.h "N-GRAM DRAFT"); the draft distribution is the point mass on it, so the draw returns it for
every u in [0, 1) and the accept test min(1, p[d] / q[d]) is u < p[d].
"""
import types

import torch

from .. import ops
from .llama_core import CausalLMOutput

DRAFT_NAME = "ngram"           # what --draft names this tier


def refuse_ngram_draft(draft, what):
    """The engines that drive their draft tier some other way (tensor-parallel, Sequoia, offloading) refuse this one by name."""
    if isinstance(draft, NgramDraft) or draft == DRAFT_NAME:
        raise NotImplementedError(f"--draft {DRAFT_NAME} (the prompt-lookup n-gram draft tier, DESIGN section 32) is implemented "
                                  f"for the single-GPU resident GraphInferenceEngine only, not for {what}")


class NgramCache:
    """The token history the n-gram draft looks matches up in: ``hist`` (cap,) int32 and ``len_dev`` int32 scalar on the
    device, ``length`` its host mirror.

    State invariant (asserted by tests/test_ngram_draft_cpu.py and tests/test_gpu_ngram_draft.py): at the start of every
    Middle_Spec, hist[0:L] holds exactly the tokens whose rows are in the full KV cache — ``TriForceRunner.history`` followed
    by ``TriForceRunner._fed`` on the host — and the shared token buffer's tok_buf[0:n + 1] continues them.  The history is
    only ever SET (prefill, extend's re-prefill) or APPENDED with confirmed tokens (TriForceRunner.step, one ngram_commit at
    the point where the penalty counts are committed), so there is no rollback.

    It has the surface the loops use of StreamingLLMEvictionCache; the eviction calls are no-ops (nothing is evicted: a
    history entry is four bytes)."""

    start_size = recent_size = 0

    def __init__(self, cap, device, gamma=6):
        self.cap, self.device, self.gamma = int(cap), torch.device(device), gamma
        assert self.cap >= 1
        self.hist = torch.zeros(self.cap, dtype=torch.int32, device=self.device)
        self.len_dev = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.length = 0

    @property
    def seq_len(self):
        return self.length

    @seq_len.setter
    def seq_len(self, value):
        # (extend() writes 0 behind reset(), as it must for the StreamingLLM cache)
        if int(value) != self.length:
            raise ValueError(f"NgramCache holds {self.length} tokens; its length changes through reset / set / commit only")

    def reset(self):
        self.len_dev.zero_()
        self.length = 0

    def set(self, input_ids):
        """The history becomes ``input_ids`` (any shape, int64): once per prompt / per extend(), plain torch copies."""
        ids = torch.as_tensor(input_ids, device=self.device).reshape(-1)
        n = ids.numel()
        if n > self.cap:
            raise IndexError(f"NgramCache overflow: {n} > {self.cap}")
        self.hist[:n].copy_(ids.to(torch.int32))
        self.len_dev.fill_(n)
        self.length = n

    def commit(self, src, n):
        """Append the first ``n`` (<= 64) entries of the int64 device row ``src``: one launch, no host read."""
        n = int(n)
        if self.length + n > self.cap:
            raise IndexError(f"NgramCache overflow: {self.length}+{n} > {self.cap}")
        ops.ngram_commit(self.hist, self.len_dev, src, n)
        self.length += n

    def tokens(self):
        """hist[0:L] as a python list (a device read: tests and debugging)."""
        L = int(self.len_dev.item())
        return self.hist[:L].tolist()

    def evict_prefill(self, incoming):
        pass

    def evict_for_spec(self, current_seq_len):
        pass

    def print_status(self):
        print("[N-gram Cache] Capacity:", self.cap, "| Cached:", self.length)


class NgramDraft:
    """``forward(input_ids, cache, cache, gamma_offset, probs=...)`` -> an output whose ``.probs`` is the static one-hot row of
    that ``gamma_offset`` (one row per offset: the lookahead graphs keep the rows of several draft steps alive at once).  There
    are no logits: ``probs=None`` is refused."""

    def __init__(self, vocab_size, device, ngram_max=3):
        self.vocab_size, self.device, self.ngram_max = int(vocab_size), torch.device(device), int(ngram_max)
        if not 1 <= self.ngram_max <= ops.NGRAM_MAX_N:
            raise ValueError(f"ngram_max={ngram_max} is outside [1, {ops.NGRAM_MAX_N}]")
        self.config = types.SimpleNamespace(vocab_size=self.vocab_size, _name_or_path=f"{DRAFT_NAME}-{self.ngram_max}")
        self.dtype = torch.float32
        self._rows, self._info = {}, {}
        self._ws = ops.ngram_workspace(self.device) if self.device.type == "cuda" else None

    def eval(self):
        return self

    def row(self, gamma_offset):
        """The static (V,) fp32 row and (4,) int32 info of a draft step; allocated at the first use, which a capture's warm-up
        passes make outside the capture."""
        if gamma_offset not in self._rows:
            assert self.device.type != "cuda" or not torch.cuda.is_current_stream_capturing(), \
                "the n-gram draft's rows are allocated by the warm-up passes, never inside a capture"
            self._rows[gamma_offset] = torch.zeros(self.vocab_size, dtype=torch.float32, device=self.device)
            self._info[gamma_offset] = torch.zeros(4, dtype=torch.int32, device=self.device)
        return self._rows[gamma_offset], self._info[gamma_offset]

    def set_history(self, input_ids, cache):
        """What the 68M's chunked prefill is for this tier: the whole token history in one copy."""
        cache.set(input_ids)

    @torch.inference_mode()
    def __call__(self, input_ids, kv_cache=None, graph_cache=None, position_ids=None, gamma_offset=-1, attention_mask=None,
                 storage_ids=None):
        return self.forward(input_ids, kv_cache, graph_cache, gamma_offset)

    def forward(self, input_ids, kv_cache, graph_cache=None, gamma_offset=-1, probs=None):
        if probs is None:
            raise NotImplementedError("the n-gram draft has no logits: its forward returns the one-hot probability row only "
                                      "(initialise the engine with probs=True)")
        cache = graph_cache if graph_cache is not None else kv_cache
        if gamma_offset < 0 or not isinstance(cache, NgramCache):
            raise NotImplementedError("the n-gram draft runs speculative steps (gamma_offset >= 0) over an NgramCache; a "
                                      "prompt is handed over with set_history")
        blk = input_ids.reshape(-1)
        assert blk.numel() == gamma_offset + 1 <= ops.NGRAM_MAX_BLOCK
        q, info = self.row(gamma_offset)
        ops.ngram_draft(cache.hist, cache.len_dev, blk, self.ngram_max, self.vocab_size, q=q, info=info, ws=self._ws)
        return CausalLMOutput(None, q)
