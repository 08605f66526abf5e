"""KV caches of the TriForce path — host-side mirror of the reference's models/cache.py
(FlashSimpleCache :20-61, RetrievalCache :117-198, StreamingLLMEvictionCache :200-265) with the
same constructors, attributes and methods, backed by HIP kernels.

Physical layout is HEAD-MAJOR ``[L][H][T][D]`` fp16 (``.k`` / ``.v``): one head's keys are
contiguous, so a split-KV wavefront streams one contiguous 256-B-per-key segment and the retrieval
scorer reads whole 2-KiB chunks.  ``key_cache`` / ``value_cache`` keep the reference's shape
``[L, 1, T, H, D]`` as permuted views of the same storage (nothing outside models/ indexes them,
SURVEY §8b B3).

Reference quirks kept on purpose: RetrievalCache.reset() does not clear
``init_graph``; StreamingLLMEvictionCache.reset() does not reset ``seq_len``.
"""
import os
from typing import Tuple

import torch

from .. import ops

# TRIFORCE_KV_CACHE: storage of the target's full KV cache (FlashSimpleCache).  "fp16" (default) or "fp8": OCP e4m3fn codes with
# one exponent byte per (layer, head, token) row (include/triforce_hip.h "FP8 KV CACHE").  With fp8 the
# decoding stays lossless with respect to the target whose attention reads the dequantized K / V, not the fp16 model.
KV_CACHE_ENV = "TRIFORCE_KV_CACHE"


def kv_cache_dtype(override=None):
    """"fp16" or "fp8": ``override`` if given, else TRIFORCE_KV_CACHE.  fp8 needs the fused decode layer (TRIFORCE_FUSE=all)."""
    return ops.fp16_or_fp8(KV_CACHE_ENV, override, "the FP8 attention exists only in that form")


# TRIFORCE_RETRIEVAL_INDEX=1: RetrievalCache keeps the fp16 chunk means of the covered region (csrc/retrieval.hip "chunk-mean
# index"): a rebuild scores from them instead of re-reading K.  Off by default: nothing is allocated.
RETRIEVAL_INDEX_ENV = "TRIFORCE_RETRIEVAL_INDEX"
TOPK_MAX_CHUNKS = 32768                               # tf_retrieval_topk's limit on the chunk count


def retrieval_index(override=None):
    """Whether RetrievalCache keeps a chunk-mean index: ``override`` if given, else TRIFORCE_RETRIEVAL_INDEX."""
    if override is not None:
        return bool(override)
    v = os.environ.get(RETRIEVAL_INDEX_ENV, "0").strip().lower() or "0"
    if v not in ("0", "1"):
        raise ValueError(f"{RETRIEVAL_INDEX_ENV}={v!r}: expected 0 or 1")
    return v == "1"


# TRIFORCE_RETRIEVAL_KV: storage of the retrieval cache's rows [0, max_budget) (RetrievalCache).  "fp16" (default) or "fp8": the
# row format of TRIFORCE_KV_CACHE=fp8, codes + one exponent byte per row (include/triforce_hip.h "FP8 RETRIEVAL CACHE", DESIGN
# section 21).  The retrieval cache only drafts, so the decoding stays lossless with respect to the target either way.
RETRIEVAL_KV_ENV = "TRIFORCE_RETRIEVAL_KV"


def retrieval_kv_dtype(override=None):
    """"fp16" or "fp8": ``override`` if given, else TRIFORCE_RETRIEVAL_KV.  fp8 needs the fused decode layer (TRIFORCE_FUSE=all)."""
    return ops.fp16_or_fp8(RETRIEVAL_KV_ENV, override, "the attention over codes + fp16 spec rows exists only in that form")


def _refuse_tier(dtype, env, home, what):
    """The caches without an FP8 form: refuse the knob instead of ignoring it.  ``home``: the one cache that implements it."""
    if dtype() == "fp8":
        raise NotImplementedError(f"{env}=fp8 is implemented for the single-GPU {home} only, not for {what}")


def _refuse_retrieval_fp8(what):
    _refuse_tier(retrieval_kv_dtype, RETRIEVAL_KV_ENV, "retrieval cache (RetrievalCache)", what)


def _refuse_fp8(what):
    _refuse_tier(kv_cache_dtype, KV_CACHE_ENV, "resident cache (FlashSimpleCache)", what)


class Cache:
    """Base class (reference models/cache.py:6-17)."""

    fp8 = False                                       # True: the rows are FP8 codes (CodedRows), there is no .k / .v

    def update(self, key_states, value_states, layer_idx) -> Tuple[torch.Tensor, torch.Tensor]:
        raise NotImplementedError("Make sure to implement `update` in a subclass.")


def _refuse_gqa(cfg, what):
    from .config_yarn import refuse_gqa
    refuse_gqa(cfg, what)


def _geom(model):
    cfg = model.config
    heads = cfg.num_key_value_heads
    return cfg.num_hidden_layers, heads, cfg.hidden_size // cfg.num_attention_heads


def _alloc(L, H, T, D, device):
    k = torch.zeros(L, H, T, D, dtype=torch.float16, device=device)
    v = torch.zeros(L, H, T, D, dtype=torch.float16, device=device)
    return k, v


def _ref_view(t):
    # (L,H,T,D) storage -> the reference's [L,1,T,H,D] shape
    return t.permute(0, 2, 1, 3).unsqueeze(1)


def _rows(x):
    # accepts the reference's (1,n,H,D) or (n,H,D); returns (n,H,D)
    return x[0] if x.dim() == 4 else x


class CodedRows:
    """K / V rows in the FP8 row format (include/triforce_hip.h "FP8 KV CACHE"), the one place that spells it out: e4m3fn codes
    ``kc`` / ``vc`` [L][H][T][D] and one exponent byte per row ``ke`` / ``ve`` [L][H][T]; an empty row is zero codes under
    the smallest exponent.  The caches that hold one bind the four tensors under the same names."""

    def __init__(self, L, H, T, D, device, knob):
        if D != 128:                                  # the kernels over codes exist for this width only
            raise NotImplementedError(f"{knob}=fp8 needs head_dim 128 (got {D}): the FP8 row format and its attention are "
                                      "built for that width")
        self.kc = torch.zeros(L, H, T, D, dtype=torch.float8_e4m3fn, device=device)
        self.vc = torch.zeros(L, H, T, D, dtype=torch.float8_e4m3fn, device=device)
        self.ke = torch.full((L, H, T), ops.KV_FP8_EMIN + 127, dtype=torch.uint8, device=device)
        self.ve = torch.full((L, H, T), ops.KV_FP8_EMIN + 127, dtype=torch.uint8, device=device)

    def nbytes(self):
        return self.kc.nbytes + self.vc.nbytes + self.ke.nbytes + self.ve.nbytes

    def reset(self):
        for codes, exp in ((self.kc, self.ke), (self.vc, self.ve)):
            codes.view(torch.uint8).zero_()
            exp.fill_(ops.KV_FP8_EMIN + 127)

    def layer(self, i):
        """(k codes, v codes, k exponents, v exponents) views of layer ``i``, (H,T,D) and (H,T); of a slice of layers (the
        same indexing under the name ``layers``), (n,H,T,D) and (n,H,T)."""
        return self.kc[i], self.vc[i], self.ke[i], self.ve[i]

    layers = layer

    def dequant_into(self, layers, k_out, v_out, src_t0, dst_t0, n):
        """Rows [dst_t0, dst_t0 + n) of the fp16 views k_out / v_out (n layers,H,T',D) = deq of rows [src_t0, src_t0 + n)."""
        ops.kv_dequant_rows_pair(*self.layers(layers), k_out, v_out, src_t0, dst_t0, n)


def _refuse_k_v(cls, knob, use):
    """The __getattr__ of a cache class that may hold codes (only reached for missing attributes): .k / .v of an FP8 cache, fp16
    storage that does not exist, get an explanation instead of a bare name."""
    def __getattr__(self, name):
        if name in ("k", "v") and self.fp8:
            raise AttributeError(f"{cls}.{name}: the cache holds FP8 codes ({knob}=fp8), there is no fp16 storage to index; "
                                 f"use {use} or dequantize(layer)")
        raise AttributeError(name)
    return __getattr__


def _hold_coded_rows(cache, T, knob):
    """Give ``cache`` a CodedRows of T rows per head as ``coded``, the store's tensors under their own names (plain attributes:
    the forward reads them every layer), the reference-shaped views of the codes, and ``fp8``."""
    c = cache.coded = CodedRows(cache.layers, cache.num_heads, T, cache.head_dim, cache.device, knob)
    cache.kc, cache.vc, cache.ke, cache.ve = c.kc, c.vc, c.ke, c.ve
    cache.key_cache, cache.value_cache = _ref_view(c.kc), _ref_view(c.vc)
    cache.fp8 = True


class FlashSimpleCache(Cache):
    """Full KV cache of the target model (reference cache.py:20-61).

    ``kv_dtype`` (None: TRIFORCE_KV_CACHE) = "fp8" stores e4m3fn codes ``kc`` / ``vc`` [L][H][T][D] with exponent bytes ``ke`` /
    ``ve`` [L][H][T]; ``.k`` / ``.v`` do not exist then.  Fresh decode-sized rows pass through the fp16 staging ``stage_k`` /
    ``stage_v`` [H][32][D]; prefill chunks and the retrieval build read one dequantized layer in ``scratch_k`` / ``scratch_v``
    [H][T][D]."""

    def __init__(self, model, max_budget=1024, kv_dtype=None) -> None:
        self.seq_len = 0
        self.max_budget = max_budget
        self.layers, self.num_heads, self.head_dim = _geom(model)
        self.hidden_size = model.config.hidden_size
        self.device = model.device
        self.scores = []
        if kv_cache_dtype(kv_dtype) == "fp8":
            _refuse_gqa(model.config, f"{KV_CACHE_ENV}=fp8 (the FP8 KV cache)")
            H, T, D = self.num_heads, max_budget, self.head_dim
            _hold_coded_rows(self, T, KV_CACHE_ENV)
            self.stage_k = torch.zeros(H, ops.SKINNY_MAX_ROWS, D, dtype=torch.float16, device=self.device)
            self.stage_v = torch.zeros(H, ops.SKINNY_MAX_ROWS, D, dtype=torch.float16, device=self.device)
            self.scratch_k = torch.zeros(H, T, D, dtype=torch.float16, device=self.device)
            self.scratch_v = torch.zeros(H, T, D, dtype=torch.float16, device=self.device)
            return
        self.k, self.v = _alloc(self.layers, self.num_heads, max_budget, self.head_dim, self.device)
        self.key_cache, self.value_cache = _ref_view(self.k), _ref_view(self.v)

    __getattr__ = _refuse_k_v("FlashSimpleCache", KV_CACHE_ENV, "kc / vc / ke / ve")

    def nbytes(self):
        """Device bytes of the cache storage (FP8: codes, exponents, staging and layer scratch)."""
        if not self.fp8:
            return self.k.nbytes + self.v.nbytes
        return self.coded.nbytes() + sum(t.nbytes for t in (self.stage_k, self.stage_v, self.scratch_k, self.scratch_v))

    def dequantize(self, layer, rows=None):
        """(k, v): fresh (H, rows, D) fp16 tensors of deq(K), deq(V) of ``layer``, rows [0, rows) (default seq_len)."""
        n = self.seq_len if rows is None else rows
        if not self.fp8:
            return self.k[layer, :, :n].clone(), self.v[layer, :, :n].clone()
        H, D = self.num_heads, self.head_dim
        k = torch.empty(1, H, n, D, dtype=torch.float16, device=self.device)
        v = torch.empty_like(k)
        self.coded.dequant_into(slice(layer, layer + 1), k, v, 0, 0, n)
        return k[0], v[0]

    def scratch_layer(self, layer, rows):
        """FP8: dequantize rows [0, rows) of ``layer`` into the layer scratch and return its (H,T,D) views."""
        self.coded.dequant_into(slice(layer, layer + 1), self.scratch_k.unsqueeze(0), self.scratch_v.unsqueeze(0), 0, 0, rows)
        return self.scratch_k, self.scratch_v

    def layer_codes(self, layer):
        """FP8: (k codes, v codes, k exponents, v exponents) of ``layer``: (H,T,D) and (H,T) views."""
        return self.coded.layer(layer)

    def print_status(self):
        print("[Full Cache] Cached:", self.seq_len, "| Budget:", self.max_budget)

    def reset(self):
        self.seq_len = 0
        if self.fp8:
            self.coded.reset()
            return
        self.k.zero_()
        self.v.zero_()

    def layer_kv(self, layer_idx):
        if self.fp8:                                  # fp16 views of the layer: its rows [0, seq_len) dequantized into the scratch
            return self.scratch_layer(layer_idx, self.seq_len)
        return self.k[layer_idx], self.v[layer_idx]

    def tail_source(self, layers, prefill):
        """(k, v, first_row, exp) holding the generated-token rows [prefill, seq_len) of `layers` on the device: fp16 rows and
        ``exp`` None, or codes and ``exp`` = their (k, v) exponent bytes."""
        if self.fp8:
            return self.kc[layers], self.vc[layers], prefill, (self.ke[layers], self.ve[layers])
        return self.k[layers], self.v[layers], prefill, None

    def append_slot(self, layer_idx, n):
        """Slot where the fused RoPE+append kernel writes this layer's n new rows; seq_len advances
        after the last layer exactly like update() (cache.py:58-59)."""
        if self.seq_len + n > self.max_budget:
            raise IndexError(f"FlashSimpleCache overflow: {self.seq_len}+{n} > {self.max_budget}")
        slot = self.seq_len
        if layer_idx == self.layers - 1:
            self.seq_len += n
        return slot

    def update(self, key_states, value_states, layer_idx):
        k, v = _rows(key_states), _rows(value_states)
        n = k.shape[0]
        s = self.seq_len
        if self.fp8:                                  # quantize, return deq of rows [0, s + n) in the reference's shape
            kr, vr = k.permute(1, 0, 2).contiguous(), v.permute(1, 0, 2).contiguous()
            ops.kv_quant_rows(kr, vr, *self.layer_codes(layer_idx), s)
            kd, vd = self.dequantize(layer_idx, s + n)
            if layer_idx == self.layers - 1:
                self.seq_len += n
            return kd.permute(1, 0, 2).unsqueeze(0), vd.permute(1, 0, 2).unsqueeze(0)
        self.k[layer_idx, :, s:s + n] = k.permute(1, 0, 2)
        self.v[layer_idx, :, s:s + n] = v.permute(1, 0, 2)
        key = self.key_cache[layer_idx][:, :s + n]
        value = self.value_cache[layer_idx][:, :s + n]
        if layer_idx == self.layers - 1:
            self.seq_len += n
        return key, value


class OffloadingFlashSimpleCache(Cache):
    """Single-GPU offloading cache (reference cache.py:63-115, entry point test/offloading.py): the whole KV
    lives in pinned host memory and every target forward streams it layer by layer through two device buffers.

    The reference does this synchronously (`.cpu()` of the new rows, then a full-layer H2D on the compute stream,
    :98-104).  Here the live tokens of layer i+1 are prefetched on a copy stream (tf_kv_h2d_async) while layer i
    computes, the new rows go back with tf_kv_d2h_async, and a small device mirror of the generated-token rows
    serves RetrievalCache.update_graph_cache without touching host memory."""

    def __init__(self, model, max_budget=1024, tail_capacity=None) -> None:
        _refuse_fp8("OffloadingFlashSimpleCache")
        _refuse_gqa(model.config, "the offloading cache (OffloadingFlashSimpleCache)")
        self.seq_len = 0
        self.max_budget = max_budget
        self.layers, self.num_heads, self.head_dim = _geom(model)
        self.hidden_size = model.config.hidden_size
        self.device = model.device
        L, H, T, D = self.layers, self.num_heads, max_budget, self.head_dim
        self.cpu_k = _pinned_zeros(L, H, T, D)
        self.cpu_v = _pinned_zeros(L, H, T, D)
        self.key_cache, self.value_cache = _ref_view(self.cpu_k), _ref_view(self.cpu_v)
        self.buf_k = [torch.zeros(H, T, D, dtype=torch.float16, device=self.device) for _ in range(2)]
        self.buf_v = [torch.zeros(H, T, D, dtype=torch.float16, device=self.device) for _ in range(2)]
        self.key_cache_buffer, self.value_cache_buffer = self.buf_k[0], self.buf_v[0]
        self.load_stream = torch.cuda.Stream(device=self.device)
        self.tail_base = None                       # first token row mirrored in tail_k/v (= prefill length)
        self.tail_capacity = tail_capacity
        self.tail_k = self.tail_v = None
        self._ready = {}

    def print_status(self):
        print("[Offloading Flash Simple Cache] Cached Size:", self.seq_len, "| Budget:", self.max_budget)

    def reset(self):
        self.seq_len = 0
        self.cpu_k.zero_()
        self.cpu_v.zero_()

    def set_tail(self, base, capacity):
        """Mirror rows [base, base+capacity) (the generated tokens) on the device as they are produced."""
        self.tail_base = base
        if self.tail_k is None or self.tail_k.shape[2] < capacity:
            self.tail_k, self.tail_v = _alloc(self.layers, self.num_heads, capacity, self.head_dim, self.device)

    def tail_source(self, layers, prefill):
        assert self.tail_base == prefill, "OffloadingFlashSimpleCache.set_tail(prefill, capacity) must be called first"
        return self.tail_k[layers], self.tail_v[layers], 0, None

    # -- streaming protocol driven by the model forward ---------------------------------------
    def _fetch(self, layer_idx):
        b = layer_idx % 2
        ops.kv_h2d_async(self.buf_k[b], self.cpu_k[layer_idx], self.seq_len, self.load_stream)
        ops.kv_h2d_async(self.buf_v[b], self.cpu_v[layer_idx], self.seq_len, self.load_stream)
        ev = torch.cuda.Event()
        ev.record(self.load_stream)
        self._ready[layer_idx] = ev

    def begin_forward(self):
        self.load_stream.wait_stream(torch.cuda.current_stream(self.device))
        self._ready = {}
        for i in range(min(2, self.layers)):
            self._fetch(i)

    def layer_kv(self, layer_idx):
        torch.cuda.current_stream(self.device).wait_event(self._ready[layer_idx])
        b = layer_idx % 2
        return self.buf_k[b], self.buf_v[b]

    def append_slot(self, layer_idx, n):
        if self.seq_len + n > self.max_budget:
            raise IndexError(f"OffloadingFlashSimpleCache overflow: {self.seq_len}+{n} > {self.max_budget}")
        return self.seq_len                          # seq_len advances in end_forward (every layer sees the same slot)

    def layer_done(self, layer_idx, slot, n):
        b = layer_idx % 2
        if self.tail_base is not None and slot >= self.tail_base:
            ops.kv_copy_rows_pair(self.buf_k[b].unsqueeze(0), self.buf_v[b].unsqueeze(0), self.tail_k[layer_idx:layer_idx + 1],
                                  self.tail_v[layer_idx:layer_idx + 1], slot, slot - self.tail_base, n)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self.device))
        self.load_stream.wait_event(done)
        ops.kv_d2h_async(self.cpu_k[layer_idx], self.buf_k[b], slot, n, self.load_stream)
        ops.kv_d2h_async(self.cpu_v[layer_idx], self.buf_v[b], slot, n, self.load_stream)
        if layer_idx + 2 < self.layers:
            self._fetch(layer_idx + 2)
        self._pending = n

    def end_forward(self):
        torch.cuda.current_stream(self.device).wait_stream(self.load_stream)
        self.seq_len += getattr(self, "_pending", 0)
        self._pending = 0


class RetrievalCache(Cache):
    """Per-head retrieval cache (reference cache.py:117-198): chunk-mean scoring, top-k, gather.

    ``prefill`` — the rows [0, prefill) the selection covers — can be moved after construction with ``reanchor``
    (``prefill0`` keeps the constructor's value).  ``index`` (None: TRIFORCE_RETRIEVAL_INDEX) keeps the chunk means of the
    covered region in ``index`` [L][H][Cmax][D] fp16, Cmax = the full cache's capacity // chunk_size, allocated at the first
    build; ``indexed_chunks[layer]`` chunks of it are valid, and a build computes only the missing ones.

    ``kv_dtype`` (None: TRIFORCE_RETRIEVAL_KV) = "fp8" stores rows [0, max_budget) as e4m3fn codes ``kc`` / ``vc``
    [L][H][max_budget][D] with exponent bytes ``ke`` / ``ve`` [L][H][max_budget] (gathered and refreshed as codes: copied from
    an FP8 full cache, quantized from an fp16 one); the gamma + 1 rows of a spec forward stay fp16 in ``spec_k`` / ``spec_v``
    [L][H][gamma + 1][D]; ``.k`` / ``.v`` do not exist then."""

    _tail_plan = None                                 # (source key, launch plan, source first row) of the per-step refresh

    def __init__(self, model, max_budget=1024, prefill=1024, chunk_size=8, gamma=6, index=None, kv_dtype=None) -> None:
        self.chunk_size = chunk_size
        self.prefill = self.prefill0 = prefill
        self.chunks = prefill // self.chunk_size
        self.select_sets = max_budget // self.chunk_size
        self.gamma = gamma
        self.max_budget = max_budget
        assert prefill % self.chunk_size == 0, f"prefill should be multiple of chunk_size, got {prefill} % {self.chunk_size}"
        assert max_budget % self.chunk_size == 0, f"max_budget should be multiple of chunk_size, got {max_budget} % {self.chunk_size}"
        self.real_budget = max_budget + gamma + 1
        self.layers, self.num_heads, self.head_dim = _geom(model)
        self.hidden_size = model.config.hidden_size
        self.device = model.device
        self.q_heads = model.config.num_attention_heads       # > num_heads: grouped-query, selection per KV head
        if retrieval_kv_dtype(kv_dtype) == "fp8":
            _refuse_gqa(model.config, f"{RETRIEVAL_KV_ENV}=fp8 (the FP8 retrieval cache)")
            _hold_coded_rows(self, max_budget, RETRIEVAL_KV_ENV)
            self.spec_k, self.spec_v = _alloc(self.layers, self.num_heads, gamma + 1, self.head_dim, self.device)
        else:
            self.k, self.v = _alloc(self.layers, self.num_heads, self.real_budget, self.head_dim, self.device)
            self.key_cache, self.value_cache = _ref_view(self.k), _ref_view(self.v)
        self.init_graph = False
        self.last_scores = [None] * self.layers      # (H,C) fp16 / (H,sets) int32 of the last build, for parity checks
        self.last_idx = [None] * self.layers
        self.use_index = retrieval_index(index)
        self.index, self.indexed_chunks = None, [0] * self.layers

    __getattr__ = _refuse_k_v("RetrievalCache", RETRIEVAL_KV_ENV, "kc / vc / ke / ve, spec_k / spec_v")

    def nbytes(self):
        """Device bytes of the K / V storage (FP8: codes, exponents and the fp16 spec rows)."""
        if not self.fp8:
            return self.k.nbytes + self.v.nbytes
        return self.coded.nbytes() + self.spec_k.nbytes + self.spec_v.nbytes

    def dequantize(self, layer):
        """(k, v): fresh (H, real_budget, D) fp16 tensors of what the spec forward's attention reads in ``layer``: deq of the
        coded rows, then the fp16 spec rows."""
        if not self.fp8:
            return self.k[layer].clone(), self.v[layer].clone()
        H, D, B = self.num_heads, self.head_dim, self.max_budget
        k = torch.empty(1, H, self.real_budget, D, dtype=torch.float16, device=self.device)
        v = torch.empty_like(k)
        self.coded.dequant_into(slice(layer, layer + 1), k, v, 0, 0, B)
        k[0, :, B:], v[0, :, B:] = self.spec_k[layer], self.spec_v[layer]
        return k[0], v[0]

    def layer_codes(self, layer):
        """FP8: (k codes, v codes, k exponents, v exponents) of ``layer``: (H,max_budget,D) and (H,max_budget) views."""
        return self.coded.layer(layer)

    def reanchor(self, new_prefill):
        """Move the covered region to rows [0, new_prefill): the tail then starts there.  Moves no data — the caller follows
        it with a rebuild (a forward with ``rebuild_retrieval=True``) and the tail copy.  Growing and shrinking are both
        legal; shrinking forgets the chunk means above the new bound (those rows are about to be rewritten)."""
        new_prefill, c = int(new_prefill), self.chunk_size
        if new_prefill % c:
            raise ValueError(f"new_prefill={new_prefill} is not a multiple of chunk_size={c}")
        if new_prefill < self.prefill0:
            raise ValueError(f"new_prefill={new_prefill} is below prefill0={self.prefill0}, the region the cache was built over")
        if new_prefill // c > TOPK_MAX_CHUNKS:
            raise ValueError(f"new_prefill={new_prefill} is {new_prefill // c} chunks of {c} rows, more than the top-k's limit "
                             f"of {TOPK_MAX_CHUNKS} chunks")
        self.prefill, self.chunks = new_prefill, new_prefill // c
        self._tail_plan = None                       # (it holds the tail's first row)
        self.indexed_chunks = [min(n, self.chunks) for n in self.indexed_chunks]

    def _index_layer(self, kv_cache, layer_idx):
        """This layer's (H, Cmax, D) view of the chunk-mean index over ``kv_cache``, allocated at the first use."""
        cmax = kv_cache.max_budget // self.chunk_size
        key = (id(kv_cache), cmax)
        if self.index is None or self._index_key != key:
            self.index = torch.zeros(self.layers, self.num_heads, cmax, self.head_dim, dtype=torch.float16, device=self.device)
            self._index_key, self.indexed_chunks = key, [0] * self.layers
        return self.index[layer_idx]

    def print_status(self):
        print("[Retrieval Cache] Budget:", self.max_budget, " | PreFill:", self.prefill, " | Chunk Size:", self.chunk_size,
              " | Chunks:", self.chunks, " | Select Sets:", self.select_sets)

    def layer_kv(self, layer_idx):
        if self.fp8:                                  # the fp16 part: the spec rows (their row 0 is key max_budget)
            return self.spec_k[layer_idx], self.spec_v[layer_idx]
        return self.k[layer_idx], self.v[layer_idx]

    @property
    def spec_slot(self):
        return self.real_budget - self.gamma - 1

    def init_graph_cache(self, kv_cache, query_states, layer_idx):
        q = query_states.reshape(-1, self.q_heads, self.head_dim)
        assert 1 == q.shape[0], "query_states should be 1 for init"
        # grouped-query: one selection per KV head from the group's mean query; multi-head: q itself
        q = ops.group_mean_query(q[0], self.num_heads).unsqueeze(0)
        if kv_cache.fp8:                              # FP8 cache: score / select / gather over the dequantized prefill rows
            src_k, src_v = kv_cache.scratch_layer(layer_idx, self.prefill)
        else:
            src_k, src_v = kv_cache.layer_kv(layer_idx)
        if self.use_index:                            # means of the chunks not yet indexed, then the scores from the index
            index = self._index_layer(kv_cache, layer_idx)
            done = self.indexed_chunks[layer_idx]
            if done < self.chunks:
                ops.chunk_mean(src_k, index, done, self.chunks, self.chunk_size)
                self.indexed_chunks[layer_idx] = self.chunks
            scores = ops.retrieval_score_indexed(index, q[0].contiguous(), self.chunks)
        else:
            scores = ops.retrieval_score(src_k, q[0].contiguous(), self.chunks, self.chunk_size)
        idx = ops.retrieval_topk(scores, self.select_sets)
        if not self.fp8:
            ops.retrieval_gather(src_k, src_v, idx, self.k[layer_idx], self.v[layer_idx], self.chunk_size)
        elif kv_cache.fp8:                            # codes -> codes: the middle tier reads the deq the target reads
            kc, vc, ke, ve = kv_cache.layer_codes(layer_idx)
            ops.retrieval_gather_fp8(kc, vc, idx, *self.layer_codes(layer_idx), self.chunk_size, src_exp=(ke, ve))
        else:
            ops.retrieval_gather_fp8(src_k, src_v, idx, *self.layer_codes(layer_idx), self.chunk_size)
        self.last_scores[layer_idx], self.last_idx[layer_idx] = scores, idx
        if layer_idx == self.layers - 1:
            self.init_graph = True

    def _copy_tail(self, kv_cache, layers):
        """Rows [max_budget - g, max_budget) of ``layers`` = the g generated rows of ``kv_cache``.  What the source holds
        (tail_source) and what this cache holds select the operation:
            fp16 rows -> fp16 rows   copied       (ops.kv_copy_rows_pair)
            codes     -> fp16 rows   dequantized  (CodedRows.dequant_into; never planned)
            fp16 rows -> codes       quantized    (ops.kv_quant_rows_pair)
            codes     -> codes       copied with their exponent bytes (ops.kv_quant_rows_pair, src_exp)"""
        g = kv_cache.seq_len - self.prefill
        if g > self.max_budget:
            raise IndexError(f"generated tail ({g}) exceeds the retrieval budget ({self.max_budget})")
        d0 = self.max_budget - g
        # the per-step refresh over all layers: the same tensors every step -> a launch plan; only for the resident cache,
        # whose storage never moves (the offloading cache re-allocates its tail mirror)
        planned = layers == slice(0, self.layers) and self.key_cache.is_cuda and type(kv_cache) is FlashSimpleCache
        if planned:
            key, plan = (id(kv_cache), kv_cache.key_cache.data_ptr()), self._tail_plan
            if plan is not None and plan[0] == key:
                plan[1](plan[2], d0, g)
                return
        src_k, src_v, t0, src_exp = kv_cache.tail_source(layers, self.prefill)
        if src_exp is not None and not self.fp8:
            kv_cache.coded.dequant_into(layers, self.k[layers], self.v[layers], t0, d0, g)
            return
        if self.fp8:
            dst, how = self.coded.layers(layers), {"src_exp": src_exp}
            plan_of, run = ops.KvQuantPairPlan, ops.kv_quant_rows_pair
        else:
            dst, how = (self.k[layers], self.v[layers]), {}
            plan_of, run = ops.KvCopyPairPlan, ops.kv_copy_rows_pair
        if planned:
            self._tail_plan = (key, plan_of(src_k, src_v, *dst, **how), t0)
            self._tail_plan[1](t0, d0, g)
        else:
            run(src_k, src_v, *dst, t0, d0, g, **how)

    def update_graph_cache(self, kv_cache=None):
        self._copy_tail(kv_cache, slice(0, self.layers))

    def update_graph_cache_retrieval(self, kv_cache, query_states, layer_idx):
        self.init_graph_cache(kv_cache, query_states, layer_idx)
        self._copy_tail(kv_cache, slice(layer_idx, layer_idx + 1))

    def update(self, new_k_cache, new_v_cache, layer_idx):
        k, v = _rows(new_k_cache), _rows(new_v_cache)
        if self.fp8:                                  # the spec rows stay fp16; returns [deq(codes) | spec rows], reference shape
            self.spec_k[layer_idx], self.spec_v[layer_idx] = k.permute(1, 0, 2), v.permute(1, 0, 2)
            kd, vd = self.dequantize(layer_idx)
            return kd.permute(1, 0, 2).unsqueeze(0), vd.permute(1, 0, 2).unsqueeze(0)
        s = self.spec_slot
        self.k[layer_idx, :, s:] = k.permute(1, 0, 2)
        self.v[layer_idx, :, s:] = v.permute(1, 0, 2)
        return self.key_cache[layer_idx][:, :self.real_budget], self.value_cache[layer_idx][:, :self.real_budget]

    def reset(self):
        if self.fp8:
            self.coded.reset()
            self.spec_k.zero_()
            self.spec_v.zero_()
        else:
            self.k.zero_()
            self.v.zero_()
        if self.prefill != self.prefill0:            # a new prompt: the region the cache was built over, no chunk mean valid
            self.reanchor(self.prefill0)
        self.indexed_chunks = [0] * self.layers


class StreamingLLMEvictionCache(Cache):
    """Sink + sliding-window cache of the 68M draft (reference cache.py:200-265); keys un-rotated."""

    def __init__(self, model, gamma=6, start_size=16, recent_size=496) -> None:
        self.gamma = gamma
        self.start_size = start_size
        self.recent_size = recent_size
        self.real_budget = self.start_size + self.recent_size + self.gamma + 1 + 1 + 1
        self.seq_len = 0  # just for prefill usage
        self.layers, self.num_heads, self.head_dim = _geom(model)
        self.hidden_size = model.config.hidden_size
        self.device = model.device
        self.k, self.v = _alloc(self.layers, self.num_heads, self.real_budget, self.head_dim, self.device)
        self.key_cache, self.value_cache = _ref_view(self.k), _ref_view(self.v)

    def print_status(self):
        print("[StreamingLLM Cache] Start Size:", self.start_size, "| Recent Size:", self.recent_size, "| Gamma:", self.gamma,
              "| Real Budget:", self.real_budget, "| Cached:", self.seq_len)

    def layer_kv(self, layer_idx):
        return self.k[layer_idx], self.v[layer_idx]

    @property
    def spec_slot(self):
        return self.real_budget - self.gamma - 3

    def append_slot(self, layer_idx, n):
        assert self.seq_len + n <= self.start_size + self.recent_size
        slot = self.seq_len
        if layer_idx == self.layers - 1:
            self.seq_len += n
        return slot

    def update(self, key_states, value_states, layer_idx):
        k, v = _rows(key_states), _rows(value_states)
        n = k.shape[0]
        assert self.seq_len + n <= self.start_size + self.recent_size
        s = self.seq_len
        self.k[layer_idx, :, s:s + n] = k.permute(1, 0, 2)
        self.v[layer_idx, :, s:s + n] = v.permute(1, 0, 2)
        key = self.key_cache[layer_idx][:, :s + n]
        value = self.value_cache[layer_idx][:, :s + n]
        if layer_idx == self.layers - 1:
            self.seq_len += n
        return key, value

    def spec_update(self, new_k_cache, new_v_cache, layer_idx, gamma_offset=0):
        k, v = _rows(new_k_cache), _rows(new_v_cache)
        start = self.spec_slot
        end = start + k.shape[0]
        self.k[layer_idx, :, start:end] = k.permute(1, 0, 2)
        self.v[layer_idx, :, start:end] = v.permute(1, 0, 2)
        return self.key_cache[layer_idx][:, :end], self.value_cache[layer_idx][:, :end]

    def reset(self):
        self.k.zero_()
        self.v.zero_()

    def evict_prefill(self, incoming):
        if self.seq_len + incoming <= self.start_size + self.recent_size:
            return
        size_keep = self.recent_size - incoming
        ops.kv_shift_rows_pair(self.k, self.v, self.seq_len - size_keep, self.start_size, size_keep)
        self.seq_len = self.start_size + self.recent_size - incoming

    def evict_for_spec(self, current_seq_len):
        if self.k.is_cuda:
            plan = getattr(self, "_shift_plan", None)
            if plan is None:
                plan = self._shift_plan = ops.KvShiftPairPlan(self.k, self.v)
            plan(current_seq_len - self.recent_size, self.start_size, self.recent_size)
            return
        ops.kv_shift_rows_pair(self.k, self.v, current_seq_len - self.recent_size, self.start_size, self.recent_size)


# =============================================================================================
# Tensor-parallel / offloading caches (reference cache.py:268-383, :485-584)
# =============================================================================================
def _pin(t):
    return t.pin_memory() if torch.cuda.is_available() else t


def _pinned_zeros(*shape):
    """fp16 zeros in pinned host memory, allocated pinned from the start (t.pin_memory() would hold a pageable AND a
    pinned copy of a 50 GB offloaded cache for a moment)."""
    return torch.zeros(*shape, dtype=torch.float16, pin_memory=torch.cuda.is_available())


class DistributedSimpleCache(Cache):
    """This rank's heads of the full KV cache: layers < on_chip_layers live in HBM, the rest in pinned host
    memory and are streamed through two DistributedKVCacheBuffer's (reference cache.py:268-351).
    Unlike the reference, on_chip_layers == num_layers (nothing offloaded — the natural setting with
    288 GB of HBM) is allowed."""

    def __init__(self, config, max_budget=1024, device=None, on_chip_layers=0, ssl=0):
        _refuse_fp8("DistributedSimpleCache (the tensor-parallel and Sequoia engines)")
        _refuse_gqa(config, "DistributedSimpleCache (the tensor-parallel, offloading and Sequoia engines)")
        self.config = config
        self.world_size, self.local_rank = config.world_size, config.local_rank
        self.device = torch.device(device)
        self.max_budget = max_budget
        self.hidden_size = config.hidden_size
        self.num_heads = config.num_key_value_heads // self.world_size
        self.head_dim = config.hidden_size // config.num_attention_heads
        self.layers = config.num_hidden_layers
        self.on_chip_layers = min(on_chip_layers, self.layers)
        self.seq_len = 0
        n_on, n_off = self.on_chip_layers, self.layers - self.on_chip_layers
        self.k, self.v = _alloc(n_on, self.num_heads, max_budget, self.head_dim, self.device)
        self.cpu_k = _pinned_zeros(n_off, self.num_heads, max_budget, self.head_dim)
        self.cpu_v = _pinned_zeros(n_off, self.num_heads, max_budget, self.head_dim)
        self.key_cache, self.value_cache = _ref_view(self.k), _ref_view(self.v)
        self.cpu_key_cache, self.cpu_value_cache = _ref_view(self.cpu_k), _ref_view(self.cpu_v)

    def print_status(self):
        print("Cached Size:", self.seq_len, "| Max Budget:", self.max_budget)

    def reset(self):
        self.seq_len = 0
        self.cpu_k.zero_()
        self.cpu_v.zero_()
        self.k.zero_()
        self.v.zero_()

    def normal_(self, seq_len=1024 * 127):
        """The reference's own synthetic filler (cache.py:303-308)."""
        self.seq_len = seq_len
        for t in (self.cpu_k, self.cpu_v, self.k, self.v):
            t.normal_()

    def layer_kv(self, layer_idx):
        assert layer_idx < self.on_chip_layers, (layer_idx, self.on_chip_layers)
        return self.k[layer_idx], self.v[layer_idx]

    def host_layer_kv(self, layer_idx):
        i = layer_idx - self.on_chip_layers
        assert 0 <= i, (layer_idx, self.on_chip_layers)
        return self.cpu_k[i], self.cpu_v[i]

    def gather_kv_incremental(self, indices, offset):
        """Sequoia: keep only the accepted tree nodes — rows offset+indices[j] -> offset+j of every layer, then
        seq_len = offset + len(indices) (reference cache.py:333-343).  On-chip layers: one tf_kv_gather_rows
        launch; host-resident layers: pinned-memory row copies; the device mirror of the generated rows kept by
        the retrieval cache (``tail_mirror``) is compacted the same way."""
        idx = [int(i) for i in indices]
        assert all(b > a for a, b in zip(idx, idx[1:])), "accept list must be strictly increasing"
        n = len(idx)
        if n and idx != list(range(n)):
            dev_idx = torch.tensor(idx, dtype=torch.int32, device=self.device)
            if self.on_chip_layers > 0:
                ops.kv_gather_rows(self.k, self.v, offset, dev_idx, max_index=idx[-1])
            if self.on_chip_layers < self.layers:
                src = torch.tensor([offset + i for i in idx], dtype=torch.long)
                for t in (self.cpu_k, self.cpu_v):
                    t[:, :, offset:offset + n] = t[:, :, src]
            tm = getattr(self, "tail_mirror", None)
            if tm is not None and tm.tail_k is not None:
                ops.kv_gather_rows(tm.tail_k, tm.tail_v, offset - tm.prefill, dev_idx, max_index=idx[-1])
        self.seq_len = offset + n


class DistributedKVCacheBuffer:
    """Device staging buffer for one offloaded layer (reference cache.py:353-383)."""

    fp8 = False                                       # fp16 rows (not a Cache subclass: says so itself)

    def __init__(self, config, max_budget=1024, device=None) -> None:
        self.config = config
        self.max_budget = max_budget
        self.device = torch.device(device)
        self.num_heads = config.num_key_value_heads // config.world_size
        self.head_dim = config.hidden_size // config.num_attention_heads
        self.k = torch.zeros(self.num_heads, max_budget, self.head_dim, dtype=torch.float16, device=self.device)
        self.v = torch.zeros(self.num_heads, max_budget, self.head_dim, dtype=torch.float16, device=self.device)
        self.key_cache, self.value_cache = self.k.permute(1, 0, 2).unsqueeze(0), self.v.permute(1, 0, 2).unsqueeze(0)
        self.seq_len = 0

    def copy_kv(self, kv_cache, layer_idx, stream):
        """Stream the live tokens of one offloaded layer host -> device on `stream` (cache.py:372-376)."""
        hk, hv = kv_cache.host_layer_kv(layer_idx)
        ops.kv_h2d_async(self.k, hk, kv_cache.seq_len, stream)
        ops.kv_h2d_async(self.v, hv, kv_cache.seq_len, stream)
        self.seq_len = kv_cache.seq_len

    def copy_back(self, kv_cache, layer_idx, t0, n, stream):
        """Write the n new tokens back to the pinned host cache (cache.py:345-351)."""
        hk, hv = kv_cache.host_layer_kv(layer_idx)
        ops.kv_d2h_async(hk, self.k, t0, n, stream)
        ops.kv_d2h_async(hv, self.v, t0, n, stream)


class DistributedRetrievalCache:
    """Per-rank retrieval cache, always in HBM (reference cache.py:485-584).  Differences from the
    single-GPU class that the reference has and we keep: reset() clears init_graph, and building twice
    without a reset raises (cache.py:519-520,577-580)."""

    fp8 = False                                       # fp16 rows, also in DistributedRetrievalCache_Seqouia

    def __init__(self, config, max_budget=1024, device=None, prefill=1024, chunk_size=8, gamma=6) -> None:
        _refuse_retrieval_fp8("DistributedRetrievalCache (the tensor-parallel and Sequoia engines)")
        _refuse_gqa(config, "DistributedRetrievalCache (the tensor-parallel and Sequoia engines)")
        self.config = config
        self.world_size, self.local_rank = config.world_size, config.local_rank
        self.device = torch.device(device)
        self.hidden_size = config.hidden_size
        self.num_heads = config.num_key_value_heads // self.world_size
        self.head_dim = config.hidden_size // config.num_attention_heads
        self.layers = config.num_hidden_layers
        self.chunk_size, self.prefill, self.gamma, self.max_budget = chunk_size, prefill, gamma, max_budget
        self.chunks = prefill // chunk_size
        self.select_sets = max_budget // chunk_size
        assert prefill % self.chunk_size == 0, f"prefill should be multiple of chunk_size, got {prefill} % {self.chunk_size}"
        assert max_budget % self.chunk_size == 0, f"max_budget should be multiple of chunk_size, got {max_budget} % {self.chunk_size}"
        self.real_budget = max_budget + gamma + 1
        self.init_graph = False
        self.k, self.v = _alloc(self.layers, self.num_heads, self.real_budget, self.head_dim, self.device)
        self.key_cache, self.value_cache = _ref_view(self.k), _ref_view(self.v)
        # device-side copy of the generated-token KV of EVERY layer ([prefill, seq_len) rows), filled as the
        # target forward produces them, so refreshing the retrieval tail never has to touch host memory
        self.tail_k = self.tail_v = None
        self.last_scores = [None] * self.layers
        self.last_idx = [None] * self.layers

    def print_status(self):
        print("Budget:", self.max_budget, " | Real Budget:", self.real_budget, " | PreFill:", self.prefill, " | Chunk Size:",
              self.chunk_size, " | Chunks:", self.chunks, " | Select Sets:", self.select_sets)

    def layer_kv(self, layer_idx):
        return self.k[layer_idx], self.v[layer_idx]

    @property
    def spec_slot(self):
        return self.real_budget - self.gamma - 1

    def init_graph_cache(self, kv_view, query_states, layer_idx):
        """kv_view: (k_layer, v_layer) head-major views holding this layer's prefix (HBM cache or staging buffer)."""
        if self.init_graph:
            raise ValueError("Graph is already initialized")
        q = query_states.reshape(-1, self.num_heads, self.head_dim)
        assert 1 == q.shape[0], "query_states should be 1 for init"
        src_k, src_v = kv_view
        scores = ops.retrieval_score(src_k, q[0].contiguous(), self.chunks, self.chunk_size)
        idx = ops.retrieval_topk(scores, self.select_sets)
        ops.retrieval_gather(src_k, src_v, idx, self.k[layer_idx], self.v[layer_idx], self.chunk_size)
        self.last_scores[layer_idx], self.last_idx[layer_idx] = scores, idx
        if layer_idx == self.layers - 1:
            self.init_graph = True

    def update(self, key_states, value_states, layer_idx):
        k, v = _rows(key_states), _rows(value_states)
        s = self.spec_slot
        self.k[layer_idx, :, s:] = k.permute(1, 0, 2)
        self.v[layer_idx, :, s:] = v.permute(1, 0, 2)
        return self.key_cache[layer_idx][:, :self.real_budget], self.value_cache[layer_idx][:, :self.real_budget]

    def ensure_tail(self, capacity):
        if self.tail_k is None or self.tail_k.shape[2] < capacity:
            self.tail_k, self.tail_v = _alloc(self.layers, self.num_heads, capacity, self.head_dim, self.device)

    def update_graph_cache(self, kv_cache=None):
        """Copy the generated tokens' KV [prefill, seq_len) of all layers into slots [B-g, B)
        (cache.py:566-575).  The reference reads the offloaded layers back from pinned host memory here;
        we keep those rows in `tail_k/v` on the device (written during the target forward)."""
        g = kv_cache.seq_len - self.prefill
        if g <= 0:
            return
        if g > self.max_budget:
            raise IndexError(f"generated tail ({g}) exceeds the retrieval budget ({self.max_budget})")
        ops.kv_copy_rows_pair(self.tail_k, self.tail_v, self.k, self.v, 0, self.max_budget - g, g)

    def reset(self):
        self.k.zero_()
        self.v.zero_()
        self.init_graph = False

    def normal_(self):
        self.k.normal_()
        self.v.normal_()


class DistributedRetrievalCache_Seqouia(DistributedRetrievalCache):
    """Retrieval cache of the Sequoia tree path (reference cache.py:385-483; the reference's spelling of the
    class name is kept).  Same chunk-scored build as DistributedRetrievalCache; the speculative region holds one
    KV row per TREE NODE — slot max_budget + node id, written through ``storage_ids`` (:459-466) — instead of the
    gamma+1 chain slots, so real_budget = max_budget + tree_size."""

    def __init__(self, config, max_budget=1024, device=None, prefill=1024, chunk_size=8, tree_size=128) -> None:
        super().__init__(config, max_budget=max_budget, device=device, prefill=prefill, chunk_size=chunk_size,
                         gamma=tree_size - 1)
        self.tree_size = tree_size
        assert self.real_budget == max_budget + tree_size

    def update(self, key_states, value_states, layer_idx, storage_ids):
        k, v = _rows(key_states), _rows(value_states)
        input_length = len(storage_ids)
        assert input_length == k.shape[0] and input_length == v.shape[0]
        ids = torch.as_tensor(storage_ids, device=self.k.device, dtype=torch.long)
        self.k[layer_idx].index_copy_(1, ids, k.permute(1, 0, 2).contiguous())
        self.v[layer_idx].index_copy_(1, ids, v.permute(1, 0, 2).contiguous())
        return self.key_cache[layer_idx], self.value_cache[layer_idx]
