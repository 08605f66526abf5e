"""The launch list of a decoder layer, pinned without a GPU: the ``ops`` entry points the layer body uses are replaced
by recorders that return correctly shaped CPU tensors, the fused predicate is forced, and the sequence of op names of
each engine and form is compared with a list written out by hand.  (No kernel and no arithmetic is validated here.)"""
import inspect

import pytest
import torch

RECORDED = ("embed_rows", "ss_buffer", "qkv_rope", "rope_append", "rmsnorm", "linear", "mlp_act", "attn_decode",
            "attn_prefill", "attn_rope_on_read", "attn_decode_fp8", "kv_quant_rows", "kv_dequant_rows_pair")
ROWS = (7, 17)
CFG = dict(num_hidden_layers=2, hidden_size=64, num_attention_heads=2, intermediate_size=128, vocab_size=64,
           max_position_embeddings=256)


class Trace:
    """Recorders over ``ops``: ``calls`` holds (name, {parameter: argument}) of every call, defaults filled in."""

    def __init__(self, monkeypatch, ops):
        self.ops, self.calls = ops, []
        for name in RECORDED:
            monkeypatch.setattr(ops, name, self._recorder(name, inspect.signature(getattr(ops, name))))

    def _recorder(self, name, sig):
        def record(*a, **kw):
            b = sig.bind(*a, **kw)
            b.apply_defaults()
            self.calls.append((name, dict(b.arguments)))
            return getattr(self, "_" + name, lambda **_: None)(**b.arguments)
        record.__signature__ = sig                        # (a later Trace may wrap this one)
        return record

    def names(self):
        return [n for n, _ in self.calls if n != "ss_buffer"]           # (an allocation, not a launch)

    def args(self, name):
        return [a for n, a in self.calls if n == name]

    # -- what each recorder hands back: zeros of the real op's shape, dtype and layout ----------------------------
    def _block(self, M, N, like, dtype=torch.float16):
        if isinstance(like, self.ops.Act) or like is True:
            return self.ops.Act(torch.zeros(N // 8, M, 8, dtype=torch.float16), M)
        return torch.zeros(M, N, dtype=dtype)

    def _embed_rows(self, embed, ids, packed, out):
        return out if out is not None else self._block(ids.numel(), embed.shape[1], bool(packed))

    def _ss_buffer(self, hidden, device):
        return torch.zeros(hidden // 16, 32, dtype=torch.float32)

    def _qkv_rope(self, x, H, D, **_):
        return torch.zeros(x.shape[0], H, D, dtype=torch.float16)

    def _rope_append(self, qkv, H, D, **_):
        return torch.zeros(qkv.shape[0], H, D, dtype=torch.float16)

    def _rmsnorm(self, x, **_):
        return torch.zeros_like(x)

    def _linear(self, x, w, out_f32, out, **_):
        if out is not None:
            return out
        return self._block(x.shape[0], w.N, None if out_f32 else x, torch.float32 if out_f32 else torch.float16)

    def _mlp_act(self, h, wgu, **_):
        return self._block(h.shape[0], wgu.N // 2, h)

    def _attn_decode(self, q, packed, **_):
        return self._block(q.shape[0], q.shape[1] * q.shape[2], bool(packed))

    _attn_decode_fp8 = _attn_decode

    def _attn_prefill(self, q, **_):
        return self._block(q.shape[0], q.shape[1] * q.shape[2], None)

    _attn_rope_on_read = _attn_prefill


def force_fused(monkeypatch, ops, weights, fused):
    """The fused predicate of the single-GPU models, forced: it asks for packed device weights, which a CPU never has."""
    monkeypatch.setattr(ops, "FUSE_MODE", "all")
    monkeypatch.setattr(ops, "can_fuse", lambda *a: fused)
    monkeypatch.setattr(ops, "can_fuse_rows", lambda *a: fused)
    weights.wqkv[0].wp_rope = object() if fused else None


def make_target(cfg=CFG):
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    return LlamaForCausalLM(LlamaConfig.from_dict(cfg), "cpu").init_random(1)


def make_draft(cfg=CFG):
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM
    return LlamaForCausalLM(LlamaConfig.from_dict(cfg), "cpu").init_random(2)


def make_tp(monkeypatch, rows, fused, cfg=CFG):
    """DistributedLlama at world size 1 (no process group is touched there) with its fused predicate forced."""
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.TP_llama import DistributedLlama
    c = LlamaConfig.from_dict(cfg)
    llm = DistributedLlama("random:3", config=c, device="cpu", local_rank=0, world_size=1, prefill=32, gen_len=32,
                           retrieval_budget=16, kv_offload=True, on_chip_layers=c.num_hidden_layers, gamma=rows - 1)
    llm.init_parameters()
    monkeypatch.setattr(llm, "_fused_decode", lambda q_len, tree=None: fused)
    return llm


def ids_of(rows, vocab=CFG["vocab_size"]):
    return (torch.arange(rows).view(1, -1) * 5 + 3) % vocab


def fake_fp8(ops, weights):
    """Fp8Linear stand-ins on every GEMM weight (the real ones quantize on the device) and the tier switched on."""
    for pl in [weights.lm_head] + weights.wqkv + weights.wo + weights.wgu + weights.wd:
        f8 = object.__new__(ops.Fp8Linear)
        f8.src, f8.N, f8.K, f8.split, f8.rope = pl, pl.N, pl.K, pl.split, pl.rope
        pl.fp8 = f8
    weights.retrieval_fp8 = True


L = CFG["num_hidden_layers"]
FUSED_LAYER = ["qkv_rope", "attn_decode", "linear", "mlp_act", "linear"]
PLAIN_LAYER = ["rmsnorm", "linear", "rope_append", "attn_prefill", "linear", "rmsnorm", "mlp_act", "linear"]


def _with_attention(layer, attention):
    return [attention if n.startswith("attn_") else n for n in layer]


@pytest.mark.parametrize("rows", ROWS)
def test_target_fused(cpu_ops, monkeypatch, rows):
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache
    m = make_target()
    force_fused(monkeypatch, cpu_ops, m.weights, True)
    kv, rc = FlashSimpleCache(m, 64), RetrievalCache(m, max_budget=16, prefill=32, chunk_size=8, gamma=rows - 1)
    # the retrieval-cache (spec) forward
    t = Trace(monkeypatch, cpu_ops)
    out = m(input_ids=ids_of(rows), kv_cache=kv, graph_cache=rc, position_ids=torch.arange(rows).view(1, -1), spec=True)
    assert out.logits.shape == (1, rows, CFG["vocab_size"])
    assert t.names() == ["embed_rows"] + FUSED_LAYER * L + ["linear"]
    assert [a["ss_in"] is None for a in t.args("qkv_rope")] == [True] + [False] * (L - 1)
    assert all(a["ss_in"] is not None for a in t.args("mlp_act") + t.args("linear")[-1:])
    # the full-cache forward: the k-octet-major rows (from 17) go through the decode attention, row-major ones do not
    t = Trace(monkeypatch, cpu_ops)
    m(input_ids=ids_of(rows), kv_cache=kv)
    attention = "attn_decode" if cpu_ops.act_packed(rows) else "attn_prefill"
    assert cpu_ops.act_packed(rows) == (rows == 17)
    assert t.names() == ["embed_rows"] + _with_attention(FUSED_LAYER, attention) * L + ["linear"]
    assert [a["ss_in"] is None for a in t.args("qkv_rope")] == [True] + [False] * (L - 1)
    assert kv.seq_len == rows


@pytest.mark.parametrize("rows", ROWS)
def test_target_fused_spec_forward_streams_fp8_weights(cpu_ops, monkeypatch, rows):
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache
    m = make_target()
    force_fused(monkeypatch, cpu_ops, m.weights, True)
    fake_fp8(cpu_ops, m.weights)
    kv, rc = FlashSimpleCache(m, 64), RetrievalCache(m, max_budget=16, prefill=32, chunk_size=8, gamma=rows - 1)
    t = Trace(monkeypatch, cpu_ops)
    m(input_ids=ids_of(rows), kv_cache=kv, graph_cache=rc, position_ids=torch.arange(rows).view(1, -1), spec=True)
    assert t.names() == ["embed_rows"] + FUSED_LAYER * L + ["linear"]
    gemm_weights = [a["wqkv"] for a in t.args("qkv_rope")] + [a["w"] for a in t.args("linear")] + \
                   [a["wgu"] for a in t.args("mlp_act")]
    assert len(gemm_weights) == 4 * L + 1 and all(isinstance(w, cpu_ops.Fp8Linear) for w in gemm_weights)
    W = m.weights
    assert [a["w"] for a in t.args("linear")] == [w.fp8 for i in range(L) for w in (W.wo[i], W.wd[i])] + [W.lm_head.fp8]
    # every other forward keeps the fp16 weights
    t = Trace(monkeypatch, cpu_ops)
    m(input_ids=ids_of(rows), kv_cache=kv)
    assert not any(isinstance(a["w"], cpu_ops.Fp8Linear) for a in t.args("linear"))


@pytest.mark.parametrize("rows", ROWS)
def test_target_unfused(cpu_ops, monkeypatch, rows):
    from triforce_amd.models.cache import FlashSimpleCache
    m = make_target()
    force_fused(monkeypatch, cpu_ops, m.weights, False)
    kv = FlashSimpleCache(m, 64)
    t = Trace(monkeypatch, cpu_ops)
    out = m(input_ids=ids_of(rows), kv_cache=kv)
    assert out.logits.shape == (1, rows, CFG["vocab_size"])
    assert t.names() == ["embed_rows"] + PLAIN_LAYER * L + ["rmsnorm", "linear"]
    # layer 0 norms the embedding rows alone; every later norm folds the pending residual add
    assert [a["residual"] is None for a in t.args("rmsnorm")] == [True] + [False] * (2 * L)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("rows", ROWS)
def test_draft_fallback(cpu_ops, monkeypatch, rows, fused):
    from triforce_amd.models.cache import StreamingLLMEvictionCache
    m = make_draft()
    force_fused(monkeypatch, cpu_ops, m.weights, fused)
    c = StreamingLLMEvictionCache(m, gamma=6, start_size=4, recent_size=40)
    t = Trace(monkeypatch, cpu_ops)
    out = m.forward(ids_of(rows), c, c)
    assert out.logits.shape == (1, rows, CFG["vocab_size"])
    if fused:
        assert t.names() == _with_attention(FUSED_LAYER, "attn_rope_on_read") * L + ["linear"]
        assert [a["ss_in"] is None for a in t.args("qkv_rope")] == [True] + [False] * (L - 1)
    else:
        assert t.names() == _with_attention(PLAIN_LAYER, "attn_rope_on_read") * L + ["rmsnorm", "linear"]
    assert not any(a["rotate_k"] for a in t.args("qkv_rope") + t.args("rope_append"))     # keys are cached un-rotated


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("rows", ROWS)
def test_tensor_parallel_engine_at_world_size_1(cpu_ops, monkeypatch, rows, fused):
    llm = make_tp(monkeypatch, rows, fused)
    want = ["embed_rows"] + (FUSED_LAYER * L + ["linear"] if fused else PLAIN_LAYER * L + ["rmsnorm", "linear"])
    t = Trace(monkeypatch, cpu_ops)
    logits = llm.inference(ids_of(rows))
    assert logits.shape == (1, rows, CFG["vocab_size"]) and llm.kv_cache.seq_len == rows
    assert t.names() == want
    t = Trace(monkeypatch, cpu_ops)
    llm.retrieval_inference(ids_of(rows), torch.arange(rows, 2 * rows).view(1, -1))
    assert t.names() == want
    if fused:                                            # residual + sums of squares in the o / down GEMM's own epilogue
        assert all(a["out"] is a["resid"] is not None and a["ss_out"] is not None for a in t.args("linear")[:-1])
        assert [a["ss_in"] is None for a in t.args("qkv_rope")] == [True] + [False] * (L - 1)
