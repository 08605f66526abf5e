"""tf_retrieval_topk_large without a GPU: C ABI, argument gates, ops constants, RetrievalCache routing and limits."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ERANGE = -22, -34


def test_entry_point_is_declared_exported_restated_and_gates_before_launching():
    from triforce_amd import hip, ops
    decl = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "triforce_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+tf_retrieval_topk_large\s*\(", decl)
    assert re.search(r"#define\s+TF_RETRIEVAL_TOPK_LARGE_MAX_CHUNKS\s+1048576\b", decl)
    lib = hip.lib()
    assert "tf_retrieval_topk_large" in hip.SIGNATURES and hasattr(lib, "tf_retrieval_topk_large")
    assert ops.TOPK_LARGE_MAX_CHUNKS == 1048576 and ops.TOPK_LARGE_MAX_SETS == 8193
    # host buffers stand in for device pointers: every call below must return before any launch
    p, null = ctypes.cast((ctypes.c_int32 * 16)(), ctypes.c_void_p), ctypes.c_void_p(0)

    def topk(scores=p, idx=p, C=1048576, sets=4, H=1):
        return lib.tf_retrieval_topk_large(scores, idx, C, sets, H, null)
    for bad in (dict(scores=null), dict(idx=null), dict(C=1, sets=1), dict(C=0, sets=1), dict(sets=0), dict(sets=-1),
                dict(C=100, sets=101), dict(H=0), dict(H=-1)):
        assert topk(**bad) == EINVAL, bad
    assert topk(C=1048577) == ERANGE and topk(C=1 << 30) == ERANGE
    assert topk(sets=8194) == ERANGE and topk(C=8194, sets=8194) == ERANGE
    for both in (dict(C=1048577, H=0), dict(C=1048577, scores=null), dict(sets=8194, idx=null), dict(C=1048577, sets=1048578)):
        assert topk(**both) == EINVAL, both                              # TF_EINVAL outranks TF_ERANGE


def _cache(**kw):
    from triforce_amd.models.cache import RetrievalCache
    cfg = types.SimpleNamespace(num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, hidden_size=16)
    return RetrievalCache(types.SimpleNamespace(config=cfg, device="cpu"), gamma=1, **kw)


@pytest.mark.parametrize("chunks,want", [(32768, "retrieval_topk"), (32769, "retrieval_topk_large")])
def test_retrieval_cache_routes_by_the_chunk_count(chunks, want, monkeypatch):
    from triforce_amd import ops
    calls = []
    monkeypatch.setattr(ops, "group_mean_query", lambda q, heads: q)
    monkeypatch.setattr(ops, "retrieval_score", lambda k, q, C, chunk: ("scores", C))
    monkeypatch.setattr(ops, "retrieval_gather", lambda *a: None)
    for name in ("retrieval_topk", "retrieval_topk_large"):
        monkeypatch.setattr(ops, name, lambda scores, sets, _n=name: (calls.append((_n, scores, sets)), "idx")[1])
    rc = _cache(max_budget=8, prefill=chunks * 2, chunk_size=2)
    assert rc.topk_max_chunks == (32768 if chunks <= 32768 else ops.TOPK_LARGE_MAX_CHUNKS)
    kv = types.SimpleNamespace(fp8=False, layer_kv=lambda layer: (None, None))
    rc.init_graph_cache(kv, torch.zeros(1, 2, 8, dtype=torch.float16), 0)
    assert calls == [(want, ("scores", chunks), 4)] and rc.last_idx[0] == "idx" and rc.init_graph


def test_retrieval_cache_limits_are_fixed_at_construction():
    with pytest.raises(ValueError, match="1048577 chunks of 1 rows, more than the large top-k's limit of 1048576 chunks"):
        _cache(max_budget=8, prefill=1048577, chunk_size=1)
    with pytest.raises(ValueError, match="8194 chunks of 1 rows, more than the 8193 the large top-k selects"):
        _cache(max_budget=8194, prefill=32769, chunk_size=1)
    _cache(max_budget=8193, prefill=32769, chunk_size=1)
    small = _cache(max_budget=64, prefill=128, chunk_size=8)
    assert small.topk_max_chunks == 32768 == _cache(max_budget=8194, prefill=32768, chunk_size=1).topk_max_chunks
    with pytest.raises(ValueError, match="32769 chunks of 8 rows, more than the top-k's limit of 32768 chunks"):
        small.reanchor(32769 * 8)
    big = _cache(max_budget=64, prefill=32776 * 2, chunk_size=2)
    big.reanchor(1048576 * 2)                                            # a cache built above the limit grows to the large one
    assert big.chunks == 1048576
