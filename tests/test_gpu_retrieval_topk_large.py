"""tf_retrieval_topk_large on the device against a plain torch restatement of its contract, against
tf_retrieval_topk and the oracle where they still apply, and through a resident engine over 32 776 chunks.  All torch.equal."""
import pytest
import torch

from oracle import ref_ops as R
from tests import helpers as Hh
from tests.test_gpu_e2e import GAP_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def reference(scores, sets):
    """(H, sets) int32: chunk 0, then the sets - 1 best of [1, C) by sortable_fp16 pattern, ascending chunk among equals."""
    H, C = scores.shape
    b = scores[:, 1:].view(torch.int16).to(torch.int64) & 0xFFFF
    pattern = torch.where((b & 0x8000) != 0, (~b) & 0xFFFF, b | 0x8000)
    key = (pattern << 32) | (0xFFFFFFFF - torch.arange(1, C, device=scores.device))
    order = key.argsort(dim=1, descending=True)[:, :sets - 1] + 1
    return torch.cat([torch.zeros_like(order[:, :1]), order], dim=1).to(torch.int32)


def materials(H, C, seed):
    gen = torch.Generator().manual_seed(seed)
    rnd = torch.randn(H, C, generator=gen).half()
    at = torch.randint(1, C, (H, 40), generator=gen)
    at[:, :5] = torch.tensor([1, 2, C - 3, C - 2, C - 1])                # ... some of them in the scalar head and tail
    rnd.scatter_(1, at, torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan")]).half().repeat(8).expand(H, 40))
    four = torch.tensor([-1.0, 0.5, 0.50048828125, 2.0]).half()[torch.randint(0, 4, (H, C), generator=gen)]
    ramp = (torch.arange(C) / C).half().repeat(H, 1)                     # non-decreasing; the best are the last 7 chunks
    ramp[:, C - 7:] = torch.arange(2, 9).half()
    return {"random": rnd, "four values": four, "all equal": torch.full((H, C), 0.25).half(), "ramp": ramp}


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("C", [32769, 65537, 131080, 1048576])
def test_large_topk_equals_the_reference(C, H):
    from triforce_amd import ops
    for name, scores in materials(H, C, 7 * H + C % 1000).items():
        scores = scores.to(DEV)
        want = reference(scores, 8193)
        for sets in (2, 513, 8193):
            got = ops.retrieval_topk_large(scores, sets)
            assert got.dtype == torch.int32 and torch.equal(got, want[:, :sets]), (name, C, sets, H)
            assert torch.equal(ops.retrieval_topk_large(scores, sets), got), (name, C, sets, H)     # deterministic
        if name == "all equal":
            assert torch.equal(want[0].cpu(), torch.arange(8193, dtype=torch.int32))


@pytest.mark.parametrize("C", [2, 3, 1000, 32768, 65536])
def test_large_topk_equals_the_small_kernel_and_the_oracle_where_they_apply(C):
    from triforce_amd import ops
    for name, scores in materials(3, max(C, 8), C).items():
        scores = scores[:, :C].contiguous()
        for sets in sorted({1, 2, min(C, 3), min(C, 513), min(C, 8193)}):
            got = ops.retrieval_topk_large(scores.to(DEV), sets)
            if C <= 32768:
                assert torch.equal(got, ops.retrieval_topk(scores.to(DEV), sets)), (name, C, sets)
            else:                                                        # the last size at which the oracle's key is sound
                assert torch.equal(got.cpu().long(), R.retrieval_topk(scores, sets)), (name, C, sets)


def test_engine_over_32776_chunks_selects_by_the_large_kernel():
    """A two-layer D = 128 target over a 65 552-token prompt at chunk_size 2: the selection is the reference's on the device's
    own scores, the cache re-anchors past its first size, the greedy stream passes tests/test_gpu_e2e.py's teacher-forced check."""
    from triforce_amd import ops
    from triforce_amd.utils.decoding import TriForce
    g = dict(Hh.load_golden("small_gamma6"), prefill=65552, budget=64, chunk=2, gen_len=12,
             tcfg=Hh.specs.tiny_target_config(vocab_size=1024, layers=2, hidden=256, heads=2, max_pos=70000))
    ge = Hh.build_product(g, DEV)
    res = TriForce(Hh.FakeTokenizer(), ge, Hh.prompt_of(g).to(DEV), gamma=g["gamma"], max_len=g["gen_len"], top_k=-1,
                   top_p=g["top_p"], temperature=g["temperature"], return_details=True)
    rc = ge.engine.graph_cache
    assert rc.chunks == 32776 and rc.topk_max_chunks == ops.TOPK_LARGE_MAX_CHUNKS
    for layer in range(rc.layers):
        assert torch.equal(rc.last_idx[layer], reference(rc.last_scores[layer], rc.select_sets))
    gaps = Hh.teacher_forced_gaps(g, res["tokens"])
    assert max(gaps) < GAP_TOL, f"token {gaps.index(max(gaps))} trails the oracle argmax by {max(gaps):.4f} logit"
    assert sum(1 for x in gaps if x == 0.0) >= len(gaps) - 3
    rc.reanchor(65552 + 2 * 8)
