"""Prompt-lookup n-gram draft tier (include/triforce_hip.h "N-GRAM DRAFT") on CPU: the torch restatement
of the rule (ops.ngram_draft_host) against a brute force, the history commit, and the real TriForceRunner loop over a
tiny-sized target with every HIP op swapped for its oracle restatement (cpu_ops).  The kernels are checked against the same
restatement in tests/test_gpu_ngram_draft.py, which imports the named cases below."""
import pytest
import torch

from tests import helpers as Hh

GREEDY = dict(top_k=-1, top_p=1e-9, temperature=1.0)


def brute(ctx, N, V):
    """The rule, ten lines: for every candidate j the longest n = N .. 1 whose n tokens ending at j equal the context's last n."""
    T = len(ctx)
    ok = lambda t: 0 <= t < V
    best = (0, -1)
    for j in range(T - 1):
        for n in range(min(N, j + 1), 0, -1):
            if all(ok(ctx[j - k]) and ctx[j - k] == ctx[T - 1 - k] for k in range(n)):
                best = max(best, (n, j))
                break
    d = ctx[best[1] + 1] if best[0] >= 1 else ctx[T - 1]
    return (d if ok(d) else 0), best[0], best[1], T


def run_rule(hist, blk, N, V, cap=None, device="cpu", q_fill=None):
    """ops.ngram_draft over hist ++ blk on ``device`` -> (q, info as a list)."""
    from triforce_amd import ops
    cap = max(len(hist), 1) if cap is None else cap
    h = torch.zeros(cap, dtype=torch.int32)
    h[:len(hist)] = torch.tensor(hist, dtype=torch.int64).to(torch.int32)
    h, L = h.to(device), torch.tensor([len(hist)], dtype=torch.int32, device=device)
    q = None if q_fill is None else torch.full((V,), q_fill, dtype=torch.float32, device=device)
    q, info = ops.ngram_draft(h, L, torch.tensor(blk, dtype=torch.int64, device=device), N, V, q=q)
    return q, info.tolist()


# (name, hist, blk, N, V, expected (d, l, j*, T)) — every expectation written out by hand
NAMED = [
    ("T == 1: the token itself", [], [5], 3, 16, (5, 0, -1, 1)),
    ("L == 0: the block alone", [], [1, 2, 1], 3, 16, (2, 1, 0, 3)),
    ("no match: the last token", [1, 2, 3], [4], 3, 16, (4, 0, -1, 4)),
    ("pattern straddles the boundary", [9, 1, 2, 7, 1], [2], 3, 16, (7, 2, 2, 6)),
    ("candidate straddles the boundary", [4, 1], [2, 8, 1, 2], 3, 16, (8, 2, 2, 6)),
    ("self-overlapping run a a a", [3, 3], [3], 2, 16, (3, 2, 1, 3)),
    ("longer but older beats shorter but newer", [1, 2, 5, 9, 2, 6], [1, 2], 3, 16, (5, 2, 1, 8)),
    ("newest wins among equals", [7, 1, 7, 2, 7, 3], [7], 1, 16, (3, 1, 4, 7)),
    ("j < N - 1: a match at the very start", [4, 5, 9], [4], 3, 16, (5, 1, 0, 4)),
    ("ids 0 and V - 1", [0, 15, 0], [15, 0], 3, 16, (15, 3, 2, 5)),
    ("an id outside [0, V) in the history breaks the run", [1, 16, 2, 5, 3, 16, 2], [6, 16, 2], 3, 16, (6, 1, 6, 10)),
    ("an id outside [0, V) as the suffix's last token matches nothing", [16, 4, 16], [16], 3, 16, (0, 0, -1, 4)),
    ("a negative id equals nothing, itself included", [-1, 4, -1], [-1], 3, 16, (0, 0, -1, 4)),
    ("an id outside [0, V) as the would-be proposal", [3, 16, 7], [3], 3, 16, (0, 1, 0, 4)),
    ("a periodic history proposes the period's next symbol", [1, 2, 3] * 5, [1, 2], 3, 16, (3, 3, 13, 17)),
    ("N = 8 matches eight", list(range(1, 10)) + [0] + list(range(1, 9)), [9], 8, 16, (0, 8, 8, 19)),
    ("N = 1 looks at one token", [1, 2, 3, 1, 2, 4], [1, 2], 1, 16, (4, 1, 4, 8)),
]


@pytest.mark.parametrize("case", NAMED, ids=[c[0] for c in NAMED])
def test_named_cases(case):
    _, hist, blk, N, V, want = case
    assert brute(hist + blk, N, V) == want              # (the brute force and the hand-written expectation agree)
    q, info = run_rule(hist, blk, N, V)
    assert tuple(info) == want
    one_hot = torch.zeros(V)
    one_hot[want[0]] = 1.0
    assert torch.equal(q, one_hot)


def random_cases(n, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=gen))
    for _ in range(n):
        A, L, m, N = r(2, 4), r(0, 40), r(1, 8), r(1, 8)
        V = A if r(0, 3) else A - 1                      # one in four: the largest symbol is outside the vocabulary
        ctx = torch.randint(0, A, (L + m,), generator=gen).tolist()
        yield ctx[:L], ctx[L:], N, V


def test_host_restatement_against_the_brute_force():
    matched = 0
    for hist, blk, N, V in random_cases(400, 5):
        want = brute(hist + blk, N, V)
        q, info = run_rule(hist, blk, N, V, q_fill=float("nan"))
        assert tuple(info) == want, (hist, blk, N, V)
        assert float(q.sum()) == 1.0 and float(q[want[0]]) == 1.0 and not bool(torch.isnan(q).any())
        matched += want[1] >= 2
    assert matched > 100                                 # small alphabets: matches abound


def test_len_is_clamped_to_the_capacity():
    from triforce_amd import ops
    hist = torch.tensor([1, 2, 1, 2], dtype=torch.int32)
    blk = torch.tensor([1], dtype=torch.int64)
    for L, want in ((9, (2, 3, 2, 5)), (-3, (1, 0, -1, 1))):
        _, info = ops.ngram_draft(hist, torch.tensor([L], dtype=torch.int32), blk, 3, 8)
        assert tuple(info.tolist()) == want


# ---- the commit --------------------------------------------------------------------------------------------------------
def commit_cases(device):
    """append, the capacity refusal (IndexError on the host, nothing written by the op), int64 -> int32."""
    from triforce_amd import ops
    from triforce_amd.models.ngram_draft import NgramCache
    c = NgramCache(10, device)
    c.set(torch.tensor([[5, 6, 7]], device=device))
    src = torch.tensor([8, 9, (1 << 32) + 3, -2, 77], dtype=torch.int64, device=device)
    c.commit(src, 4)                                     # (the fifth entry is not read)
    assert c.length == 7 and int(c.len_dev) == 7 and c.tokens() == [5, 6, 7, 8, 9, 3, -2]
    c.commit(src, 0)
    assert c.length == 7 and int(c.len_dev) == 7
    with pytest.raises(IndexError, match="NgramCache overflow: 7\\+4 > 10"):
        c.commit(src, 4)
    before = c.hist.clone()
    ops.ngram_commit(c.hist, c.len_dev, src, 4)          # the op itself: L + n > cap writes nothing
    assert torch.equal(c.hist, before) and int(c.len_dev) == 7 and c.length == 7
    c.commit(src, 3)                                     # exactly full
    assert c.length == 10 and c.tokens()[7:] == [8, 9, 3]
    with pytest.raises(IndexError):
        c.set(torch.zeros(11, dtype=torch.long, device=device))
    c.reset()
    assert c.length == 0 and int(c.len_dev) == 0 and c.tokens() == []
    c.seq_len = 0                                        # (what extend() writes behind reset())
    with pytest.raises(ValueError):
        c.seq_len = 4


def test_commit():
    commit_cases("cpu")


# ---- the loop ----------------------------------------------------------------------------------------------------------
V_TINY, P_TINY, GAMMA = 512, 200, 4


def tiny_engine(device="cpu", V=V_TINY, prefill=P_TINY, gamma=GAMMA, room=160, ngram_max=3, seed=7):
    from oracle import specs
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    from triforce_amd.models.ngram_draft import NgramCache, NgramDraft
    from triforce_amd.utils.graph_infer import GraphInferenceEngine
    tcfg = specs.tiny_target_config(vocab_size=V, layers=2, hidden=256, heads=2, max_pos=4096)
    target = LlamaForCausalLM.from_state_dict(LlamaConfig.from_dict(tcfg), specs.random_state_dict(tcfg, seed, head_std=0.05), device)
    full = FlashSimpleCache(target, prefill + room)
    ge = GraphInferenceEngine(target, full, RetrievalCache(target, max_budget=128, prefill=prefill, gamma=gamma, chunk_size=8),
                              NgramDraft(V, device, ngram_max=ngram_max), NgramCache(full.max_budget, device, gamma=gamma))
    ge.initialize_eager(gamma, probs=True, **{k: GREEDY[k] for k in ("temperature", "top_p")})
    return ge


def repetitive_prompt(V, n, seed):
    """A prompt that repeats a 23-token phrase with a few random tokens in between: the lookup finds matches."""
    gen = torch.Generator().manual_seed(seed)
    phrase = torch.randint(3, V, (23,), generator=gen)
    parts = []
    while sum(p.numel() for p in parts) < n:
        parts += [phrase, torch.randint(3, V, (int(torch.randint(1, 6, (1,), generator=gen)),), generator=gen)]
    return torch.cat(parts)[:n].unsqueeze(0)


def check_invariant(run):
    """hist[0:L] is the ids of the full cache's rows; the host mirror agrees."""
    dc = run.eng.draft_cache
    want = run.history[0].tolist() + list(run._fed)
    assert dc.tokens() == want and dc.length == len(want) == run.eng.kv_cache.seq_len


def test_greedy_stream_is_the_autoregressive_stream_and_the_invariant_holds(cpu_ops):
    from triforce_amd.utils.decoding import Autoregressive, TriForceRunner
    ge = tiny_engine()
    run = TriForceRunner(Hh.FakeTokenizer(), ge, GAMMA, **GREEDY)
    assert run.ngram is ge.engine.draft_cache
    drafted = accepted = 0
    for seed in (1, 2):                                  # two prompts on one engine
        prompt = repetitive_prompt(V_TINY, P_TINY, seed)
        run.n, run.counts = 0, []
        run.prefill(prompt)
        check_invariant(run)
        while run.n < 40:
            run.step()
            check_invariant(run)
        got = list(run.emitted)
        drafted, accepted = drafted + run.draft_count, accepted + run.accepted_count
        _, ar = Autoregressive(Hh.FakeTokenizer(), ge, prompt, max_len=len(got) - 1, return_tokens=True, **GREEDY)
        assert got == ar
    assert drafted > 0 and accepted > 0                  # the stream did come out of the speculative loop


def test_invariant_holds_across_extend(cpu_ops):
    from triforce_amd.utils.decoding import TriForceRunner
    ge = tiny_engine()
    run = TriForceRunner(Hh.FakeTokenizer(), ge, GAMMA, **GREEDY)
    prompt = repetitive_prompt(V_TINY, P_TINY, 3)
    run.prefill(prompt)
    for _ in range(3):
        run.step()
    question = torch.randint(3, V_TINY, (1, 9), generator=torch.Generator().manual_seed(4))
    run.extend(question, keep=P_TINY)                    # a follow-up on the document: the history is SET again
    check_invariant(run)
    assert run.eng.draft_cache.tokens() == prompt[0].tolist() + question[0].tolist()
    for _ in range(3):
        run.step()
        check_invariant(run)
    run.extend(question[:, :4])                          # a chat turn: pending token + ids behind everything generated
    check_invariant(run)
    run.step()
    check_invariant(run)


def test_forward_refuses_logits_and_a_foreign_cache():
    from triforce_amd.models.ngram_draft import NgramCache, NgramDraft
    d, c = NgramDraft(32, "cpu"), NgramCache(16, "cpu")
    ids = torch.tensor([[3]])
    with pytest.raises(NotImplementedError, match="no logits"):
        d.forward(ids, c, c, 0, probs=None)
    with pytest.raises(NotImplementedError, match="NgramCache"):
        d.forward(ids, object(), object(), 0, probs=(0.6, 0.9))
    out = d.forward(ids, c, c, 0, probs=(0.6, 0.9))
    assert out.logits is None and float(out.probs[3]) == 1.0 and d.eval() is d and d.config.vocab_size == 32
    with pytest.raises(ValueError, match="ngram_max"):
        NgramDraft(32, "cpu", ngram_max=9)


@pytest.mark.parametrize("script", ["offloading", "offloading_TP", "offloading_seqouia"])
def test_other_entry_points_refuse_the_ngram_draft_by_name(script):
    from triforce_amd.utils import cli
    with pytest.raises(NotImplementedError, match="--draft ngram"):
        cli.parse(script, ["--draft", "ngram"])
    assert cli.parse(script, []).draft == "llama-68M"    # the default is untouched
    args = cli.parse("on_chip", ["--draft", "ngram"])
    assert cli.is_ngram_draft(args) and args.ngram_max == 3
    assert not cli.is_ngram_draft(cli.parse("on_chip", [])) and cli.parse("on_chip", []).draft == "llama-68M"


def test_tensor_parallel_engine_refuses_the_ngram_draft():
    from triforce_amd.models.ngram_draft import NgramDraft, refuse_ngram_draft
    with pytest.raises(NotImplementedError, match="tensor-parallel"):
        refuse_ngram_draft(NgramDraft(32, "cpu"), "the tensor-parallel engine")
    refuse_ngram_draft(None, "x")
    refuse_ngram_draft("llama-68M", "x")
