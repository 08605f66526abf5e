"""What the large-vocabulary sampling path costs.  HIP events, warm-up first, the forms of every comparison
alternated in one process, medians of --launches (>= 50).  One JSON line per measurement, appended to --out.
  (a) normaliser : tf_topp_probs_large / tf_topk_topp_probs_large (top_k = 50) against the route such logits took before — the
                   torch chain of utils.sampling (topk, stable sort, softmax, cumsum, scatter, softmax) — at rows 1 / 7 / 8 / 17,
                   V = 128 256 and 262 144, on sharp rows (one model-like peak) and N(0, 2.5) rows; at V = 32 000 against
                   tf_topp_probs (the price of streaming the row instead of holding it in LDS; routing never takes it there).
  (b) sampling   : tf_sample_inverse_cdf, tf_middle_accept_cur, tf_accept_chain_step at V = 128 256 from a 16-byte-aligned base
                   (16-byte loads, streamed twice) and from a base one float further (element by element).
  (c) decode     : TriForceRunner steps of tiny-v128k + its 68M-shaped draft (random weights, 2 048-token prompt), two engines
                   in one process in alternating blocks: this tree's routing, and the previous routing restated in this tree
                   (norm_logits through the torch chain above 32 768 entries, the draft issued from Python because the native
                   chain's top-p refused the vocabulary).
    python tools/large_vocab_bench.py --parts a,b,c [--out profiles/large_vocab_topp.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
DEV = "cuda:0"


def _emit(line, out):
    print(json.dumps(line), flush=True)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "a") as f:
            f.write(json.dumps(line) + "\n")


def _event_us(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3


def _alternate(forms, launches):
    for fn in forms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(launches):
        for k, fn in forms.items():
            times[k].append(_event_us(fn))
    return {k: (round(statistics.median(v), 2), round(min(v), 2)) for k, v in times.items()}


def _rows(kind, rows, V, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind == "sharp":                                    # what a language model emits: a few tokens carry the mass
        lg = torch.randn(rows, V, generator=gen)
        for r in range(rows):
            lg[r, torch.randperm(V, generator=gen)[:6]] += torch.tensor([14.0, 13.0, 12.0, 11.0, 10.0, 9.0])
        return lg
    return torch.randn(rows, V, generator=gen) * 2.5


def normaliser_part(a):
    from triforce_amd import ops
    from triforce_amd.utils import sampling as S

    def torch_route(lg, T, k, P):
        return torch.softmax(S.top_k_top_p_filter(lg / T, top_k=k, top_p=P), dim=-1)
    ops.TOPP_MULTI = False
    T, P = 0.6, 0.9
    for V in (32000, 128256, 262144):
        for rows in (1, 7, 8, 17):
            for kind in ("sharp", "sigma2.5"):
                lg = _rows(kind, rows, V, 10 * rows + V % 7).to(DEV)
                forms = {"large": lambda: ops.topp_probs_large(lg, T, P),
                         "large_top_k50": lambda: ops.topk_topp_probs_large(lg, T, 50, P)}
                if V <= ops.TOPP_MAX_VOCAB:
                    forms["tf_topp_probs"] = lambda: ops.topp_probs(lg, T, P)
                    forms["tf_topk_topp_probs_k50"] = lambda: ops.topk_topp_probs(lg, T, 50, P)
                else:
                    forms["torch_sort_chain"] = lambda: torch_route(lg, T, -1, P)
                    forms["torch_sort_chain_top_k50"] = lambda: torch_route(lg, T, 50, P)
                res = _alternate(forms, a.launches)
                _emit({"what": "temperature + top-p + softmax", "part": "a", "rows": rows, "V": V, "row_kind": kind, "T": T,
                       "top_p": P, "launches": a.launches, "median_us": {k: v[0] for k, v in res.items()},
                       "min_us": {k: v[1] for k, v in res.items()}}, a.out)


def sampling_part(a):
    from triforce_amd import ops
    V, gamma, g2 = 128256, 6, 6
    gen = torch.Generator().manual_seed(1)
    p = torch.rand(g2 + 1, V, generator=gen) * (0.4 / V) + 1e-9
    q = torch.rand(g2, V, generator=gen) * (0.4 / V) + 1e-9
    for r in range(g2 + 1):
        p[r, torch.randperm(V, generator=gen)[:40]] = 0.02
    for r in range(g2):
        q[r, torch.randperm(V, generator=gen)[:40]] = 0.02
    toks = [int(torch.nonzero(q[i] > 0.01)[3]) for i in range(g2)]

    def offset(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        return v
    forms = {}
    for label, conv in (("aligned", lambda t: t.to(DEV)), ("offset_by_one_float", offset)):
        dp, dq = conv(p), conv(q)
        u = torch.tensor([0.37], device=DEV)
        out = torch.zeros(4, dtype=torch.int64, device=DEV)
        ubuf = torch.full((64,), 0.41, device=DEV)
        cursor = torch.zeros(1, dtype=torch.int64, device=DEV)
        tokens = torch.tensor([9] + toks + [0], dtype=torch.int64, device=DEV)
        s_src = torch.tensor([100], dtype=torch.int32, device=DEV)

        def sample(dp=dp, u=u, out=out):
            ops.sample_inverse_cdf(dp[0], u, out[0:1])

        def middle(dp=dp, dq=dq, tokens=tokens, ubuf=ubuf, cursor=cursor, out=out):
            cursor.zero_()
            ops.middle_accept_cur(dp, dq[0], tokens, ubuf, cursor, 0, gamma, out)

        def chain(dp=dp, dq=dq, tokens=tokens, ubuf=ubuf, cursor=cursor, out=out, s_src=s_src):
            cursor.zero_()
            ops.accept_chain_step(dp, dq, tokens, ubuf, cursor, g2, False, 2, 0, s_src, [], out)
        forms.update({f"tf_sample_inverse_cdf/{label}": sample, f"tf_middle_accept_cur/{label}": middle,
                      f"tf_accept_chain_step/{label}": chain})
    res = _alternate(forms, a.launches)
    _emit({"what": "sampling / accept kernels (the cursor reset is one fill launch inside both timed forms)", "part": "b", "V": V,
           "launches": a.launches, "median_us": {k: v[0] for k, v in res.items()}, "min_us": {k: v[1] for k, v in res.items()}}, a.out)


def decode_part(a):
    from triforce_amd import ops
    from triforce_amd.models import zoo
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache, StreamingLLMEvictionCache
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as Draft
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.graph_infer import GraphInferenceEngine
    from triforce_amd.utils.sampling import UniformSource
    gamma, prefill, T, P = 6, 2048, 0.6, 0.9
    real_route = ops.topp_route

    def old_route(V, top_p, is_device=True, dtype=torch.float32):
        r = real_route(V, top_p, is_device, dtype)
        return "torch" if r == "large" else r

    class Tok:
        eos_token_id = 2

        def decode(self, ids, **kw):
            return ""

    def build(old):
        ops.topp_route = old_route if old else real_route
        os.environ["TRIFORCE_DRAFT_NATIVE"] = "0" if old else "1"
        target = LlamaForCausalLM.from_pretrained("random:1", torch_dtype=torch.float16, device_map=DEV,
                                                  config=zoo.config("tiny-v128k")).eval()
        draft = Draft.from_pretrained("random:1", torch_dtype=torch.float16, device_map=DEV,
                                      config=zoo.config(zoo.draft_for("tiny-v128k"))).eval()
        ge = GraphInferenceEngine(target, FlashSimpleCache(target, prefill + 4096), RetrievalCache(target, max_budget=2048, prefill=prefill, gamma=gamma, chunk_size=8),
                                  draft, StreamingLLMEvictionCache(draft, start_size=16, recent_size=256 - 16 - gamma, gamma=gamma))
        ge.initialize_cuda_graph(gamma, probs=True, temperature=T, top_p=P, verbose=False)
        run = TriForceRunner(Tok(), ge, gamma, top_p=P, temperature=T, rng=UniformSource(DEV, seed=3))
        ids = torch.randint(3, 128256, (1, prefill), generator=torch.Generator().manual_seed(0)).to(DEV)
        run.prefill(ids)
        for _ in range(4):
            run.step()
        return run
    runs = {"this_tree": build(False), "previous_routing": build(True)}
    ms = {k: [] for k in runs}
    for _ in range(a.blocks):
        for k, run in runs.items():                      # alternated blocks; the routing is looked up per call
            ops.topp_route = old_route if k == "previous_routing" else real_route
            torch.cuda.synchronize()
            n0 = run.n
            t = _event_us(lambda: [run.step() for _ in range(a.block_steps)]) / 1e3 / a.block_steps
            ms[k].append((round(t, 3), (run.n - n0) / a.block_steps))
    ops.topp_route = real_route
    _emit({"what": "TriForceRunner steps, tiny-v128k + 68M-shaped draft, random weights, prefill 2048, gamma 6", "part": "c",
           "blocks": a.blocks, "block_steps": a.block_steps,
           "step_set_up_on_device": {k: r._device_sets() is not None for k, r in runs.items()},
           "ms_per_step": {k: [x[0] for x in v] for k, v in ms.items()},
           "median_ms_per_step": {k: round(statistics.median(x[0] for x in v), 3) for k, v in ms.items()},
           "tokens_per_step": {k: round(statistics.mean(x[1] for x in v), 2) for k, v in ms.items()}}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parts = set(a.parts.split(","))
    assert parts <= {"a", "b", "c"} and a.launches >= 50
    if "a" in parts:
        normaliser_part(a)
    if "b" in parts:
        sampling_part(a)
    if "c" in parts:
        decode_part(a)


if __name__ == "__main__":
    main()
