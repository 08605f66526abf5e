"""Generate tests/golden/attn_bias_small.pt: the UNMODIFIED reference built with ``attention_bias=True`` on two tiny
multi-head targets — q/k/v/o biases, and q/k/v biases with a zero o_proj bias (the Qwen2 form) — run on the CPU.

TEST INFRASTRUCTURE ONLY; needs the reference tree (oracle/_refshim.py), so it runs in the build container:
    python -m tools.gen_attn_bias_golden
For each case it records the logits of a chunked prefill + one decode step, the greedy Autoregressive stream and the greedy
TriForce stream, and asserts that the restatement tests/attn_bias_ref.BiasedOracleTarget reproduces them (logits bit-identical,
streams identical) — which is how oracle/gen_golden.py pins the oracle.  The file stores seeds, not weights.  The reference's
retrieval cache is multi-head only, so there is no grouped-query case; the tests derive that one from the expanded state dict.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import _refshim, specs, ref_model as M  # noqa: E402
from oracle.gen_golden import build_reference_model  # noqa: E402
from tests import attn_bias_ref as B  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
VOCAB = 1024


def case_spec(name, zero_o):
    """The zoo's "tiny" target shape (hidden 256, 2 heads of 128, 2 layers) at a 1024-entry vocabulary, tiny draft."""
    tcfg = specs.llama_config(256, 768, 2, 2, vocab_size=VOCAB, max_position_embeddings=4096,
                              rope_scaling=dict(type="yarn", factor=16.0, original_max_position_embeddings=256),
                              name="tiny-yarn-bias-target")
    tcfg["attention_bias"] = True
    dcfg = specs.llama_config(128, 256, 2, 2, vocab_size=VOCAB, max_position_embeddings=2048, name="tiny-draft")
    return dict(name=name, tcfg=tcfg, dcfg=dcfg, tseed=2901, dseed=2902, pseed=2903, bseed=2904, zero_o=zero_o, head_std=0.05,
                bias_std=B.BIAS_STD, prefill=512, budget=128, gamma=6, chunk=8, gen_len=24, temperature=1.0, top_p=1e-9)


def state_dicts(g):
    """(target state dict as the reference's module takes it — an o_proj bias always, zeros in the Qwen2 form —, draft)."""
    tsd = specs.random_state_dict(g["tcfg"], g["tseed"], head_std=g["head_std"])
    tsd = B.add_biases(g["tcfg"], tsd, g["bseed"], std=g["bias_std"], zero_o=g["zero_o"])
    return tsd, specs.random_state_dict(g["dcfg"], g["dseed"], head_std=g["head_std"])


def run_case(ref, g):
    tsd, dsd = state_dicts(g)
    prompt = specs.random_prompt(VOCAB, g["prefill"], g["pseed"])
    gamma, recent = g["gamma"], 256 - 16 - g["gamma"]
    target = build_reference_model(ref, g["tcfg"], tsd)
    for layer in target.model.layers:                                   # the reference really built biased projections
        assert all(getattr(layer.self_attn, n).bias is not None for n in B.PROJ)
    draft = build_reference_model(ref, g["dcfg"], dsd, draft=True)
    cache = ref.cache.FlashSimpleCache(target, g["prefill"] + g["gen_len"] + 16)
    gcache = ref.cache.RetrievalCache(target, max_budget=g["budget"], prefill=g["prefill"], gamma=gamma, chunk_size=g["chunk"])
    dcache = ref.cache.StreamingLLMEvictionCache(draft, start_size=16, recent_size=recent, gamma=gamma)
    eng = _refshim.EagerEngine(ref, target, cache, gcache, draft, dcache, g["temperature"], g["top_p"])
    tok = _refshim.FakeTokenizer()

    # -- logits: a chunked prefill of 200 tokens, then one decode step
    with torch.inference_mode():
        l1 = target(input_ids=prompt[:, :128], kv_cache=cache, graph_cache=None).logits
        l2 = target(input_ids=prompt[:, 128:200], kv_cache=cache, graph_cache=None).logits
        l3 = target(input_ids=prompt[:, 200:201], kv_cache=cache, graph_cache=None).logits
    oeng = B.build_oracle(g, tsd, dsd)
    o1 = oeng.model.forward(prompt[:, :128], oeng.kv_cache)
    o2 = oeng.model.forward(prompt[:, 128:200], oeng.kv_cache)
    o3 = oeng.model.forward(prompt[:, 200:201], oeng.kv_cache)
    assert torch.equal(l1, o1) and torch.equal(l2, o2) and torch.equal(l3, o3), f"[{g['name']}] restatement logits differ"
    # the biases matter: the bias-free oracle on the same weights is somewhere else entirely
    plain = M.OracleTarget(g["tcfg"], tsd).forward(prompt[:, :128], M.FullCache(g["tcfg"], 256))
    assert float((plain - o1).abs().max()) > 0.1, "biases too small to matter"
    cache.reset()

    # -- greedy streams
    emitted = []
    orig_stream = ref.decoding.spec_stream
    ref.decoding.spec_stream = lambda t, tokenizer, color="blue": emitted.append(int(torch.as_tensor(t).reshape(-1)[0]))
    try:
        ref.decoding.Autoregressive(tok, eng, prompt, max_len=g["gen_len"], top_k=-1, top_p=g["top_p"],
                                    temperature=g["temperature"], verbose=True)
        ar = list(emitted)
        emitted.clear()
        acc, _ = ref.decoding.TriForce(tok, eng, prompt, gamma=gamma, max_len=g["gen_len"], top_k=-1, top_p=g["top_p"],
                                       temperature=g["temperature"], verbose=True)
        tf = list(emitted)
    finally:
        ref.decoding.spec_stream = orig_stream
    o_ar = M.autoregressive(oeng, prompt, g["gen_len"], g["temperature"], g["top_p"])
    assert o_ar == ar, f"[{g['name']}] AR stream mismatch\n{o_ar}\n{ar}"
    res = M.triforce(oeng, prompt, gamma, g["gen_len"], g["temperature"], g["top_p"])
    assert res["tokens"] == tf, f"[{g['name']}] TriForce stream mismatch\n{res['tokens']}\n{tf}"
    n = min(len(ar), len(tf))
    assert tf[:n] == ar[:n], "greedy invariant violated"
    print(f"[{g['name']}] ok: {len(ar)} AR tokens, {len(tf)} TriForce tokens, acceptance {acc:.3f}")
    return dict(g, logits=[l1[0, -1].clone(), l2[0, -1].clone(), l3[0, -1].clone()], ar_tokens=ar, triforce_tokens=tf,
                acceptance_rate=float(acc))


def main():
    ref = _refshim.load_reference()
    cases = [run_case(ref, case_spec("mha_qkvo", zero_o=False)), run_case(ref, case_spec("mha_qkv_zero_o", zero_o=True))]
    path = os.path.join(GOLDEN, "attn_bias_small.pt")
    torch.save(dict(cases=cases), path)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
