"""Generate tests/golden/qk_norm_small.pt: ``transformers``' Qwen3ForCausalLM — the independent definition of an attention
layer with per-head q / k RMSNorm in front of the rotation — evaluated in float64 on two tiny models, on the CPU.

TEST INFRASTRUCTURE ONLY; needs ``transformers`` with Qwen3, so it runs where that is installed:
    python -m tools.gen_qk_norm_golden
For the tiny multi-head and the tiny grouped-query shape (vocabulary 1024, plain RoPE, theta 1e6) it builds the HF model
(eager attention, ``.double()``) from the seeded state dicts of tests/qk_norm_ref.py, runs a 200-token prompt and 7
teacher-forced decode steps through HF's own KV cache, and asserts that tests/qk_norm_ref.forward_fp64 gives the same logits
up to float64 rounding (bound 1e-8 on O(1) logits: both are float64 evaluations of one formula and differ in summation order
only, and any difference of DEFINITION — norm / rotation order, per-head scope, eps, weight placement — is many orders
larger).  Two numerical inputs of the path are not architecture and are handed to HF as data: the fp16-rounded RoPE tables and
the fp16-rounded softmax scale (oracle/ref_ops.py), which is what every model of this project computes with.
It also checks the YaRN-over-theta tables (llama_core.yarn_inv_freq with the model's rope_theta) against
transformers.modeling_rope_utils.ROPE_INIT_FUNCTIONS["yarn"].  The file stores seeds, HF's logits rows (fp32) and table
samples: no weights.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_ops as R, specs  # noqa: E402
from tests import qk_norm_ref as Q  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
VOCAB, PROMPT, DECODE, LAST = 1024, 200, 7, 8
FP64_BOUND = 1e-8
YARN = dict(factor=4.0, original_max_position_embeddings=32768, rope_theta=1e6, head_dim=128)


def case_spec(name, hidden, heads, kv_heads):
    tcfg = specs.llama_config(hidden, 768, 2, heads, vocab_size=VOCAB, max_position_embeddings=4096, rope_theta=1e6,
                              name=f"tiny-{name}-qknorm")
    tcfg.update(num_key_value_heads=kv_heads, qk_norm=True, model_type="qwen3")
    return dict(name=name, tcfg=tcfg, tseed=3001, nseed=3002, pseed=3003, head_std=0.05, norm_std=Q.QK_NORM_STD)


def ids_of(g):
    return specs.random_prompt(VOCAB, PROMPT + DECODE, g["pseed"])


def build_hf(cfg, sd):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    D = R.head_dim_of(cfg)
    hc = Qwen3Config(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                     num_hidden_layers=cfg["num_hidden_layers"], num_attention_heads=cfg["num_attention_heads"],
                     num_key_value_heads=cfg["num_key_value_heads"], head_dim=D, rms_norm_eps=cfg["rms_norm_eps"],
                     max_position_embeddings=cfg["max_position_embeddings"], attention_bias=False, tie_word_embeddings=False,
                     rope_parameters=dict(rope_type="default", rope_theta=cfg["rope_theta"]), attn_implementation="eager")
    model = Qwen3ForCausalLM(hc).double().eval()
    missing, unexpected = model.load_state_dict({k: v.double() for k, v in sd.items()}, strict=False)
    assert not unexpected and all("rotary_emb" in m for m in missing), (missing, unexpected)
    # data, not architecture: the path's fp16-rounded tables and softmax scale
    cos, sin = (t.double() for t in R.rope_tables_for(cfg))
    model.model.rotary_emb.forward = lambda x, position_ids: (cos[position_ids], sin[position_ids])
    for layer in model.model.layers:
        assert type(layer.self_attn.q_norm).__name__ == "Qwen3RMSNorm" and layer.self_attn.q_norm.weight.shape == (D,)
        layer.self_attn.scaling = float(R.softmax_scale_for(D))
    return model


class _Fp64Working:
    """HF's Qwen3 module computes its RMSNorm statistics and its softmax in torch.float32 whatever the model's dtype, which
    leaves a ``.double()`` model ~6e-7 from a float64 evaluation.  Inside this context the module's own name ``torch`` answers
    ``float32`` with float64: every line of HF's definition runs as written, at float64 working precision.  Validated against
    transformers 5.15.0, where modeling_qwen3 names torch.float32 in Qwen3RMSNorm.forward and eager_attention_forward only;
    another version may use it elsewhere — run_case records how far the as-shipped model is from this one, which would show."""

    class _Proxy:
        def __getattr__(self, name):
            return torch.float64 if name == "float32" else getattr(torch, name)

    def __enter__(self):
        from transformers.models.qwen3 import modeling_qwen3 as mq
        self.mq, self.saved = mq, mq.torch
        mq.torch = self._Proxy()

    def __exit__(self, *exc):
        self.mq.torch = self.saved


def hf_rows(model, ids):
    with torch.inference_mode():
        out = model(input_ids=ids[:, :PROMPT], use_cache=True)
        rows, past = [out.logits[0, -LAST:]], out.past_key_values
        for t in range(PROMPT, PROMPT + DECODE):
            out = model(input_ids=ids[:, t:t + 1], past_key_values=past, use_cache=True)
            rows.append(out.logits[0])
            past = out.past_key_values
    return torch.cat(rows)                                            # (LAST + DECODE, V) float64


def run_case(g):
    sd, _ = Q.state_dicts_of(g["tcfg"], g["tseed"], g["nseed"], g["head_std"])
    ids = ids_of(g)
    model = build_hf(g["tcfg"], sd)
    as_shipped = hf_rows(model, ids)                                  # fp32 statistics / softmax inside, as HF ships it
    with _Fp64Working():
        hf = hf_rows(model, ids)
    ours = Q.forward_fp64(g["tcfg"], sd, ids[0])[PROMPT - LAST:]
    dev = float((ours - hf).abs().max())
    assert dev < FP64_BOUND, f"[{g['name']}] forward_fp64 is {dev:.3e} from HF's float64 logits"
    # the norms are not decoration: the same matrices without them are somewhere else entirely
    plain = Q.forward_fp64(g["tcfg"], Q.without_norms(sd), ids[0])[PROMPT - LAST:]
    assert float((plain - hf).abs().max()) > 0.1, "norm-free logits too close: the check would be vacuous"
    shipped = float((as_shipped - hf).abs().max())
    print(f"[{g['name']}] forward_fp64 vs HF float64: max |d| = {dev:.3e} over {tuple(hf.shape)} logits, max |logit| = "
          f"{float(hf.abs().max()):.3f}; HF with its fp32 statistics and softmax is {shipped:.3e} from that")
    return dict(g, prompt_len=PROMPT, decode=DECODE, last=LAST, logits=hf.float().clone(), fp64_dev=dev, hf_fp32_dev=shipped)


def yarn_check():
    from transformers import Qwen3Config
    from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.llama_core import rope_tables_for, yarn_inv_freq
    D, f, orig, theta = YARN["head_dim"], YARN["factor"], YARN["original_max_position_embeddings"], YARN["rope_theta"]
    hc = Qwen3Config(hidden_size=2 * D, num_attention_heads=2, num_key_value_heads=2, head_dim=D,
                     max_position_embeddings=int(f * orig),
                     rope_parameters=dict(rope_type="yarn", factor=f, original_max_position_embeddings=orig, rope_theta=theta))
    inv_hf, att_hf = ROPE_INIT_FUNCTIONS["yarn"](hc, torch.device("cpu"))
    inv, att = yarn_inv_freq(D, f, orig, base=theta)
    rel = float(((inv.double() - inv_hf.double()).abs() / inv_hf.double()).max())
    assert torch.equal(inv, inv_hf.float()) and rel == 0.0 and abs(att - att_hf) < 1e-12, (rel, att, att_hf)
    cfg = LlamaConfig(hidden_size=2 * D, num_attention_heads=2, max_position_embeddings=int(f * orig), rope_theta=theta,
                      qk_norm=True, rope_scaling=dict(rope_type="yarn", factor=f, original_max_position_embeddings=orig))
    cos, sin = rope_tables_for(cfg)
    pos = torch.tensor([0, 1, 7, 1000, 32767, 32768, 100000, int(f * orig) - 1])
    fr = torch.outer(pos.float(), inv_hf.float())
    emb = torch.cat([fr, fr], dim=-1)
    want_c, want_s = (emb.cos() * att_hf).half(), (emb.sin() * att_hf).half()
    # the tables built from HF's frequencies and attention factor, the same fp32 way: bit-equal
    assert torch.equal(cos[pos], want_c) and torch.equal(sin[pos], want_s)
    dc = float((cos[pos].float() - want_c.float()).abs().max())
    base10k = yarn_inv_freq(D, f, orig)[0]
    assert float((base10k - inv).abs().max()) > 1e-3, "theta did not reach the tables"
    print(f"[yarn] inv_freq vs HF: max rel {rel:.3e}; attention factor {att:.12f} vs {att_hf:.12f}; table samples max |d| {dc:.3e}")
    return dict(YARN, positions=pos, cos=cos[pos].clone(), sin=sin[pos].clone(), inv_freq=inv_hf.float().clone(),
                attention_factor=float(att_hf), inv_freq_rel=rel)


def main():
    cases = [run_case(case_spec("mha", 256, 2, 2)), run_case(case_spec("gqa", 512, 4, 2))]
    path = os.path.join(GOLDEN, "qk_norm_small.pt")
    torch.save(dict(cases=cases, yarn=yarn_check(), fp64_bound=FP64_BOUND), path)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
