"""End-to-end parity on a real MI355X: the product engine (HIP kernels through the C ABI, hipGraph
replay) against the CPU oracle and the golden fixtures recorded from the reference.

Greedy bar (north star): token-for-token equal to the reference's CPU/eager path at temp=0.  fp32
accumulation order differs between devices — and between HOST CPUs: the oracle run on the GPU box's CPU
does not reproduce, bit for bit, a 40-token golden stream recorded on the build container's CPU — so the
device-independent form of the criterion is teacher-forced: every token the device emits must be the
oracle's argmax given the same prefix (up to GAP_TOL of logit where two logits are within fp16 noise),
and the stream must share a long prefix with the golden one.
"""
import pytest
import torch

from oracle import ref_model as M
from oracle import ref_ops as R
from oracle import specs
from tests import helpers as Hh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# Logit bar: the north star's "within 1e-3 fp16" is one fp16 spacing (2^-10) at |x| in [1,2).  Logits ARE fp16
# values (lm_head output cast to float), so the resolution-aware form of that bar is: no logit further than
# 2 fp16 spacings at the largest logit magnitude of the tensor (3.9e-3 for max|x| in [2,4)), never below 1e-3,
# and the mean deviation below 1e-3.
LOGIT_MEAN_TOL = 1e-3
GAP_TOL = 8e-3        # an emitted token's oracle logit may trail the oracle's best by at most ~2 fp16 spacings


def _logit_check(what, got, want, spacings=2.0):
    import math
    d = (got - want).abs()
    mag = max(1.0, float(want.abs().max()))
    bound = max(1e-3, spacings * 2.0 ** (math.floor(math.log2(mag)) - 10))
    Hh.record("logit_check", float(d.max()) / bound, what=what, max_abs=float(d.max()), mean_abs=float(d.mean()), bound=bound,
              mean_bound=LOGIT_MEAN_TOL, mean_used=float(d.mean()) / LOGIT_MEAN_TOL, max_ref=mag, spacings=spacings)
    assert d.max() <= bound and d.mean() < LOGIT_MEAN_TOL, \
        f"{what}: max |dlogit| {d.max():.2e} (bound {bound:.2e}), mean {d.mean():.2e}"


@pytest.mark.parametrize("name", ["small_gamma6", "cfg1_greedy"])
@pytest.mark.parametrize("graphs", [False, True])
def test_greedy_triforce_matches_reference_golden(name, graphs):
    from triforce_amd.utils.decoding import Autoregressive, TriForce
    g = Hh.load_golden(name)
    ge = Hh.build_product(g, DEV, graphs=graphs)
    prompt = Hh.prompt_of(g).to(DEV)
    tok = Hh.FakeTokenizer()
    _, ar = Autoregressive(tok, ge, prompt, max_len=g["gen_len"], top_k=-1, top_p=g["top_p"],
                           temperature=g["temperature"], return_tokens=True)
    res = TriForce(tok, ge, prompt, gamma=g["gamma"], max_len=g["gen_len"], top_k=-1, top_p=g["top_p"],
                   temperature=g["temperature"], return_details=True)
    for what, stream in (("autoregressive", ar), ("triforce", res["tokens"])):
        gaps = Hh.teacher_forced_gaps(g, stream)
        worst = max(gaps)
        assert worst < GAP_TOL, f"{what}: token {gaps.index(worst)} trails the oracle argmax by {worst:.4f} logit"
        exact = sum(1 for x in gaps if x == 0.0)
        assert exact >= len(gaps) - 3, f"{what}: only {exact}/{len(gaps)} tokens are the oracle's exact argmax"
    gold_ar, gold_tf = g["ar_tokens"], g["triforce"][0]["tokens"]
    assert Hh.common_prefix(ar, gold_ar) >= min(16, len(ar)), (ar[:24], gold_ar[:24])
    assert Hh.common_prefix(res["tokens"], gold_tf) >= min(16, len(gold_tf)), (res["tokens"][:24], gold_tf[:24])
    # lossless on the device itself: greedy TriForce and greedy AR come from the same kernels
    n = min(len(ar), len(res["tokens"]))
    assert Hh.common_prefix(ar[:n], res["tokens"][:n]) >= min(16, n)
    m = min(len(res["tokens"]), len(gold_tf))
    if res["tokens"][:m] == gold_tf[:m]:
        k = min(len(res["counts"]), len(g["counts"][0]))
        assert res["counts"][:k - 1] == g["counts"][0][:k - 1]            # identical accept/rollback trace
    # second prompt on the same engine: exercises update_graph_cache_retrieval and the draft seq_len quirk
    res2 = TriForce(tok, ge, prompt, gamma=g["gamma"], max_len=16, top_k=-1, top_p=g["top_p"],
                    temperature=g["temperature"], return_details=True)
    assert max(Hh.teacher_forced_gaps(g, res2["tokens"])) < GAP_TOL
    assert Hh.common_prefix(res2["tokens"], g["triforce"][-1]["tokens"]) >= 8


@pytest.mark.parametrize("name", ["small_gamma6", "cfg1_greedy"])
def test_logits_and_retrieval_stages_match_oracle(name):
    """Stage-wise parity (SURVEY §7 'Tie-breaking'): prefill logits, retrieval scores, top-k given the device's
    own scores (bit-exact vs the oracle rule), gathered cache (bit-exact given indices), spec-forward logits
    given an identical retrieval cache, draft probabilities."""
    g = Hh.load_golden(name)
    oeng, tsd, dsd = Hh.build_oracle(g)
    ge = Hh.build_product(g, DEV, tsd, dsd)
    prompt = Hh.prompt_of(g)
    oeng.inference(prompt[:, :-1])
    lo = oeng.inference(prompt[:, -1:])
    ge.inference(prompt[:, :-1].to(DEV))
    lp = ge.inference(prompt[:, -1:].to(DEV)).cpu()
    _logit_check("prefill logits", lp, lo)
    pk = ge.engine.kv_cache.k.permute(0, 2, 1, 3).cpu()[:, :g["prefill"]]
    dk = (pk.float() - oeng.kv_cache.key_cache[:, :g["prefill"]].float()).abs()
    assert Hh.bound("prefill: cached keys, max", dk.max(), 8e-3) and Hh.bound("prefill: cached keys, mean", dk.mean(), 2e-4), f"cached keys: max {dk.max():.2e} mean {dk.mean():.2e}"
    pg, og = ge.engine.graph_cache, oeng.graph_cache
    for l in range(og.layers):
        dev_scores = pg.last_scores[l].cpu()
        ds = (dev_scores.float() - og.last_scores[l].float()).abs()
        assert Hh.bound("retrieval scores (fp16 dot of a chunk mean)", ds.max(), 8e-3), f"layer {l} retrieval scores differ by {ds.max():.3e}"
        # top-k: exact w.r.t. the scores the device itself produced
        assert torch.equal(pg.last_idx[l].cpu().long(), R.retrieval_topk(dev_scores, og.select_sets))
        # gather: exact w.r.t. the device's indices and the device's own full cache
        full_k = ge.engine.kv_cache.k[l].permute(1, 0, 2).cpu()
        want = R.retrieval_gather(full_k[:g["prefill"]], pg.last_idx[l].cpu().long(), g["chunk"])
        assert torch.equal(pg.k[l, :, :g["budget"]].permute(1, 0, 2).cpu(), want)
    # spec forward given an identical retrieval cache: overwrite the device caches with the oracle's
    pg.k.copy_(og.key_cache.permute(0, 2, 1, 3))
    pg.v.copy_(og.value_cache.permute(0, 2, 1, 3))
    gamma = g["gamma"]
    vt = torch.tensor([[11, 12, 13] + [100] * (gamma - 2)])
    S = oeng.kv_cache.seq_len
    pos = torch.arange(S, S + gamma + 1).unsqueeze(0)
    so = oeng.model.forward(vt, oeng.kv_cache, og, position_ids=pos, spec=True)
    sp = ge.engine.model(input_ids=vt.to(DEV), kv_cache=ge.engine.kv_cache, graph_cache=pg, position_ids=pos.to(DEV),
                         spec=True).logits.cpu()
    _logit_check("spec logits", sp, so)
    # draft: prefill + one spec step
    oeng.graph_draft_prefill(prompt)
    ge.graph_draft_prefill(prompt.to(DEV))
    qo = oeng.graph_draft_inference(vt[:, :3], gamma_offset=2)
    qp = ge.graph_draft_inference(vt[:, :3].to(DEV), gamma_offset=2).cpu()
    assert Hh.bound("draft probability row (top-p)", (qo - qp).abs().max(), 5e-4), f"draft probs differ by {(qo - qp).abs().max():.3e}"


def test_native_draft_forward_is_bit_identical_to_the_op_by_op_chain(monkeypatch):
    """tf_draft_forward_68m (one C call issuing the whole 68M forward: embedding + positions, 2 x 5 layer launches,
    lm_head, top-p) against the same forward issued entry point by entry point from Python: decode steps over a warm
    StreamingLLM cache, every speculative offset, logits, probability rows and the K / V rows written — all bit for bit;
    and replayed from a hipGraph."""
    from oracle import specs
    from triforce_amd.models.cache import StreamingLLMEvictionCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as Draft
    g = Hh.load_golden("small_gamma6")
    gamma = g["gamma"]
    dsd = specs.random_state_dict(g["dcfg"], g["dseed"], head_std=g["head_std"])
    cfg = LlamaConfig.from_dict(g["dcfg"])

    def run(native):
        monkeypatch.setenv("TRIFORCE_DRAFT_NATIVE", "1" if native else "0")
        m = Draft.from_state_dict(cfg, dsd, DEV)
        c = StreamingLLMEvictionCache(m, start_size=16, recent_size=256 - 16 - gamma, gamma=gamma)
        assert (m._native_model() is not None) == native
        gen = torch.Generator().manual_seed(5)
        outs = []
        for n in (20, 7, 1):                                           # non-speculative appends (<= 32 rows each)
            ids = torch.randint(3, cfg.vocab_size, (1, n), generator=gen).to(DEV)
            outs.append(m.forward(ids, c, None, -1).logits)
        for off in range(gamma + 3):                                   # speculative steps at every offset, with top-p
            ids = torch.randint(3, cfg.vocab_size, (1, off + 1), generator=gen).to(DEV)
            o = m.forward(ids, c, c, off, probs=(0.6, 0.9))
            outs += [o.logits, o.probs]
        torch.cuda.synchronize()
        return m, c, outs

    m0, c0, ref = run(False)
    m1, c1, got = run(True)
    assert len(ref) == len(got)
    for a, b in zip(ref, got):
        assert a.shape == b.shape and torch.equal(a, b)
    assert torch.equal(c0.k, c1.k) and torch.equal(c0.v, c1.v) and c0.seq_len == c1.seq_len
    # graph replay of the native call
    ids = torch.randint(3, cfg.vocab_size, (1, 3)).to(DEV)
    want = m0.forward(ids, c0, c0, 2, probs=(0.6, 0.9))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m1.forward(ids, c1, c1, 2, probs=(0.6, 0.9))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = m1.forward(ids, c1, c1, 2, probs=(0.6, 0.9))
    for _ in range(2):
        cap.logits.zero_()
        cap.probs.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap.logits, want.logits) and torch.equal(cap.probs, want.probs)


def test_periodic_retrieval_rebuild_stays_lossless_on_device():
    """--rebuild_every: re-selecting the retrieval chunks inside a target verify changes what the
    middle model drafts from, never what the target accepts — the greedy stream stays on the oracle's argmax path,
    and the rebuilt slots hold exactly the chunks the fresh index names."""
    from triforce_amd.utils.decoding import TriForce
    g = Hh.load_golden("small_gamma6")
    ge = Hh.build_product(g, DEV, graphs=True)
    prompt, tok = Hh.prompt_of(g).to(DEV), Hh.FakeTokenizer()
    res = TriForce(tok, ge, prompt, gamma=g["gamma"], max_len=g["gen_len"], top_k=-1, top_p=g["top_p"],
                   temperature=g["temperature"], return_details=True, rebuild_every=2)
    assert max(Hh.teacher_forced_gaps(g, res["tokens"])) < GAP_TOL
    assert Hh.common_prefix(res["tokens"], g["ar_tokens"]) >= min(16, len(res["tokens"]))
    rc, kv = ge.engine.graph_cache, ge.engine.kv_cache
    gen, cs = kv.seq_len - rc.prefill, rc.chunk_size
    keep = min(rc.select_sets, (rc.max_budget - gen) // cs)               # sets not overwritten by the generated tail
    for layer in (0, rc.layers - 1):
        idx = rc.last_idx[layer].long()[:, :keep]                         # (H, keep)
        src_k, src_v = kv.layer_kv(layer)
        rows = (idx.unsqueeze(-1) * cs + torch.arange(cs, device=DEV)).reshape(rc.num_heads, -1)   # (H, keep*cs)
        pick = rows.unsqueeze(-1).expand(-1, -1, rc.head_dim)
        assert torch.equal(rc.k[layer, :, :keep * cs], src_k.gather(1, pick))
        assert torch.equal(rc.v[layer, :, :keep * cs], src_v.gather(1, pick))


def test_stochastic_triforce_with_injected_uniforms():
    """cfg3-style sampling (T=0.6, top_p=0.9) over 128 uniform streams (round 3: 32 — the paired bias then sat at +1.6
    standard errors on both metrics, the sign a subtle accept-test difference would have; the verdict asked for >= 128),
    product and oracle consuming the same explicit uniforms.  The oracle's runs are cached (tests/golden/
    stochastic_oracle_runs.json, written by oracle/gen_stochastic_runs.py from the pinned CPU oracle: the GPU box then
    spends no time on the CPU side); four of them are re-run live here and any difference from the cache — the GPU box's
    host CPU may order its fp32 GEMM sums differently — is written to the parity notes.  Every accept / resample decision is a bit-exact function of (p, q, r) (tests/test_gpu_ops.py), but an
    inverse-CDF draw from ~1000 comparably likely tokens flips as soon as the device's probabilities (fp16 logits:
    ~1e-3 relative) move a CDF boundary across the uniform — measured: a stream survives 5 draws at the median — after
    which the two runs are different draws from the same distributions.  So the end-to-end claim is distributional:
      * the first token (one draw from the prefill distribution) agrees in almost every run, and runs share a prefix;
      * acceptance and tokens per outer step, run by run against the oracle's run on the same uniforms: the mean of the
        paired differences stays within 4 standard errors of zero (accepted counts within a step are correlated, so the
        spread is taken from the runs themselves, not from a binomial formula), and the pooled values within 20 %
        (a wrong sampler or accept rule moves both far outside)."""
    import math
    from triforce_amd.utils.decoding import TriForce
    from triforce_amd.utils.sampling import UniformSource
    g = Hh.load_golden("small_gamma6")
    oeng, tsd, dsd = Hh.build_oracle(g, temperature=0.6, top_p=0.9)
    ge = Hh.build_product(g, DEV, tsd, dsd, temperature=0.6, top_p=0.9, graphs=True)
    prompt = Hh.prompt_of(g)
    runs, max_len = 128, 24
    import json
    import os
    cached = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "stochastic_oracle_runs.json")))
    assert cached["max_len"] == max_len and cached["gamma"] == g["gamma"] and len(cached["runs"]) >= runs
    prefixes, d_acc, d_tok = [], [], []
    acc_w = dr_w = acc_g = dr_g = tok_w = tok_g = steps_w = steps_g = 0
    for seed in range(runs):
        us = Hh.fixed_uniforms(n=2048, seed=500 + seed)
        c = cached["runs"][seed]
        assert c["seed"] == 500 + seed
        want = {"tokens": c["tokens"], "accepted": c["accepted"], "drafted": c["drafted"], "n": c["n"],
                "counts": [0] * c["steps"]}
        if seed % 37 == 0:                                # the cache is the oracle: spot-check it live
            live = M.triforce(oeng, prompt, g["gamma"], max_len, 0.6, 0.9, rng=M.InjectedRng(us))
            if (live["accepted"], live["drafted"], live["n"]) != (c["accepted"], c["drafted"], c["n"]):
                Hh.note(f"stochastic: live oracle run {seed} differs from the cached one (host-CPU GEMM order): "
                        f"{(live['accepted'], live['drafted'], live['n'])} vs {(c['accepted'], c['drafted'], c['n'])}")
        got = TriForce(Hh.FakeTokenizer(), ge, prompt.to(DEV), gamma=g["gamma"], max_len=max_len, top_k=-1, top_p=0.9,
                       temperature=0.6, rng=UniformSource(DEV, values=us), return_details=True)
        n = min(len(got["tokens"]), len(want["tokens"]))
        prefixes.append(Hh.common_prefix(got["tokens"][:n], want["tokens"][:n]))
        acc_w, dr_w = acc_w + want["accepted"], dr_w + want["drafted"]
        acc_g, dr_g = acc_g + got["accepted"], dr_g + got["drafted"]
        tok_w, steps_w = tok_w + want["n"], steps_w + len(want["counts"])
        tok_g, steps_g = tok_g + got["n"], steps_g + len(got["counts"])
        d_acc.append(got["accepted"] / max(got["drafted"], 1) - want["accepted"] / max(want["drafted"], 1))
        d_tok.append(got["n"] / len(got["counts"]) - want["n"] / len(want["counts"]))
    Hh.note(f"stochastic common prefixes (of {max_len}+ tokens, {runs} runs): {sorted(prefixes)}")
    assert sum(1 for c in prefixes if c >= 1) >= runs - 3, prefixes          # the first draw agrees (near-)always
    assert sum(prefixes) / runs >= 3.0, prefixes
    for what, d in (("acceptance", d_acc), ("tokens per step", d_tok)):
        mean = sum(d) / runs
        se = math.sqrt(sum((x - mean) ** 2 for x in d) / (runs - 1) / runs)
        Hh.note(f"stochastic {what}: mean paired difference {mean:+.4f} +- {se:.4f} (standard error)")
        assert abs(mean) <= 4 * se + 1e-9, (what, mean, se)
    p_w, p_g = acc_w / dr_w, acc_g / dr_g
    per_w, per_g = tok_w / steps_w, tok_g / steps_g
    Hh.note(f"stochastic pooled acceptance device {p_g:.3f} vs oracle {p_w:.3f}; tokens/step {per_g:.2f} vs {per_w:.2f}")
    assert abs(p_g - p_w) <= 0.2 * max(p_w, 0.05) + 0.02 and abs(per_g - per_w) <= 0.2 * per_w
    assert acc_g > 0


def test_expected_acceptance_at_identical_states_matches_the_oracle():
    """The sampling-free companion of the stochastic test above (round-3 verdict: its paired bias sat at +1.6 standard
    errors on both metrics — is the device's accept test subtly more generous?).  Device and oracle are walked through
    the SAME states — same prompt, same teacher-forced tokens (the oracle's most likely draft / follow-up token at every
    step) — and the quantity the accept tests are draws from is compared directly:
        inner loop   alpha_1(n) = sum_v min(p_retrieval[n][v], q_draft[v])     (decoding.py:190-193)
        outer loop   alpha_2(i) = sum_v min(p_target[i][v], p_retrieval[i][v]) (decoding.py:97-99)
    i.e. the probability that a draft from that distribution is accepted.  No uniforms, no trajectories that diverge: a
    device whose probabilities made acceptance likelier would show here as a mean difference far above fp16 noise."""
    from triforce_amd.utils.decoding import TriForceRunner
    g = Hh.load_golden("small_gamma6")
    oeng, tsd, dsd = Hh.build_oracle(g, temperature=0.6, top_p=0.9)
    ge = Hh.build_product(g, DEV, tsd, dsd, temperature=0.6, top_p=0.9, graphs=False)
    gamma, V = g["gamma"], g["tcfg"]["vocab_size"]
    d1, d2 = [], []
    for ps in range(6):
        prompt = specs.random_prompt(V, g["prefill"], g["pseed"] + 17 * ps)
        # the reference's prefill protocol on both sides (decoding.py:44-62)
        oeng.kv_cache.reset(); oeng.graph_cache.reset(); oeng.draft_cache.reset()
        oeng.inference(prompt[:, :-1])
        ologits = oeng.inference(prompt[:, -1:])
        oeng.graph_draft_prefill(prompt)
        run = TriForceRunner(Hh.FakeTokenizer(), ge, gamma, -1, 0.9, 0.6)
        pd = prompt.to(DEV)
        eng = ge.engine
        eng.kv_cache.reset(); eng.graph_cache.reset(); eng.draft_cache.reset()
        ge.inference(input_ids=pd[:, :-1])
        ge.inference(input_ids=pd[:, -1:])
        ge.graph_draft_prefill(input_ids=pd)
        nxt = int(ologits[0, -1].argmax())
        S = oeng.kv_cache.seq_len
        assert eng.kv_cache.seq_len == S
        vt = torch.full((1, gamma + 1), 100, dtype=torch.long)
        vt[0, 0] = nxt
        pos = torch.arange(S, S + gamma + 1).unsqueeze(0)
        rows_o, rows_d = [], []
        for n in range(gamma):                               # every iteration "rejects": one position per iteration
            qo = oeng.graph_draft_inference(vt[:, :n + 1], gamma_offset=n)
            qd = ge.graph_draft_inference(input_ids=vt[:, :n + 1].to(DEV), gamma_offset=n).float().cpu()
            vt[0, n + 1] = int(qo.argmax())                  # the drafted token both sides verify
            po = oeng.graph_verify(vt, pos)
            pdv = ge.graph_verify(input_ids=vt.to(DEV), position_ids=pos.to(DEV)).float().cpu()
            d1.append(float(torch.minimum(pdv[n], qd).sum() - torch.minimum(po[n], qo).sum()))
            rows_o.append(po[n]); rows_d.append(pdv[n])
            vt[0, n + 1] = int(po[n].argmax())               # follow-up token of a rejection: the position is decided
        ids = vt[:, :gamma + 1]
        lo = oeng.inference(ids)
        po_full = R.norm_logits(lo[0], 0.6, -1, 0.9)
        pd_full = ge.verify_probs(ids.to(DEV), 0.6, 0.9).float().cpu()
        for i in range(gamma):
            d2.append(float(torch.minimum(pd_full[i], rows_d[i]).sum() - torch.minimum(po_full[i], rows_o[i]).sum()))
    for what, d in (("inner (draft vs retrieval model)", d1), ("outer (retrieval vs full-cache model)", d2)):
        t = torch.tensor(d)
        Hh.note(f"expected acceptance at identical states, {what}: device - oracle over {len(d)} positions: mean "
                f"{float(t.mean()):+.5f}, max |d| {float(t.abs().max()):.5f}")
        assert abs(float(t.mean())) < 5e-3 and float(t.abs().max()) < 5e-2, (what, d)


def test_greedy_divergence_from_golden_happens_only_at_near_ties():
    """Where (if anywhere) the device's greedy stream leaves the reference's golden stream, the ORACLE itself must see a
    near-tie there: its logits for the two candidate tokens, given the common prefix, differ by less than one fp16
    spacing of their magnitude.  Reports the full-stream common prefix."""
    import math
    from triforce_amd.utils.decoding import TriForce
    for name in ("small_gamma6", "cfg1_greedy"):
        g = Hh.load_golden(name)
        ge = Hh.build_product(g, DEV, graphs=True)
        res = TriForce(Hh.FakeTokenizer(), ge, Hh.prompt_of(g).to(DEV), gamma=g["gamma"], max_len=g["gen_len"], top_k=-1,
                       top_p=g["top_p"], temperature=g["temperature"], return_details=True)
        gold, dev = g["triforce"][0]["tokens"], res["tokens"]
        n = min(len(gold), len(dev))
        common = Hh.common_prefix(dev[:n], gold[:n])
        Hh.note(f"{name}: device greedy stream == golden stream for {common}/{n} tokens")
        if common == n:
            continue
        eng, _, _ = Hh.build_oracle(g)
        prompt = Hh.prompt_of(g)
        eng.kv_cache.reset()
        logits = eng.inference(prompt)[0, -1]
        for i in range(common - 1):                                  # oracle forced along the common prefix
            logits = eng.model.forward(torch.tensor([[dev[i]]]), eng.kv_cache, None)[0, -1]
        if common > 0:
            logits = eng.model.forward(torch.tensor([[dev[common - 1]]]), eng.kv_cache, None)[0, -1]
        a, b = float(logits[dev[common]]), float(logits[gold[common]])
        spacing = 2.0 ** (math.floor(math.log2(max(abs(a), abs(b), 2.0 ** -14))) - 10)
        assert abs(a - b) <= spacing, (f"{name}: streams split at token {common} ({dev[common]} vs {gold[common]}) where "
                                       f"the oracle's logits differ by {abs(a - b):.5f} > one fp16 spacing {spacing:.5f}")


def test_7b_dimension_layer_logits_match_oracle():
    """One decoder layer at the 7B's real widths (hidden 4096, 32 heads x 128, intermediate 11008, vocabulary 32000,
    YaRN tables) over a 4 103-slot retrieval cache: the fused decode kernels (norm / RoPE / residual epilogues, split-KV
    attention, fp32-out lm_head) against the oracle's op-by-op forward, at the logit bar of the small configs."""
    from oracle import specs
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    cfg = specs.llama2_7b_128k_config()
    cfg["num_hidden_layers"] = 1
    sd = specs.random_state_dict(cfg, 31)                 # N(0, 0.02) everywhere: logits ~N(0, 1.3^2) like the 7B bench
    gamma, budget, prefill = 6, 4096, 8192
    ot = M.OracleTarget(cfg, sd)
    ogc = M.RetrievalCacheO(cfg, budget, prefill, 8, gamma)
    gen = torch.Generator().manual_seed(5)
    ogc.key_cache.copy_(torch.randn(ogc.key_cache.shape, generator=gen).half())
    ogc.value_cache.copy_(torch.randn(ogc.value_cache.shape, generator=gen).half())
    okv = M.FullCache(cfg, 64)
    model = LlamaForCausalLM.from_state_dict(LlamaConfig.from_dict(cfg), sd, DEV)
    pg = RetrievalCache(model, max_budget=budget, prefill=prefill, gamma=gamma, chunk_size=8)
    pg.k.copy_(ogc.key_cache.permute(0, 2, 1, 3))
    pg.v.copy_(ogc.value_cache.permute(0, 2, 1, 3))
    pkv = FlashSimpleCache(model, 64)
    ids = torch.randint(3, 32000, (1, gamma + 1), generator=gen)
    pos = torch.arange(100000, 100000 + gamma + 1).unsqueeze(0)
    want = ot.forward(ids, okv, ogc, position_ids=pos, spec=True)
    got = model(input_ids=ids.to(DEV), kv_cache=pkv, graph_cache=pg, position_ids=pos.to(DEV), spec=True).logits.cpu()
    _logit_check("7B-width layer, retrieval-cache forward", got, want)
    s = pg.spec_slot                                                     # the gamma+1 rows written by the fused epilogue
    dk = (pg.k[0, :, s:].permute(1, 0, 2).cpu().float() - ogc.key_cache[0, s:].float()).abs()
    assert Hh.bound("7B-width layer: appended K rows, max", dk.max(), 8e-3) and Hh.bound("7B-width layer: appended K rows, mean", dk.mean(), 2e-6)
    trail = want.max(-1).values - want.gather(-1, got.argmax(-1, keepdim=True))[..., 0]   # device argmax vs oracle's best
    assert float(trail.max()) < GAP_TOL


def test_full_scale_7b_greedy_triforce_is_lossless_on_device():
    """BASELINE configs[1] at FULL size (Llama-2-7B-128K shape, 124 928-token KV prefix, budget 4096, gamma 6,
    hipGraphs): greedy TriForce must reproduce the target's own greedy continuation.  The prefix KV is the reference's
    synthetic filler (N(0,1), cache.py:303-308) — losslessness does not depend on how the prefix was produced — and
    the check is teacher-forced on the device: every emitted token must be the argmax of a plain autoregressive
    forward over the same prefix (up to GAP_TOL where two logits are within fp16 noise).  Guards the 64-bit offsets,
    the 131K-position YaRN table and the 32-layer caches that the tiny configs cannot reach."""
    import argparse
    import bench
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.sampling import UniformSource
    args = argparse.Namespace(target="llama-7B-128K", prefill=124928, budget=4096, chunk_size=8, gamma=6, temp=1.0,
                              top_p=1e-9, gen_cap=256, seed=0, no_graphs=False)
    dev = torch.device(DEV)
    target, draft = bench.load_models(args, dev, "random", "random:1", "random:2")
    ge = bench.build_engine(args, dev, target, draft)
    assert sorted(ge.target_graphs) == [1, 7, 8]               # the target verify is replayed from its hipGraph here
    tcfg, _ = bench.target_config(args.target)
    ids = torch.randint(3, tcfg.vocab_size, (1, args.prefill), generator=torch.Generator().manual_seed(0)).to(dev)
    run = TriForceRunner(bench._Tok(), ge, args.gamma, top_k=-1, top_p=args.top_p, temperature=args.temp,
                         rng=UniformSource(dev, seed=0))
    bench.do_prefill(run, ge, ids, "synthetic")
    P = ge.engine.kv_cache.seq_len
    assert P == args.prefill
    while run.n < 20:
        run.step()
    stream = list(run.emitted)
    assert len(stream) >= 21 and ge.engine.kv_cache.seq_len == P + run.n
    # teacher-forced plain decode over the same prefix
    eng = ge.engine
    eng.kv_cache.seq_len = P
    gaps = []
    for i in range(len(stream) - 1):
        tok = torch.tensor([[stream[i]]], device=dev)
        logits = eng.model(input_ids=tok, kv_cache=eng.kv_cache, graph_cache=None).logits[0, -1]
        gaps.append(float(logits.max() - logits[stream[i + 1]]))
    assert max(gaps) < GAP_TOL, f"token {gaps.index(max(gaps)) + 1} trails the autoregressive argmax by {max(gaps):.4f}"
    assert sum(1 for x in gaps if x == 0.0) >= len(gaps) - 2
    del ge, run, eng, target, draft
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ["small_gamma6", "cfg1_greedy"])
def test_captured_target_verify_equals_eager(name):
    """The full-cache forward replayed from its hipGraph (append slot and key count read from device memory, launch
    sized by the cache capacity) against the eager forward of the same block: same logits up to the fp32 summation
    order of a different split-KV partition, same rows appended, same probabilities; and the q_len == 1 graph used by
    the autoregressive baseline against the eager step."""
    from triforce_amd.utils.sampling import norm_logits
    g = Hh.load_golden(name)
    ge = Hh.build_product(g, DEV, graphs=True)
    gamma = g["gamma"]
    assert sorted(ge.target_graphs) == sorted({1, gamma + 1, gamma + 2})
    prompt = Hh.prompt_of(g).to(DEV)
    ge.inference(prompt[:, :-1])
    ge.inference(prompt[:, -1:])
    kvc = ge.engine.kv_cache
    S = kvc.seq_len
    for q_len in (gamma + 1, gamma + 2):
        ids = torch.randint(3, g["tcfg"]["vocab_size"], (1, q_len), generator=torch.Generator().manual_seed(q_len)).to(DEV)
        want = ge.inference(ids, eager=True)
        rows_k = kvc.k[:, :, S:S + q_len].clone()
        assert kvc.seq_len == S + q_len
        kvc.seq_len = S
        kvc.k[:, :, S:S + q_len].zero_()
        got = ge.inference(ids)
        assert kvc.seq_len == S + q_len
        _logit_check(f"captured verify q={q_len}", got.cpu(), want.cpu())
        dk = (kvc.k[:, :, S:S + q_len].float() - rows_k.float()).abs()
        assert float(dk[0].max()) == 0.0 and float(dk.max()) < 2e-2           # layer 0 rows do not depend on attention
        kvc.seq_len = S
        p_graph = ge.verify_probs(ids, g["temperature"], g["top_p"]).clone()
        kvc.seq_len = S
        p_eager = norm_logits(want[0], temperature=g["temperature"], top_k=-1, top_p=g["top_p"])
        assert Hh.bound("captured vs eager target verify: probability rows", (p_graph - p_eager).abs().max(), 1e-3)
        kvc.seq_len = S
    tok = prompt[:, -1:]
    a = ge.decode_step(tok).clone()
    kvc.seq_len = S
    b = ge.engine.model(input_ids=tok, kv_cache=kvc, graph_cache=None).logits
    _logit_check("captured AR step", a.cpu(), b.cpu())
    # a cache one row short of the block must refuse the replay, not write past the end
    kvc.seq_len = kvc.max_budget - gamma
    with pytest.raises(IndexError):
        ge.inference(torch.zeros((1, gamma + 1), dtype=torch.long, device=DEV))
    kvc.seq_len = S


@pytest.mark.parametrize("spec_str,lo_mid,hi_mid,lo_tgt,hi_tgt", [
    ("aligned:0.7:0.9:0", 0.50, 0.85, 0.78, 0.97),
    ("aligned:0.3:0.97:0", 0.15, 0.45, 0.90, 1.00),
])
def test_aligned_weights_set_the_acceptance_on_device(spec_str, lo_mid, hi_mid, lo_tgt, hi_tgt):
    """Aligned synthetic weights (models/aligned.py) through the HIP kernels and hipGraphs: the calibration lands on the
    requested retrieval -> target acceptance and the decode loop then sees both requested rates (same bands as the CPU
    test of the host logic, tests/test_aligned_cpu.py)."""
    from oracle import specs
    from triforce_amd.models import aligned
    from triforce_amd.models.cache import FlashSimpleCache, RetrievalCache, StreamingLLMEvictionCache
    from triforce_amd.models.config_yarn import LlamaConfig
    from triforce_amd.models.modeling_llama import LlamaForCausalLM
    from triforce_amd.models.modeling_llama_68m import LlamaForCausalLM as Draft
    from triforce_amd.utils.decoding import TriForceRunner
    from triforce_amd.utils.graph_infer import GraphInferenceEngine
    from triforce_amd.utils.sampling import UniformSource
    V, P, B, gamma = 4096, 2048, 256, 4
    tcfg = LlamaConfig.from_dict(specs.tiny_target_config(vocab_size=V, layers=2, hidden=256, heads=2, max_pos=8192))
    dcfg = LlamaConfig.from_dict(specs.draft_68m_config(vocab_size=V))
    spec = aligned.parse_spec(spec_str)
    target = LlamaForCausalLM(tcfg, DEV).init_aligned(spec, attn_keys=B)
    draft = Draft(dcfg, DEV).init_aligned(spec, attn_keys=256)
    ge = GraphInferenceEngine(target, FlashSimpleCache(target, P + 400),
                              RetrievalCache(target, max_budget=B, prefill=P, gamma=gamma, chunk_size=8), draft,
                              StreamingLLMEvictionCache(draft, start_size=16, recent_size=256 - 16 - gamma, gamma=gamma))
    ge.initialize_cuda_graph(gamma, probs=True, temperature=0.6, top_p=0.9, verbose=False)
    run = TriForceRunner(Hh.FakeTokenizer(), ge, gamma, top_k=-1, top_p=0.9, temperature=0.6,
                         rng=UniformSource(DEV, seed=3))
    run.prefill(specs.random_prompt(V, P, 11).to(DEV))
    cal = target.weights.aligned["calibration"]
    assert abs(cal["probe_acceptance"] - spec.retrieval_acc) < 0.02 and cal["probe_acceptance_gain0"] > 0.98
    steps = 48
    for i in range(steps):
        run.eager_every = 4                                            # mix graph replays and eager verifies
        run.step()
    per_token = run.accepted_count / (run.accepted_count + run.resample_count)
    middle = sum(run.acc_rate_middle_list) / len(run.acc_rate_middle_list)
    assert lo_tgt <= per_token <= hi_tgt, per_token
    assert lo_mid <= middle <= hi_mid, middle
    assert run.n / steps > (2.0 if spec.retrieval_acc < 0.95 else 2.5)
    assert 2 not in run.emitted and all(3 <= t < V for t in run.emitted)
    # the in-place re-draw used by bench.py's secondary measurement: graphs keep working, acceptance collapses
    target.weights.overwrite_random_(1)
    draft.weights.overwrite_random_(2)
    run2 = TriForceRunner(Hh.FakeTokenizer(), ge, gamma, top_k=-1, top_p=0.9, temperature=0.6,
                          rng=UniformSource(DEV, seed=4))
    run2.prefill(specs.random_prompt(V, P, 11).to(DEV))
    for _ in range(12):
        run2.step()
    # (no acceptance claim here: at this toy size N(0, 0.02) weights give both models near-uniform distributions over
    # the 4096 tokens, which overlap; the 7B / 32000-token collapse to ~0.01 is bench.py's ``random_weights`` line)
    assert target.weights.aligned is None and run2.n >= 12 and all(0 <= t < V for t in run2.emitted)


def test_static_verify_rows_equal_per_step_copies_and_lifetime_is_guarded():
    """The decode loop hands the retrieval-verify graph's STATIC output to the outer accept test instead of copying a
    probability row out per inner step (row i of the last replay is bit-identical to the row an earlier replay produced
    when position i was decided).  Checked here: Middle_Spec with static rows == Middle_Spec with per-step copies, bit for
    bit, on the same uniforms (stochastic settings, several drafted positions); and the lifetime guard trips when the
    verify graph replays before the rows are consumed."""
    from triforce_amd.utils.decoding import Middle_Spec, TriForceRunner
    from triforce_amd.utils.sampling import UniformSource
    g = Hh.load_golden("small_gamma6")
    ge = Hh.build_product(g, DEV, temperature=0.8, top_p=0.95, graphs=True)
    assert ge.static_outputs and ge.verify_generation() is not None
    vals = Hh.fixed_uniforms(seed=123)
    run = TriForceRunner(Hh.FakeTokenizer(), ge, g["gamma"], top_k=-1, top_p=0.95, temperature=0.8,
                         rng=UniformSource(DEV, values=vals))
    run.prefill(Hh.prompt_of(g).to(DEV))
    tok = run.next_token
    out = {}
    for static in (True, False, True):
        ge.static_outputs = static
        rng = UniformSource(DEV, values=vals)
        rng.advance(7)
        ids, rows, acc = Middle_Spec(tok, ge, g["gamma"], False, Hh.FakeTokenizer(), rng=rng)
        out.setdefault(static, []).append((list(ids), rows.clone(), acc))
    ge.static_outputs = True
    (ids_s, rows_s, acc_s), (ids_s2, rows_s2, _) = out[True]
    ids_c, rows_c, acc_c = out[False][0]
    assert ids_s == ids_c == ids_s2 and acc_s == acc_c
    assert torch.equal(rows_s, rows_c), "static retrieval-verify rows differ from the per-step copies"
    assert torch.equal(rows_s, rows_s2), "re-running the same inner loop is not bitwise deterministic"
    Hh.note(f"static verify rows == per-step copies over {len(ids_s) - 1} drafted positions (acceptance {acc_s:.2f})")
    # lifetime guard: a stray replay of the verify graph between Middle_Spec and the accept test must be caught
    run.step()                                             # a normal step passes the guard
    bufs = run.bufs
    gen0 = ge.verify_generation()
    Middle_Spec(run.next_token, ge, g["gamma"], False, Hh.FakeTokenizer(), rng=run.rng, buffers=bufs)
    assert bufs.rows_generation == ge.verify_generation() > gen0
    ge.graph_verify(bufs.verify_tokens, bufs.positions, clone=False)           # the stray replay
    assert ge.verify_generation() != bufs.rows_generation   # ... is what TriForceRunner.step's assert compares


@pytest.mark.parametrize("temperature,top_p", [(0.8, 0.95), (1.0, 1e-9)])
def test_one_launch_inner_iterations_emit_the_identical_stream(temperature, top_p, monkeypatch):
    """Round 5: an inner iteration of Middle_Spec (reference decoding.py:182-220) is ONE hipGraph — draft step,
    draw, retrieval verify, accept test, with the uniforms behind a device cursor the kernels advance themselves.  Nothing
    about the arithmetic changes, so against rounds 2-4's form (two replays + two eager kernels per iteration) the emitted
    tokens, the per-step accept counts and the consumed uniforms must be IDENTICAL — over a run long enough (>= 150 outer
    steps at T = 0.8, ~600 inner iterations) that a token id, a probability row or a cursor value consumed before it was
    visible, or a cursor out of step with the host's mirror, would show as a diverged stream.  Also: a second runner with a
    fresh uniform stream on the same engine (re-capture against the new buffers), and the cursor check itself (a host mirror
    pushed out of step must raise)."""
    from triforce_amd.utils import decoding as Dm
    from triforce_amd.utils.decoding import TriForce, TriForceRunner
    from triforce_amd.utils.sampling import UniformSource
    g = dict(Hh.load_golden("small_gamma6"), gen_len=260, budget=320)     # room for a long run (tail <= retrieval budget)
    prompt, tok = Hh.prompt_of(g).to(DEV), Hh.FakeTokenizer()
    vals = Hh.fixed_uniforms(n=4096, seed=901)
    max_len = 230
    out = {}
    for mode, inner in {"four launches": False, "one graph": True}.items():
        # a FRESH engine per form: a second prompt on one engine legitimately differs from the first (the reference's draft
        # seq_len quirk, SURVEY section 7, which the product keeps) — so first runs are compared with first runs, second with second
        monkeypatch.setattr(Dm, "INNER_GRAPH", inner)
        ge = Hh.build_product(g, DEV, temperature=temperature, top_p=top_p, graphs=True)
        for run_no in (1, 2):                                   # the second run: a new runner and uniform stream -> re-capture
            rng = UniformSource(DEV, values=vals)
            res = TriForce(tok, ge, prompt, gamma=g["gamma"], max_len=max_len, top_k=-1, top_p=top_p, temperature=temperature,
                           rng=rng, return_details=True)
            out[(mode, run_no)] = (res["tokens"], res["counts"], rng.pos)
        assert bool(ge._inner) == inner
    for run_no in (1, 2):
        ref, got = out[("four launches", run_no)], out[("one graph", run_no)]
        assert len(ref[1]) >= 30
        assert got[0] == ref[0], f"run {run_no}: tokens diverge at {Hh.common_prefix(got[0], ref[0])} of {len(ref[0])}"
        assert got[1] == ref[1] and got[2] == ref[2], f"run {run_no}: accept counts / uniform position differ"
    ref = out[("four launches", 1)]
    Hh.note(f"inner-iteration graphs: {len(ref[0])} tokens / {len(ref[1])} steps identical to the four-launch form, first and "
            f"second prompt (T={temperature}, top_p={top_p})")
    # the device cursor and the host's mirror are compared at every record: a mirror pushed out of step raises
    run = TriForceRunner(tok, ge, g["gamma"], top_k=-1, top_p=top_p, temperature=temperature, rng=UniformSource(DEV, values=vals))
    assert run.inner is not None
    run.prefill(prompt)
    run.step()
    run.rng.pos += 1                                   # (the device copy is current: nothing refreshes it)
    with pytest.raises(RuntimeError, match="out of step"):
        run.step()


def test_uniform_stream_refill_in_place_under_the_inner_graphs(monkeypatch):
    """The captured inner iterations and the on-device step read their uniforms as buf[cursor + k] behind FIXED addresses, so
    `UniformSource` refills its one buffer in place and resets the device cursor when a block is used up (every 65 536 numbers
    in production — ~3 600 outer steps — which no other device test reaches).  A seeded stream with a 48-number block refills every
    few outer steps: tokens, accept counts and the final stream position must equal the four-launch form's, which draws the
    same blocks through plain pointers."""
    from triforce_amd.utils import decoding as Dm
    from triforce_amd.utils.decoding import TriForce
    from triforce_amd.utils.sampling import UniformSource
    g = dict(Hh.load_golden("small_gamma6"), gen_len=120, budget=320)
    prompt, tok = Hh.prompt_of(g).to(DEV), Hh.FakeTokenizer()
    out, refills = {}, {}
    for mode, inner in {"four launches": False, "one graph": True}.items():
        monkeypatch.setattr(Dm, "INNER_GRAPH", inner)
        ge = Hh.build_product(g, DEV, temperature=0.8, top_p=0.9, graphs=True)
        rng = UniformSource(DEV, seed=5, block=48)
        count = [0]
        room = rng._room

        def counting(n, room=room, rng=rng, count=count):
            before = rng.pos
            room(n)
            count[0] += int(rng.pos < before)
        rng._room = counting
        res = TriForce(tok, ge, prompt, gamma=g["gamma"], max_len=96, top_k=-1, top_p=0.9, temperature=0.8, rng=rng,
                       return_details=True)
        out[mode], refills[mode] = (res["tokens"], res["counts"], rng.pos), count[0]
        assert bool(ge._inner) == inner
    assert refills["one graph"] >= 3 and refills["one graph"] == refills["four launches"], refills
    ref, got = out["four launches"], out["one graph"]
    assert got[0] == ref[0], f"tokens diverge at {Hh.common_prefix(got[0], ref[0])} of {len(ref[0])} ({refills} refills)"
    assert got[1] == ref[1] and got[2] == ref[2]
    Hh.note(f"uniform stream refilled in place {refills['one graph']} times under the inner graphs: {len(ref[0])} tokens identical "
            "to the four-launch form")


def test_draft_prefill_graph_equals_eager(monkeypatch):
    """The 68M draft's prompt pass replays ONE captured steady-state step (shift the StreamingLLM window by 64 rows, run 64
    rows) per full chunk once the window is full; the result must equal the all-eager pass bit for bit: returned logits,
    draft cache contents, cache length — including a ragged last chunk and a second prompt through the cached graph."""
    g = Hh.load_golden("cfg1_greedy")
    ge = Hh.build_product(g, DEV, graphs=False)
    eng = ge.engine
    prompt = Hh.prompt_of(g).to(DEV)
    vocab = g["dcfg"]["vocab_size"]
    other = torch.randint(3, vocab, (1, 1500 + 37), generator=torch.Generator().manual_seed(4)).to(DEV)
    results = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("TRIFORCE_DRAFT_PREFILL_GRAPH", mode)
        outs = []
        for ids in (prompt, other, prompt[:, :1000]):                 # 1000 = 15 full chunks + 40: below the graph threshold
            eng.draft_cache.reset()
            eng.draft_cache.seq_len = 0
            lg = ge.graph_draft_prefill(input_ids=ids)
            torch.cuda.synchronize()
            outs.append((lg.clone(), eng.draft_cache.k.clone(), eng.draft_cache.v.clone(), eng.draft_cache.seq_len))
        results[mode] = outs
    assert getattr(eng, "_dpf_graph", None) is not None and eng._dpf_graph[1] is not None, "the steady step was not captured"
    for (la, ka, va, sa), (lb, kb, vb, sb) in zip(results["0"], results["1"]):
        assert sa == sb and torch.equal(la, lb) and torch.equal(ka, kb) and torch.equal(va, vb)


def _bench_line(*extra, timeout=600):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--target", "tiny", "--prefill", "2048", "--budget",
           "256", "--gamma", "4", "--steps", "4", "--warmup", "1", "--weights", "random:3", *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=root)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return lines[0]


def test_bench_plain_line_dumps_the_last_step_and_full_line_adds_the_extras(tmp_path):
    """bench.py on the tiny target: a plain run times exactly --steps steps and carries the headline fields only; with
    --dump-outputs it writes the last timed step's tokens (float64) and its target verify's probabilities (float32, one
    row per verified token), the same in two runs with the same arguments; --full adds the measurements of their own."""
    import numpy as np
    from triforce_amd.models import zoo
    gamma, vocab = 4, zoo.config("tiny").vocab_size
    runs = []
    for k in range(2):
        out = tmp_path / f"dump{k}"
        j = _bench_line("--dump-outputs", str(out))
        assert j["steps"] == 4 and j["warmup"] == 1 and j["n_gpus"] == 1 and not j["full"]
        assert j["unit"] == "tokens/s" and j["higher_is_better"] is True and j["dtype"] == "f16"
        assert j["value"] > 0 and j["ms_per_step"] > 0 and j["tokens"] >= 4
        assert abs(j["value"] - j["tokens"] / (4 * j["ms_per_step"] * 1e-3)) < 0.01 * j["value"]
        for key in ("stage_latency_us", "roofline_stages", "ar_baseline_tokens_per_s", "random_weights", "cpu_baseline"):
            assert key not in j, key
        tok, probs = np.load(out / "tokens.npy"), np.load(out / "verify_probs.npy")
        assert tok.dtype == np.float64 and tok.ndim == 1 and 1 <= tok.size <= gamma + 2
        assert np.all(tok == np.round(tok)) and np.all((tok >= 0) & (tok < vocab))
        assert probs.dtype == np.float32 and probs.shape[0] in (gamma + 1, gamma + 2) and probs.shape[1] == vocab
        assert np.all(probs >= 0) and np.allclose(probs.sum(axis=1), 1.0, atol=1e-3)
        runs.append((tok, probs))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    j = _bench_line("--full", "--no-cpu-baseline", timeout=900)
    assert j["full"] and j["steps"] == 4
    assert j["stage_latency_us"]["target_verify_us"] > 0 and j["ar_baseline_tokens_per_s"] > 0 and j["roofline_stages"]
