"""GPU: residual-stream task vectors (Hendel et al.) — the grouped capture
``tvr_trace_capture_resid`` (``Model.capture_resid``), the site kind
``TVR_SITE_SET_RESID_PRE_VEC`` and the experiment functions built on them.

Bars (tests/test_gpu_engine.py's fp32 bars): logits 1e-4 of max|ref|,
probabilities 1e-5 of the largest softmax value, extracted vectors 1e-4
relative.  The capture's bound is derived: a sum of n fp32 terms in any order
is within (n - 1) ulp-halves of the running magnitude, so per element
|err| <= n_g * 2^-23 * sum|x| over the group's rows, plus 2^-23 * max|x| for
the centring on a trace filled on the exact-fp16 path.

Experiment parity (tests 4 and 5) runs on the tiny model with 4 layers: on 52
contexts x 4 layers the fp64 oracle's smallest top-2 gap is 3.1e-4 of
max|logit| (above the logit bar; 8.4e-5 on the 2-layer model), and the patch
changes the argmax in 106 of the 208 pairs.
"""
import functools
import random

import numpy as np
import pytest
import torch

import tvr_amd
from conftest import GEMM_MODES, TINY_STD, make_oracle
from oracle import reference_experiments as R
from tvr_amd import _lib, experiments

pytestmark = pytest.mark.gpu

ARROW = tvr_amd.tasks.ARROW
KIND6, KIND3 = _lib.SITE_SET_RESID_PRE_VEC, _lib.SITE_SET_RESID_PRE_POS
FP32_TOL, FP32_PROB_TOL, VEC_TOL = 1e-4, 1e-5, 1e-4
EPS = 2.0 ** -23


def rel_err(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def ragged_prompts(cfg, lens, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [[0] + torch.randint(1, cfg.d_vocab, (n - 1,), generator=g).tolist() for n in lens]


@pytest.fixture(scope="module")
def exact16_model(tiny_cfg, tokenizer):
    """fp16-valued weights: the exact-fp16 GEMMs are bound and the trace is
    uncentred (as tests/test_gpu_exact16.py builds its tiny model)."""
    sd = tvr_amd.weights.synth_hf_state_dict(tiny_cfg, seed=0, std=0.3, fp16=True)
    m = tvr_amd.Model.from_hf_state_dict(tiny_cfg, sd, device="cuda", tokenizer=tokenizer, gemm="x2f16")
    assert m.exact16
    return m


def filled_trace(model, prompts, defer=False):
    trace = model.trace(len(prompts), sum(map(len, prompts)))
    model.forward_clean(prompts, trace=trace, defer=defer)
    return trace


# ------------------------------------------------------------ 1. capture = export
def check_capture(model, prompts, pos, groups, n_groups, uncentred):
    trace = filled_trace(model, prompts)
    L = model.cfg.n_layers
    out = model.capture_resid(trace, pos, groups, n_groups)
    assert tuple(out.shape) == (n_groups, L + 1, model.cfg.d_model)
    off = np.concatenate([[0], np.cumsum([len(p) for p in prompts])[:-1]])
    p = np.asarray([len(q) - 1 for q in prompts]) if pos is None else np.asarray(pos)
    grp = np.zeros(len(prompts), dtype=np.int64) if groups is None else np.asarray(groups)
    worst = 0.0
    for l in range(L + 1):
        x = trace.resid_pre(l).double().cpu()
        for g in range(n_groups):
            rows = x[(off + p)[grp == g]]
            if rows.shape[0] == 0:
                assert out[g, l].abs().max().item() == 0.0
                continue
            bound = rows.shape[0] * EPS * rows.abs().sum(0) + (EPS * rows.abs().max() if uncentred else 0.0)
            err = (out[g, l].double().cpu() - rows.sum(0)).abs()
            worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
            assert bool((err <= bound).all()), (l, g, (err / bound).max().item())
    print(f"capture: worst error / bound {worst:.3f} ({len(prompts)} prompts, {n_groups} groups)")
    again = model.capture_resid(trace, pos, groups, n_groups)
    assert torch.equal(out, again)  # bitwise reproducible
    acc = model.capture_resid(trace, pos, groups, n_groups, out=out.clone())
    assert acc.data_ptr() != out.data_ptr() and torch.equal(acc, out + out)  # += on a caller's buffer
    return out


CAPTURE_CASES = {
    # 5 ragged prompts, first / middle / last positions, three groups (every group one chunk)
    "ragged": ([3, 7, 15, 7, 3], [0, 3, 14, 0, 2], [0, 1, 0, 2, 1], 3),
    # the defaults: last positions, one group
    "defaults": ([3, 7, 15, 7, 3], None, None, 1),
    # 40 prompts: group 0 holds 35 rows (chunks of 16 + 16 + 3 and the second pass), group 2 five rows
    # (one chunk, summed straight into out), group 1 none (its rows of out stay zero)
    "chunked": ([3] * 20 + [5] * 20, None, [0] * 7 + [2] + ([0] * 7 + [2]) * 4, 3),
    # identity groups: per-prompt vectors
    "identity": ([3, 7, 15, 7, 3], None, [0, 1, 2, 3, 4], 5),
}


@pytest.mark.parametrize("case", list(CAPTURE_CASES))
def test_capture_equals_export(tiny_model, case):
    lens, pos, groups, n_groups = CAPTURE_CASES[case]
    check_capture(tiny_model, ragged_prompts(tiny_model.cfg, lens), pos, groups, n_groups, uncentred=False)


@pytest.mark.parametrize("case", list(CAPTURE_CASES))
def test_capture_equals_export_exact16(exact16_model, case):
    lens, pos, groups, n_groups = CAPTURE_CASES[case]
    out = check_capture(exact16_model, ragged_prompts(exact16_model.cfg, lens), pos, groups, n_groups, uncentred=True)
    # TransformerLens' residual stream is centred: so are the captured sums
    assert out.double().mean(-1).abs().max().item() <= 1e-5 * out.abs().max().item()


def test_capture_runs_a_deferred_forward_first(tiny_model):
    prompts = ragged_prompts(tiny_model.cfg, [3, 7, 15])
    want = tiny_model.capture_resid(filled_trace(tiny_model, prompts))
    got = tiny_model.capture_resid(filled_trace(tiny_model, prompts, defer=True))
    assert torch.equal(want, got)


# ------------------------------------------------------- 2. kind 6 reproduces kind 3
def kind3_and_kind6(model, defer):
    """The same row swaps as kind 3 (source row of the trace) and as kind 6
    (the exported row as a caller's vector): a mid position of the T = 15
    prompt (rows 6..14 recomputed) and last positions, at every layer."""
    L = model.cfg.n_layers
    prompts = ragged_prompts(model.cfg, [15, 7, 3, 15])
    swaps = [(0, 6, 3, 9), (0, 14, 1, 6), (1, 6, 2, 2), (2, 2, 0, 14)]  # (seq, pos, src_seq, src_pos)
    n = len(swaps) * L
    s3 = tvr_amd.make_sites(n)
    for k, (seq, pos, sseq, spos) in enumerate(swaps):
        for l in range(L):
            r = s3[k * L + l]
            r["seq"], r["pos"], r["src_seq"], r["src_pos"], r["layer"] = seq, pos, sseq, spos, l
            r["target"] = prompts[seq][1]
    s3["kind"] = KIND3
    s6 = s3.copy()
    s6["kind"], s6["vec"] = KIND6, np.arange(n)
    s6["src_seq"] = s6["src_pos"] = 0
    trace = filled_trace(model, prompts, defer)
    out3 = model.patch_sweep(trace, s3, None, topk=3, return_logits=True)
    # the rows kind 3 read, exported from the trace that sweep used (a fused sweep has just filled it)
    off = trace.seq_offsets
    vectors = torch.stack([trace.resid_pre(int(r["layer"]))[off[int(r["src_seq"])] + int(r["src_pos"])] for r in s3])
    trace = filled_trace(model, prompts, defer)
    out6 = model.patch_sweep(trace, s6, vectors, topk=3, return_logits=True)
    return out3, out6


@pytest.mark.parametrize("defer", [False, True], ids=["filled", "deferred"])
def test_kind6_reproduces_kind3_bitwise(tiny_model, defer):
    out3, out6 = kind3_and_kind6(tiny_model, defer)
    for k in ("logits", "prob", "topk"):
        assert torch.equal(out3[k], out6[k]), k


@pytest.mark.parametrize("defer", [False, True], ids=["filled", "deferred"])
def test_kind6_reproduces_kind3_exact16(exact16_model, defer):
    """The exact-fp16 path's rows carry one constant per row; the exported
    (centred) vector does not: equal to fp32 rounding, not bitwise."""
    out3, out6 = kind3_and_kind6(exact16_model, defer)
    e = rel_err(out6["logits"], out3["logits"])
    ep = (out6["prob"] - out3["prob"]).abs().max().item() / torch.softmax(out3["logits"], -1).max().item()
    print(f"kind 6 vs kind 3, exact-fp16: logits {e:.2e} prob {ep:.2e}")
    assert e <= FP32_TOL and ep <= FP32_PROB_TOL


# ------------------------------------------------------- 3. kind 6 against the oracle
@pytest.fixture(scope="module")
def oracle_cases(tiny_cfg, tiny_oracle):
    """12 sites: 3 prompts x (layer 0, layer L-1) x (a mid position, the last
    one), each with its own random vector of the norm of a real residual row,
    and the oracle's last-position logits under the hook."""
    L, d = tiny_cfg.n_layers, tiny_cfg.d_model
    prompts = ragged_prompts(tiny_cfg, [15, 7, 3], seed=11)
    g = torch.Generator().manual_seed(5)
    _, cache = tiny_oracle.run_with_cache(torch.tensor([prompts[0]]))
    norm = cache[f"blocks.{L - 1}.hook_resid_pre"][0, -1].norm().item()
    cases = [(i, l, pos) for i, p in enumerate(prompts) for l in (0, L - 1) for pos in (len(p) // 2, len(p) - 1)]
    vecs = torch.randn(len(cases), d, generator=g)
    vecs = vecs / vecs.norm(dim=1, keepdim=True) * norm
    ref = []
    for k, (i, l, pos) in enumerate(cases):
        def fn(x, hook, pos=pos, v=vecs[k]):
            x[0, pos] = v
            return x
        ref.append(tiny_oracle.run_with_hooks(torch.tensor([prompts[i]]), [(f"blocks.{l}.hook_resid_pre", fn)])[0, -1])
    clean = [tiny_oracle.forward(torch.tensor([p]))[0, -1] for p in prompts]
    return dict(prompts=prompts, cases=cases, vecs=vecs, ref=ref, clean=clean)


def kind6_sites(r):
    s = tvr_amd.make_sites(len(r["cases"]))
    for k, (i, l, pos) in enumerate(r["cases"]):
        s[k]["seq"], s[k]["layer"], s[k]["pos"], s[k]["vec"] = i, l, pos, k
        s[k]["target"] = r["prompts"][i][1]
    s["kind"] = KIND6
    return s


def assert_matches_oracle(out, rows, sites, refs, what):
    worst = worst_p = 0.0
    for j, ref in zip(rows, refs):
        e = rel_err(out["logits"][j], ref)
        sm = torch.softmax(ref, 0)
        ep = abs(out["prob"][j].item() - sm[int(sites[j]["target"])].item()) / sm.max().item()
        worst, worst_p = max(worst, e), max(worst_p, ep)
        assert e <= FP32_TOL, (what, j, e)
        assert ep <= FP32_PROB_TOL, (what, j, ep)
    print(f"{what}: logits {worst:.2e} prob {worst_p:.2e}")


def unaligned(vectors):
    """The same values at a base that is float- but not 16-byte aligned."""
    buf = torch.empty(vectors.numel() + 1, device=vectors.device)
    view = buf[1:].view(vectors.shape)
    view.copy_(vectors)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("defer", [False, True], ids=["filled", "deferred"])
def test_kind6_against_oracle(tiny_model, oracle_cases, defer):
    r = oracle_cases
    sites, vecs = kind6_sites(r), r["vecs"].cuda()
    n = len(sites)
    out = tiny_model.patch_sweep(filled_trace(tiny_model, r["prompts"], defer), sites, vecs, topk=3, return_logits=True)
    assert_matches_oracle(out, range(n), sites, r["ref"], f"kind 6 ({'deferred' if defer else 'filled'})")
    for j in range(n):
        assert out["topk"][j].tolist() == torch.topk(out["logits"][j], 3).indices.tolist()
    # an unaligned view of the same vectors: accepted, same results
    out_u = tiny_model.patch_sweep(filled_trace(tiny_model, r["prompts"], defer), sites, unaligned(vecs), topk=3,
                                   return_logits=True)
    for k in ("logits", "prob", "topk"):
        assert torch.equal(out[k], out_u[k]), k


@pytest.mark.parametrize("defer", [False, True], ids=["filled", "deferred"])
def test_kind6_mixed_with_other_kinds(tiny_model, oracle_cases, defer):
    """One launch holding kinds 0, 1, 2 and 6: the kind-6 rows still match the
    oracle, the kind-0 rows the clean forward, and kinds 1 / 2 what they give
    in a launch of their own."""
    r = oracle_cases
    s6, vecs = kind6_sites(r), r["vecs"].cuda()
    n6, npr = len(s6), len(r["prompts"])
    other = tvr_amd.make_sites(3 * npr)
    other["seq"] = np.tile(np.arange(npr), 3)
    other["kind"] = np.repeat([_lib.SITE_NONE, _lib.SITE_REPLACE_HEAD_ALLPOS, _lib.SITE_ADD_ATTN_OUT_LASTPOS], npr)
    other["layer"], other["head"], other["vec"] = 0, 1, np.tile(np.arange(npr), 3)
    other["target"] = [p[1] for p in r["prompts"]] * 3
    mixed = np.concatenate([other[:npr], s6[: n6 // 2], other[npr:], s6[n6 // 2:]])
    rows6 = list(range(npr, npr + n6 // 2)) + list(range(3 * npr + n6 // 2, 3 * npr + n6))
    rows_other = list(range(npr)) + list(range(npr + n6 // 2, 3 * npr + n6 // 2))
    out = tiny_model.patch_sweep(filled_trace(tiny_model, r["prompts"], defer), mixed, vecs, topk=3, return_logits=True)
    assert_matches_oracle(out, rows6, mixed, r["ref"], "kind 6 in a mixed launch")
    assert_matches_oracle(out, range(npr), mixed, r["clean"], "kind 0 in the same launch")
    alone = tiny_model.patch_sweep(filled_trace(tiny_model, r["prompts"], defer), other, vecs, topk=3,
                                   return_logits=True)
    assert rel_err(out["logits"][rows_other], alone["logits"]) <= FP32_TOL


@pytest.mark.parametrize("defer", [False, True], ids=["filled", "deferred"])
def test_kind6_in_the_set_sweep(tiny_model, oracle_cases, defer):
    """tvr_patch_sweep_sets: kind 6 owns an empty patch range next to a head-set
    site; unaligned vectors are fine for both kinds."""
    r = oracle_cases
    s6, vecs = kind6_sites(r), r["vecs"].cuda()
    n6 = len(s6)
    hs = tvr_amd.make_sites(1)
    hs["kind"], hs["seq"], hs["target"] = _lib.SITE_REPLACE_HEADSET_LASTPOS, 1, r["prompts"][1][1]
    sites = np.concatenate([s6[:5], hs, s6[5:]])
    off = np.asarray([0] * 6 + [2] * (n6 - 4), dtype=np.int32)  # the set site (index 5) owns patches [0, 2)
    pat = np.asarray([(0, 1, 2), (1, 3, 4)], dtype=np.int32)
    rows6 = list(range(5)) + list(range(6, n6 + 1))
    out = tiny_model.patch_sweep_sets(filled_trace(tiny_model, r["prompts"], defer), sites, off, pat, vecs, topk=3,
                                      return_logits=True)
    assert_matches_oracle(out, rows6, sites, r["ref"], "kind 6 in the set sweep")
    out_u = tiny_model.patch_sweep_sets(filled_trace(tiny_model, r["prompts"], defer), sites, off, pat, unaligned(vecs),
                                        topk=3, return_logits=True)
    for k in ("logits", "prob", "topk"):
        assert torch.equal(out[k], out_u[k]), k
    # the head-set row is what the set sweep gives without the kind-6 sites around it
    solo = tiny_model.patch_sweep_sets(filled_trace(tiny_model, r["prompts"], defer), hs, np.asarray([0, 2], np.int32),
                                       pat, vecs, topk=3, return_logits=True)
    assert rel_err(out["logits"][5], solo["logits"][0]) <= FP32_TOL
    with pytest.raises(ValueError, match="own patches"):  # a kind-6 site owning patches is refused
        bad = off.copy()
        bad[1:6] = 1
        tiny_model.patch_sweep_sets(filled_trace(tiny_model, r["prompts"]), sites, bad, pat, vecs)


# ----------------------------------------- 4 / 5. experiment parity, 4-layer tiny model
@functools.lru_cache(maxsize=None)
def reference4():
    """The 4-layer tiny model's oracles and the reference experiment, once:
    θ by the run_with_cache loop (fp32 oracle), the patched top-1 ids and
    accuracies by the fp64 oracle, Δprob by the fp32 oracle."""
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    cfg = tvr_amd.get_config("tiny").with_(n_layers=4)
    sd = tvr_amd.weights.synth_hf_state_dict(cfg, seed=0, std=TINY_STD)
    tok = tvr_amd.tokenizer.SyntheticTokenizer(cfg.d_vocab)
    o32, o64 = make_oracle(cfg, sd, tok), make_oracle(cfg, sd, tok, torch.float64)
    L = cfg.n_layers
    contexts = list(tvr_amd.tasks.letter_to_caps)
    random.seed(1234)
    pool = contexts.copy()
    theta = torch.zeros(L + 1, cfg.d_model)
    for _ in range(96):
        random.shuffle(pool)
        ids = R.mix_multitoken_contexts_and_query(pool[:4], pool[4][0], ARROW, None, o32)
        _, cache = o32.run_with_cache(torch.tensor(ids))
        for l in range(L):
            theta[l] += cache[f"blocks.{l}.hook_resid_pre"][0, -1]
        theta[L] += cache[f"blocks.{L - 1}.hook_resid_post"][0, -1]
    theta /= 96
    f = o32.to_single_token(ARROW)
    top1 = torch.zeros(len(contexts), L, dtype=torch.long)
    gap = torch.zeros(len(contexts), L, dtype=torch.float64)
    hits = [0] * L
    dprob = torch.zeros(L, dtype=torch.float64)
    for i, (x, y) in enumerate(contexts):
        tokens = torch.tensor([[0, o32.to_single_token(x), f]])
        answer = o32.to_tokens(y, prepend_bos=False)[0, 0]
        base = torch.softmax(o32.forward(tokens)[0, -1], 0)[answer]
        for l in range(L):
            def fn(v, hook, l=l):
                v[0, -1] = theta[l].to(v.dtype)
                return v
            lg = o64.run_with_hooks(tokens, [(f"blocks.{l}.hook_resid_pre", fn)])[0, -1]
            t2 = torch.topk(lg, 2)
            top1[i, l] = t2.indices[0]
            gap[i, l] = (t2.values[0] - t2.values[1]) / lg.abs().max()
            hits[l] += o64.to_string(int(t2.indices[0])) == y
            lg32 = o32.run_with_hooks(tokens, [(f"blocks.{l}.hook_resid_pre", fn)])[0, -1]
            dprob[l] += (torch.softmax(lg32, 0)[answer] - base).double()
    clean_top1 = torch.stack([o64.forward(torch.tensor([[0, o32.to_single_token(x), f]]))[0, -1].argmax()
                              for x, _ in contexts])
    return dict(cfg=cfg, sd=sd, tok=tok, contexts=contexts, theta=theta, top1=top1, gap=gap,
                acc=[1.0 * h / len(contexts) for h in hits], dprob=dprob / len(contexts), clean_top1=clean_top1)


@functools.lru_cache(maxsize=None)
def engine4(gemm):
    r = reference4()
    return tvr_amd.Model.from_hf_state_dict(r["cfg"], r["sd"], device="cuda", tokenizer=r["tok"], gemm=gemm)


@pytest.mark.parametrize("gemm", GEMM_MODES)
def test_experiment_parity(gemm):
    r, model = reference4(), engine4(gemm)
    L, contexts = r["cfg"].n_layers, r["contexts"]
    random.seed(1234)
    theta = tvr_amd.extract_task_vectors(contexts, ARROW, model, num_contexts=96, len_contexts=4)
    assert tuple(theta.shape) == (L + 1, r["cfg"].d_model)
    e = max(rel_err(theta[l], r["theta"][l]) for l in range(L + 1))
    print(f"{gemm}: task vectors rel err {e:.2e}")
    assert e <= VEC_TOL, e
    # the patched top-1 ids of every (context, layer) pair, through the helper the experiment functions use
    f = model.to_single_token(ARROW)
    seqs = [[0, model.to_single_token(x), f] for x, _ in contexts]
    _, patched = experiments._injection_sweep(model, seqs, theta[:L].contiguous(), lambda l: l, range(L), None, 1,
                                              clean_outputs=False, kind=KIND6)
    got = patched["topk"][..., 0].cpu().long()
    keep = r["gap"] >= 1e-5
    left_out = int((~keep).sum())
    changed = int((r["top1"] != r["clean_top1"][:, None]).sum())
    print(f"{gemm}: smallest oracle gap {r['gap'].min().item():.2e}, left out {left_out}, "
          f"patch changes the argmax in {changed} of {keep.numel()} pairs, "
          f"mismatches {int((got != r['top1'])[keep].sum())}")
    assert left_out <= 0.05 * keep.numel()
    assert changed >= keep.numel() // 4  # the sweep can tell a patched forward from a clean one
    assert torch.equal(got[keep], r["top1"][keep])
    acc = tvr_amd.apply_task_vectors_to_zero_shot(theta, contexts, ARROW, model=model)
    assert acc == r["acc"]
    assert tvr_amd.apply_task_vectors_to_zero_shot(theta[:L], contexts, ARROW, model=model) == acc  # [L, d] too
    dp = tvr_amd.apply_task_vectors_to_zero_shot_by_probability(theta, contexts, ARROW, model=model)
    err = (dp.double().cpu() - r["dprob"]).abs().max().item()
    print(f"{gemm}: dprob abs err {err:.2e} (max |ref| {r['dprob'].abs().max().item():.3e})")
    assert err <= 1e-4 * r["dprob"].abs().max().item() + 1e-7


@pytest.mark.parametrize("gemm", GEMM_MODES)
def test_extract_then_patch_end_to_end(gemm):
    """Per-prompt vectors (identity groups) patched back with kind 6 equal the
    kind-3 row swap of the same rows — into their own source prompt (the
    identity patch: the clean result) and into the next prompt: the capture and
    the site agree on centred values and on ``layer`` indexing hook_resid_pre."""
    r, model = reference4(), engine4(gemm)
    L = r["cfg"].n_layers
    random.seed(3)
    prompts = tvr_amd.prompts.sample_icl_prompts(model, r["contexts"], ARROW, None, 6, 3)
    n = len(prompts)
    trace = filled_trace(model, prompts)
    per_prompt = model.capture_resid(trace, groups=list(range(n)), n_groups=n)  # [n, L + 1, d]
    for l in range(L + 1):
        last = [o + t - 1 for o, t in zip(trace.seq_offsets, trace.seq_lens)]
        assert torch.equal(per_prompt[:, l], trace.resid_pre(l)[last])
    T = np.asarray([len(p) for p in prompts])
    s3 = tvr_amd.make_sites(2 * n * L)
    s3["kind"] = KIND3
    s3["seq"] = np.tile(np.repeat(np.arange(n), L), 2)
    s3["layer"] = np.tile(np.arange(L), 2 * n)
    s3["src_seq"] = np.concatenate([np.repeat(np.arange(n), L), np.repeat((np.arange(n) + 1) % n, L)])
    s3["pos"], s3["src_pos"] = T[s3["seq"]] - 1, T[s3["src_seq"]] - 1
    s3["target"] = np.asarray([p[1] for p in prompts])[s3["seq"]]
    s6 = s3.copy()
    s6["kind"], s6["vec"] = KIND6, s3["src_seq"] * (L + 1) + s3["layer"]
    s6["src_seq"] = s6["src_pos"] = 0
    out3 = model.patch_sweep(trace, s3, None, topk=3, return_logits=True)
    out6 = model.patch_sweep(trace, s6, per_prompt, topk=3, return_logits=True)
    none = tvr_amd.make_sites(n)
    none["seq"], none["target"] = np.arange(n), [p[1] for p in prompts]
    clean = model.patch_sweep(trace, none, None, topk=3, return_logits=True)
    for k in ("logits", "prob", "topk"):
        assert torch.equal(out3[k], out6[k]), k
    for k in ("logits", "prob"):  # a prompt's own vector: the clean result (recomputed from layer l: fp32 rounding)
        own = out6[k][: n * L].view(n, L, -1)
        assert rel_err(own, clean[k].view(n, 1, -1).expand_as(own)) <= FP32_TOL, k
    assert not torch.equal(out6["logits"][n * L:], out6["logits"][: n * L])  # the cross patches do change something


# ------------------------------------------------------------------------ 6. errors
def test_errors_leave_the_model_usable(tiny_model):
    model, cfg = tiny_model, tiny_model.cfg
    prompts = ragged_prompts(cfg, [5, 3])
    trace = filled_trace(model, prompts)
    vecs = torch.randn(2, cfg.d_model, device="cuda")

    def site(**kw):
        s = tvr_amd.make_sites(1)
        s["kind"], s["pos"] = KIND6, 4
        for k, v in kw.items():
            s[k] = v
        return s

    good = site()
    want = model.patch_sweep(trace, good, vecs, return_logits=True)["logits"].clone()
    for bad, args, msg in ((site(pos=5), (vecs,), "resid patch out of range"),     # pos = T
                           (site(pos=-1), (vecs,), "resid patch out of range"),
                           (site(layer=cfg.n_layers), (vecs,), "resid patch out of range"),
                           (site(vec=2), (vecs,), "vector out of range"),           # vec = n_vectors
                           (good, (None,), "vector out of range")):                 # vectors = None
        with pytest.raises((ValueError, _lib.EngineError), match=msg):
            model.patch_sweep(trace, bad, *args)
        with pytest.raises((ValueError, _lib.EngineError), match=msg):
            model.patch_sweep_sets(trace, bad, np.zeros(2, np.int32), np.zeros((0, 3), np.int32), *args)
        assert torch.equal(model.patch_sweep(trace, good, vecs, return_logits=True)["logits"], want)
    ok = model.capture_resid(trace).clone()
    n = len(prompts)
    for kw in (dict(positions=[5, 0]),                       # a pos past the sequence
               dict(positions=[0, -1]),
               dict(groups=[0, 2], n_groups=2),               # group = n_groups
               dict(groups=[0, -1], n_groups=2),
               dict(n_groups=0),
               dict(positions=[0]),
               dict(out=torch.zeros(1, cfg.n_layers, cfg.d_model, device="cuda"))):
        with pytest.raises((ValueError, _lib.EngineError)):
            model.capture_resid(trace, **kw)
        assert torch.equal(model.capture_resid(trace), ok)
    # the engine's own validation (the façade's host checks bypassed): before any device call
    out = torch.zeros(2, cfg.n_layers + 1, cfg.d_model, device="cuda")
    i32 = dict(dtype=torch.int32)
    for pos, grp, msg in ((torch.tensor([5, 0], **i32), None, "pos of sequence 0 out of range"),
                          (None, torch.tensor([0, 2], **i32), "group of sequence 1 out of range")):
        with pytest.raises(ValueError, match=msg):
            model._ops.capture_resid(trace._h.value, pos, grp, 2, n, out)
    assert out.abs().max().item() == 0.0
    empty = model.trace(2, 8)
    with pytest.raises(ValueError, match="trace is empty"):
        model._ops.capture_resid(empty._h.value, None, None, 2, n, out)
    with pytest.raises(ValueError, match="trace is empty"):
        model.capture_resid(empty)
    assert torch.equal(model.capture_resid(trace), ok)
