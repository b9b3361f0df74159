"""GPU: joint head-set patching (tvr_patch_sweep_sets, kinds
TVR_SITE_REPLACE_HEADSET_ALLPOS / _LASTPOS) against the CPU oracle's
``run_with_hooks`` with one ``hook_result`` hook per set member.

Configs (weights ``synth_hf_state_dict(cfg, seed=0, std=0.15)``): tiny4 (the
tiny model with 4 layers) on every GEMM path, dh80 (d_head 80: 160-byte z
slices) on x2f16 with processed and with exact-fp16 weights.  48 cases per
config = 4 prompts x 2 position modes x 6 sets, run ONCE as a single mixed
launch against a filled trace and once as the fused (deferred clean) sweep.

Bars (tests/test_gpu_engine.py's): fp32-accurate paths logits 1e-4 of
max|ref|, probabilities 1e-5 of the largest softmax value; bf16 2e-2 for both.
On EVERY config, bf16 included, the top-3 ids equal the fp64 reference's
wherever its adjacent gaps among its top four logits exceed 4e-4 max|logit|,
and at most 2 of the 48 cases may be exempt by that rule (the reference alone
exempts 0 / 1 / 1 on tiny4 / dh80 / dh80-fp16); in every case the returned
top-3 is also the top-3 of the returned logits.

The set ``[(1,1),(2,1),(L-1,1)]`` names (2,1) twice on the 3-layer dh80
config; the engine rejects duplicates, and two identical hooks equal one, so
the sets are de-duplicated in order (dh80 runs ``[(1,1),(2,1)]``).
"""
import functools
import random

import numpy as np
import pytest
import torch

import tvr_amd
from conftest import make_oracle
from oracle import reference_experiments as R

pytestmark = pytest.mark.gpu

KIND = {"all": tvr_amd._lib.SITE_REPLACE_HEADSET_ALLPOS, "last": tvr_amd._lib.SITE_REPLACE_HEADSET_LASTPOS}
BF16_TOL = 2e-2
FP32_TOL, FP32_PROB_TOL = 1e-4, 1e-5
TOP3_GAP, MAX_EXEMPT = 4e-4, 2  # every config, bf16 included
CASES = [("tiny4", "x2f16", False), ("tiny4", "x3bf16", False), ("tiny4", "f32", False), ("tiny4", "bf16", False),
         ("dh80", "x2f16", False), ("dh80", "x2f16", True)]
IDS = [f"{c}-{g}{'-exact16' if x else ''}" for c, g, x in CASES]


def rel_err(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def config(name):
    if name == "tiny4":
        return tvr_amd.get_config("tiny").with_(n_layers=4)
    return tvr_amd.PythiaConfig(3, 320, 4, 640, 512, n_ctx=256)


def head_sets(cfg):
    L, H = cfg.n_layers, cfg.n_heads
    sets = [[], [(1, 2)], [(0, 0), (0, 3), (2, 1)], [(0, h) for h in range(H)] + [(L - 1, 1)],
            [(L - 1, 0), (L - 1, 2)], [(1, 1), (2, 1), (L - 1, 1)]]
    return [list(dict.fromkeys(s)) for s in sets]  # (module docstring: dh80's last set)


def hooks_for(members, mode, vecs, H):
    out = []
    for l, h in members:
        def hook(hv, hook, h=h, v=vecs[l * H + h]):
            if mode == "all":
                hv[0, :, h, :] = v
            else:
                hv[0, -1, h, :] = v
            return hv
        out.append((f"blocks.{l}.attn.hook_result", hook))
    return out


def hooked(oracle, prompt, members, mode, vecs):
    """Last-position logits of ``prompt`` with one hook_result hook per member."""
    saved = oracle.cfg.use_attn_result
    oracle.cfg.use_attn_result = True
    try:
        return oracle.run_with_hooks(torch.tensor([prompt]), fwd_hooks=hooks_for(members, mode, vecs.to(oracle.dtype),
                                                                                 oracle.cfg.n_heads))[0, -1]
    finally:
        oracle.cfg.use_attn_result = saved


@functools.lru_cache(maxsize=None)
def reference(name, fp16):
    """Oracles (fp32: the bars; fp64: the top-3 gap rule), inputs and the 48
    reference rows of one config, computed once."""
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    cfg = config(name)
    sd = tvr_amd.weights.synth_hf_state_dict(cfg, seed=0, std=0.15, fp16=fp16)
    tok = tvr_amd.tokenizer.SyntheticTokenizer(cfg.d_vocab)
    o32, o64 = make_oracle(cfg, sd, tok), make_oracle(cfg, sd, tok, torch.float64)
    g = torch.Generator().manual_seed(21)
    prompts = [[0] + torch.randint(1, cfg.d_vocab, (n - 1,), generator=g).tolist() for n in (3, 7, 12, 30)]
    vecs = torch.randn(cfg.n_layers * cfg.n_heads, cfg.d_model, generator=torch.Generator().manual_seed(3))
    cases = [(i, mode, s) for i in range(len(prompts)) for mode in ("all", "last") for s in head_sets(cfg)]
    ref32 = [hooked(o32, prompts[i], s, mode, vecs) for i, mode, s in cases]
    ref64 = [hooked(o64, prompts[i], s, mode, vecs) for i, mode, s in cases]
    return dict(cfg=cfg, sd=sd, tok=tok, o32=o32, o64=o64, prompts=prompts, vecs=vecs, cases=cases, ref32=ref32,
                ref64=ref64)


@functools.lru_cache(maxsize=None)
def engine(name, gemm, fp16):
    r = reference(name, fp16)
    m = tvr_amd.Model.from_hf_state_dict(r["cfg"], r["sd"], device="cuda", tokenizer=r["tok"], gemm=gemm)
    assert m.exact16 == fp16
    return m


def set_tables(cfg, cases, prompts):
    """(sites, set_off, patches) of the cases: one mixed launch."""
    H = cfg.n_heads
    sites = tvr_amd.make_sites(len(cases))
    off, pat = [0], []
    for k, (i, mode, s) in enumerate(cases):
        sites[k]["seq"], sites[k]["kind"], sites[k]["target"] = i, KIND[mode], prompts[i][1]
        pat += [(l, h, l * H + h) for l, h in s]
        off.append(len(pat))
    return sites, np.asarray(off, dtype=np.int32), np.asarray(pat, dtype=np.int32).reshape(-1, 3)


def sweep(model, r, defer, **kw):
    prompts = r["prompts"]
    trace = model.trace(len(prompts), sum(map(len, prompts)))
    model.forward_clean(prompts, trace=trace, defer=defer)
    sites, off, pat = set_tables(r["cfg"], r["cases"], prompts)
    return model.patch_sweep_sets(trace, sites, off, pat, r["vecs"].cuda(), **kw), sites


@pytest.mark.parametrize("name,gemm,fp16", CASES, ids=IDS)
def test_head_sets_against_hooks(name, gemm, fp16):
    r = reference(name, fp16)
    model = engine(name, gemm, fp16)
    bf16 = gemm == "bf16"
    tol, ptol = (BF16_TOL, BF16_TOL) if bf16 else (FP32_TOL, FP32_PROB_TOL)
    for defer in (False, True):
        out, sites = sweep(model, r, defer, topk=3, return_logits=True)
        exempt, worst, worst_p, wrong = 0, 0.0, 0.0, []
        for j, (ref, ref64) in enumerate(zip(r["ref32"], r["ref64"])):
            case = (defer, j, r["cases"][j])
            e = rel_err(out["logits"][j], ref)
            sm = torch.softmax(ref, 0)
            ep = abs(out["prob"][j].item() - sm[int(sites[j]["target"])].item()) / sm.max().item()
            worst, worst_p = max(worst, e), max(worst_p, ep)
            assert e < tol, (case, e)
            assert ep <= ptol, (case, ep)
            # the set sweep's own top-k against its own logits, every case
            assert out["topk"][j].tolist() == torch.topk(out["logits"][j], 3).indices.tolist(), case
            top4 = torch.topk(ref64, 4)
            gaps = top4.values[:-1] - top4.values[1:]
            if gaps.min().item() > TOP3_GAP * ref64.abs().max().item():
                if out["topk"][j].tolist() != top4.indices[:3].tolist():
                    wrong.append((case, out["topk"][j].tolist(), top4.indices[:3].tolist(),
                                  f"gap {gaps.min().item() / ref64.abs().max().item():.2e}"))
            else:
                exempt += 1
        print(f"{name}-{gemm} fp16={fp16} defer={defer}: logits {worst:.2e} prob {worst_p:.2e} exempt {exempt} "
              f"top-3 mismatches {len(wrong)}")
        for w in wrong:
            print("  top-3 mismatch:", w)
        assert not wrong, wrong
        assert exempt <= MAX_EXEMPT, exempt


def _tiny4(gemm="x2f16"):
    return reference("tiny4", False), engine("tiny4", gemm, False)


def test_empty_set_equals_site_none_bitwise():
    r, model = _tiny4()
    prompts = r["prompts"]
    trace = model.trace(len(prompts), sum(map(len, prompts)))
    model.forward_clean(prompts, trace=trace)
    n = len(prompts)
    sites = tvr_amd.make_sites(3 * n)
    sites["seq"] = np.tile(np.arange(n), 3)
    sites["kind"] = np.repeat([0, KIND["all"], KIND["last"]], n)
    sites["target"] = [p[1] for p in prompts] * 3
    out = model.patch_sweep_sets(trace, sites, np.zeros(3 * n + 1, np.int32), np.zeros((0, 3), np.int32),
                                 r["vecs"].cuda(), topk=3, return_logits=True)
    for k in ("logits", "prob", "topk"):
        v = out[k].view(3, n, -1)
        assert torch.equal(v[0], v[1]) and torch.equal(v[0], v[2]), k
    # without any set site the call is the plain sweep
    plain = model.patch_sweep(trace, sites[:n], None, topk=3, return_logits=True)
    assert torch.equal(plain["logits"], out["logits"][:n])


@pytest.mark.parametrize("defer", [False, True])
def test_set_sweep_twice_is_bitwise_identical(defer):
    r, model = _tiny4()
    a, _ = sweep(model, r, defer, topk=3, return_logits=True)
    b, _ = sweep(model, r, defer, topk=3, return_logits=True)
    for k in ("logits", "prob", "topk"):
        assert torch.equal(a[k], b[k]), k


def test_unaligned_vectors_take_the_elementwise_kernel():
    """``vectors`` as a 4-byte-offset view: the element-wise variant of the
    head-set kernel adds the same fp32 values in the same order."""
    r, model = _tiny4()
    a, _ = sweep(model, r, False, return_logits=True)
    prompts = r["prompts"]
    trace = model.trace(len(prompts), sum(map(len, prompts)))
    model.forward_clean(prompts, trace=trace)
    sites, off, pat = set_tables(r["cfg"], r["cases"], prompts)
    store = torch.zeros(r["vecs"].numel() + 1, device="cuda")
    view = store[1:].view_as(r["vecs"])
    view.copy_(r["vecs"])
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    b = model.patch_sweep_sets(trace, sites, off, pat, view, return_logits=True)
    assert torch.equal(a["logits"], b["logits"])
    # a kind-1 site reads vectors with 16-byte loads: refused on such a view, before any launch
    one = tvr_amd.make_sites(1)
    one["kind"], one["layer"] = tvr_amd._lib.SITE_REPLACE_HEAD_ALLPOS, 1
    with pytest.raises(ValueError, match="16-byte"):
        model.patch_sweep_sets(trace, one, [0, 0], np.zeros((0, 3), np.int32), view)


def _old_kind_sites(cfg, prompts):
    """Kinds 1, 2, 3 on every prompt.  (The REPLACE_HEAD sites enter at layers
    2 and 3, where other kinds enter too: no linearised entry here; that is
    test_linearised_entry_layer_with_set_patches.)"""
    rows = []
    for i, p in enumerate(prompts):
        T = len(p)
        rows += [dict(seq=i, kind=1, layer=1 + i % 2, head=i % cfg.n_heads, vec=i),
                 dict(seq=i, kind=1, layer=1 + i % 2, head=(i + 1) % cfg.n_heads, vec=i + 4),
                 dict(seq=i, kind=2, layer=i % cfg.n_layers, vec=2),
                 dict(seq=i, kind=3, layer=(i + 1) % cfg.n_layers, pos=T // 2, src_seq=(i + 1) % len(prompts),
                      src_pos=len(prompts[(i + 1) % len(prompts)]) // 3)]
    sites = tvr_amd.make_sites(len(rows))
    for s, row in zip(sites, rows):
        for k, v in row.items():
            s[k] = v
        s["target"] = prompts[row["seq"]][1]
    return sites


@pytest.mark.parametrize("defer", [False, True])
def test_mixed_launch_leaves_old_kinds_bitwise(defer):
    """Kinds 1, 2, 3 interleaved with set sites (kind 4 and 5) in one launch:
    the old kinds' results are bitwise those of patch_sweep on them alone."""
    r, model = _tiny4()
    cfg, prompts, vecs = r["cfg"], r["prompts"], r["vecs"].cuda()
    old = _old_kind_sites(cfg, prompts)
    s_sites, s_off, s_pat = set_tables(cfg, r["cases"], prompts)
    n_old, n_set = len(old), len(s_sites)
    # interleave: an old site, then three set sites, ...
    order = sorted(range(n_old + n_set), key=lambda k: (k * 3 if k < n_old else k - n_old, k >= n_old))
    mixed = tvr_amd.make_sites(n_old + n_set)
    off, pat = [0], []
    for dst, k in enumerate(order):
        if k < n_old:
            mixed[dst] = old[k]
        else:
            mixed[dst] = s_sites[k - n_old]
            pat += s_pat[s_off[k - n_old]:s_off[k - n_old + 1]].tolist()
        off.append(len(pat))
    is_old = torch.tensor([k < n_old for k in order])
    assert is_old.sum() == n_old and not is_old[1:4].any()

    def run(fn, *a):
        trace = model.trace(len(prompts), sum(map(len, prompts)))
        model.forward_clean(prompts, trace=trace, defer=defer)
        return fn(trace, *a, topk=3, return_logits=True)

    alone = run(model.patch_sweep, old, vecs)
    both = run(model.patch_sweep_sets, mixed, off, np.asarray(pat, np.int32).reshape(-1, 3), vecs)
    for k in ("logits", "prob", "topk"):
        assert torch.equal(both[k][is_old], alone[k]), k
    sets_alone = run(model.patch_sweep_sets, s_sites, s_off, s_pat, vecs)
    for k in ("logits", "prob", "topk"):
        assert torch.equal(both[k][~is_old], sets_alone[k]), k


@pytest.mark.parametrize("gemm", ["x2f16", "bf16"])
def test_linearised_entry_layer_with_set_patches(gemm):
    """A fused sweep whose layer 1 is a linearised entry layer (only
    REPLACE_HEAD sites of layer 0 enter there) while set sites that entered at
    layer 0 have heads at layer 1: run_block_lin, then the head-set patch, then
    the O + MLP-out GEMM.  Every site against the oracle's hooks, and the
    profile shows that the linearised entry ran."""
    r, model = _tiny4(gemm)
    cfg, prompts, vecs, o32 = r["cfg"], r["prompts"], r["vecs"], r["o32"]
    H = cfg.n_heads
    members = {"all": [(0, 1), (1, 0), (1, 3)], "last": [(0, 2), (1, 2)]}
    rows, want = [], []
    for i, p in enumerate(prompts):
        h = i % H
        rows.append((dict(seq=i, kind=1, layer=0, head=h, vec=h), []))  # enters at layer 1
        want.append(hooked(o32, p, [(0, h)], "all", vecs))
        for mode, s in members.items():
            rows.append((dict(seq=i, kind=KIND[mode]), s))
            want.append(hooked(o32, p, s, mode, vecs))
    sites = tvr_amd.make_sites(len(rows))
    off, pat = [0], []
    for site, (fields, s) in zip(sites, rows):
        for k, v in fields.items():
            site[k] = v
        site["target"] = prompts[fields["seq"]][1]
        pat += [(l, hh, l * H + hh) for l, hh in s]
        off.append(len(pat))
    trace = model.trace(len(prompts), sum(map(len, prompts)))
    model.forward_clean(prompts, trace=trace, defer=True)
    model.profile(True)
    try:
        out = model.patch_sweep_sets(trace, sites, off, pat, vecs.cuda(), return_logits=True)
        torch.cuda.synchronize()
        hbm = model.profile_hbm_stats()
    finally:
        model.profile(False)
    assert hbm["lin_entry"]["launches"] >= 1, hbm["lin_entry"]
    tol = BF16_TOL if gemm == "bf16" else FP32_TOL
    errs = [rel_err(out["logits"][j], ref) for j, ref in enumerate(want)]
    print(f"lin entry + set patches {gemm}: worst logits {max(errs):.2e}")
    assert max(errs) < tol, errs


def test_bad_arguments_raise_value_error():
    r, model = _tiny4()
    prompts = r["prompts"]
    trace = model.trace(len(prompts), sum(map(len, prompts)))
    model.forward_clean(prompts, trace=trace)
    vecs = r["vecs"].cuda()
    one = tvr_amd.make_sites(1)
    one["kind"] = KIND["all"]
    with pytest.raises(ValueError, match="tvr_patch_sweep_sets"):
        model.patch_sweep(trace, one, vecs)
    with pytest.raises(ValueError, match="twice"):
        model.patch_sweep_sets(trace, one, [0, 2], [(1, 2, 0), (1, 2, 1)], vecs)
    L, H, n_vec = r["cfg"].n_layers, r["cfg"].n_heads, vecs.shape[0]
    for bad in [(L, 0, 0), (-1, 0, 0), (0, H, 0), (0, 0, n_vec), (0, 0, -1)]:
        with pytest.raises(ValueError, match="out of range"):
            model.patch_sweep_sets(trace, one, [0, 1], [bad], vecs)
    with pytest.raises(ValueError, match="set_off"):
        model.patch_sweep_sets(trace, one, [0, 2], [(1, 2, 0)], vecs)  # runs past patches
    two = tvr_amd.make_sites(2)
    two["kind"] = KIND["last"]
    with pytest.raises(ValueError, match="set_off"):
        model.patch_sweep_sets(trace, two, [1, 0, 1], [(1, 2, 0)], vecs)  # decreases
    two["kind"] = [tvr_amd._lib.SITE_NONE, KIND["last"]]
    with pytest.raises(ValueError, match="own patches"):
        model.patch_sweep_sets(trace, two, [0, 1, 1], [(1, 2, 0)], vecs)  # a kind-0 site with a patch
    # the trace is still usable after the refusals
    ok = model.patch_sweep_sets(trace, one, [0, 1], [(1, 2, 0)], vecs)
    assert torch.isfinite(ok["prob"]).all()


@pytest.mark.parametrize("name,gemm,fp16", [("tiny4", "x2f16", False), ("tiny4", "f32", False),
                                            ("dh80", "x2f16", True)], ids=["tiny4-x2f16", "tiny4-f32", "dh80-exact16"])
def test_singleton_sets_reproduce_the_cie(name, gemm, fp16):
    """All-positions singleton sets over every (l, h) = the CIE sweep: each
    engine path within the CIE bar (1e-4 max|CIE| + 1e-7) of the oracle, the
    two engine paths within twice that of each other."""
    r = reference(name, fp16)
    model = engine(name, gemm, fp16)
    cfg = r["cfg"]
    L, H = cfg.n_layers, cfg.n_heads
    prompts = r["prompts"][:3]
    answers = [[int(r["o32"].forward(torch.tensor([p]))[0, -1].argmax())] for p in prompts]
    mean = r["vecs"].view(L, H, cfg.d_model)
    ref = R.calculate_average_causal_indirect_effect(mean, prompts, answers, r["o32"]).double()
    cie = tvr_amd.calculate_average_causal_indirect_effect(mean.cuda(), prompts, answers, model=model).cpu().double()
    sets = [[(l, h)] for l in range(L) for h in range(H)]
    joint = tvr_amd.joint_head_patch_effect(mean.cuda(), sets, prompts, answers, model=model)
    dprob = joint["dprob"].cpu().double().view(L, H)
    bar = 1e-4 * ref.abs().max().item() + 1e-7
    errs = [(cie - ref).abs().max().item(), (dprob - ref).abs().max().item(), (dprob - cie).abs().max().item()]
    print(f"{name}-{gemm}: CIE sweep {errs[0]:.2e} set sweep {errs[1]:.2e} between {errs[2]:.2e} bar {bar:.2e}")
    assert errs[0] <= bar and errs[1] <= bar and errs[2] <= 2 * bar, (errs, bar)


def _loop_effect(oracle, mean, sets, prompts, answers, mode, topk):
    """joint_head_patch_effect restated as plain loops over run_with_hooks
    (and the largest softmax value met: the probability bar's scale)."""
    vecs = mean.reshape(-1, mean.shape[-1])
    dprob, acc = [0.0] * len(sets), [0] * len(sets)
    clean_p = clean_acc = pmax = 0.0
    for p, a in zip(prompts, answers):
        logits = oracle.forward(torch.tensor([p]))[0, -1]
        p0 = torch.softmax(logits, 0)[a].item()
        pmax = max(pmax, torch.softmax(logits, 0).max().item())
        clean_p += p0
        clean_acc += a in torch.topk(logits, topk).indices.tolist()
        for k, s in enumerate(sets):
            lg = hooked(oracle, p, s, mode, vecs)
            dprob[k] += torch.softmax(lg, 0)[a].item() - p0
            pmax = max(pmax, torch.softmax(lg, 0).max().item())
            acc[k] += a in torch.topk(lg, topk).indices.tolist()
    n = len(prompts)
    return [x / n for x in dprob], [x / n for x in acc], clean_p / n, clean_acc / n, pmax


@pytest.mark.parametrize("mode", ["all", "last"])
def test_facade_matches_hook_loops(mode):
    r, model = _tiny4()
    cfg, oracle = r["cfg"], r["o32"]
    L, H = cfg.n_layers, cfg.n_heads
    prompts = r["prompts"]
    answers = [int(oracle.forward(torch.tensor([p]))[0, -1].argmax()) for p in prompts]
    mean = r["vecs"].view(L, H, cfg.d_model)
    sets = head_sets(cfg)
    got = tvr_amd.joint_head_patch_effect(mean.cuda(), sets, prompts, [[a] for a in answers], model=model,
                                          positions=mode, topk=2)
    dp, acc, cp, ca, pmax = _loop_effect(oracle, mean, sets, prompts, answers, mode, 2)
    assert got["accuracy"].tolist() == acc and got["clean_accuracy"] == ca
    assert abs(got["clean_prob"] - cp) <= FP32_PROB_TOL * pmax
    assert (got["dprob"].cpu().double() - torch.tensor(dp).double()).abs().max().item() <= FP32_PROB_TOL * pmax

    # the ablation curve: top-k of a CIE map with ties, plus seeded controls
    cie = torch.randint(0, 4, (L, H), generator=torch.Generator().manual_seed(9)).float()
    counts, layer, seed = (1, 2, 5), L - 2, 4
    curve = tvr_amd.head_ablation_curve(mean.cuda(), cie, prompts, answers, model=model, counts=counts, layer=layer,
                                        n_random=2, seed=seed, positions=mode)
    tops = []
    for k in counts:
        _, idx = torch.topk(cie[: layer + 1].flatten(), k)
        tops.append([(int(i) // H, int(i) % H) for i in idx])
    rng = random.Random(seed)
    pool = [(l, h) for l in range(layer + 1) for h in range(H)]
    ctrl = [[rng.sample(pool, k) for _ in range(2)] for k in counts]
    assert curve["heads"] == tops and curve["random_heads"] == ctrl
    dp, acc, cp, ca, pmax = _loop_effect(oracle, mean, tops + [s for c in ctrl for s in c], prompts, answers, mode, 1)
    nk = len(counts)
    assert curve["top"]["accuracy"].tolist() == acc[:nk]
    assert curve["random"]["accuracy"].flatten().tolist() == acc[nk:] and curve["clean_accuracy"] == ca
    both = torch.cat([curve["top"]["dprob"], curve["random"]["dprob"].flatten()]).cpu().double()
    assert (both - torch.tensor(dp).double()).abs().max().item() <= FP32_PROB_TOL * pmax
