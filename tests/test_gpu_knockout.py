"""GPU: attention knockout (tvr_attention_knockout, tvr_patch_sweep_knockout, kind
TVR_SITE_ATTN_KNOCKOUT_LASTPOS) against the fp64 references of knockout_cases.py
and the CPU oracle's hooked forwards.

The kernel alone (tests 1-4), on attention_cases.MODELS (d_head 16 / 64 / 80 / 128,
including 6 x 16 and 3 x 128 heads) and T in knockout_cases.ALL_T, one item per
(sequence, head) of a launch with a whole sequence, one computed row behind a
cache prefix and a follower of the first sequence:
1. every blocked-set family against fp64: fp32 and the two x2f16 formats to the
   case's bar (knockout_cases.bar: 4 x the larger error of two fp32
   restatements), bf16 to that bar plus 2^-8 max |z64| (bf16 keeps 8 significant
   bits: a rounding of at most 2^-9 |z|, margin 2), and every format bit for bit
   tvr_act_rows of the fp32 z;
2. z is pre-filled with random bits: every byte outside the listed (row, head)
   slices is unchanged, the MLP columns and bf16's second plane included;
3. one-hot scores with the best key blocked: the slice is the runner-up's V row
   bit for bit;
4. an item alone equals the same item among 33, and a launch run twice is identical.

The sweep (tests 5-9), configs of tests/test_gpu_head_sets.py: 4 prompts x 6
(members, blocked) cases in one launch, on a filled trace and deferred, logits
within 1e-4 of max |ref| and probabilities within 1e-5 of the largest softmax
value (bf16 2e-2 both), the returned top-3 the top-3 of the returned logits;
knocked and clean fp64 logits differ by more than 100 x that logit bar in every
case (tests/test_knockout_cases.py), so an engine that ignored the knockout
fails; empty member or key lists equal TVR_SITE_NONE bit for bit, old kinds in a
knockout launch equal tvr_patch_sweep_sets, a sweep run twice is identical, a
linearised entry layer under knockout members, and the two façade functions
against loops of hooked oracle forwards.
"""
import ctypes
import functools
import gc
import random

import numpy as np
import pytest
import torch

import attention_cases as A
import knockout_cases as K
import tvr_amd
from conftest import make_oracle
from test_gpu_attention import BF16, F32, FMT_NAME, G, IL, X2F16, Ctx, guarded, logical, seq_array

pytestmark = [pytest.mark.gpu]

L = tvr_amd._lib
KO = L.SITE_ATTN_KNOCKOUT_LASTPOS
MODEL_IDS = [f"dh{dh}h{h}" for dh, h in K.MODELS]
FP32_TOL, FP32_PROB_TOL, BF16_TOL = K.LOGIT_TOL, K.PROB_TOL, K.BF16_TOL
BF16_EPS = 2.0 ** -8


@functools.lru_cache(maxsize=None)
def _ctx(model):
    return Ctx(*model)


@pytest.fixture(scope="module", autouse=True)
def _module():
    yield
    for cache in (_ctx, _ref, reference, engine):
        cache.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(params=K.MODELS, ids=MODEL_IDS)
def ctx(request):
    return _ctx(request.param)


@functools.lru_cache(maxsize=None)
def _ref(model, T, family):
    """(case, items, z64, bar) of one launch, computed once."""
    c = _ctx(model)
    case = _case(model, T)
    items = K.items_of(case, family, c.cos, c.sin)
    if not items:
        return case, items, None, None
    z64 = K.reference(case, items, c.cos, c.sin)
    return case, items, z64, K.bar(case, items, c.cos, c.sin, z64)[0]


@functools.lru_cache(maxsize=None)
def _case(model, T):
    return K.make(model, T)


def item_array(items):
    rows, keys = K.tables_of(items)
    arr = (L.CKnockoutItem * len(items))(*[L.CKnockoutItem(int(s), int(m), int(f), int(n)) for s, m, f, n in rows])
    return arr, keys


def launch(ctx, case, items, fmt=F32, tables=True, expect_range=False, seed=5):
    """One tvr_attention_knockout launch on guarded buffers whose z holds random bits.  Asserts that nothing
    outside the listed (row, head) slices changed.  Returns (slices, zbuf): fp32 [n_items][DH], or the halves
    [n_items][2][DH] of the other formats, and the device buffer."""
    lay, d, K2, DH = case.lay, case.d, ctx.K2, ctx.DH
    rows = lay.rows
    if not hasattr(case, "dev"):
        case.dev = (guarded(torch.from_numpy(case.qkv), float("nan")), guarded(torch.from_numpy(case.cache), float("nan")))
    qkv, cache = case.dev
    g = torch.Generator().manual_seed(seed)
    if fmt == F32:
        sent = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows + 2 * G, K2), generator=g, dtype=torch.int64).to(torch.int32)
    else:
        sent = torch.randint(-2 ** 15, 2 ** 15 - 1, (rows + 2 * G, 2 * K2), generator=g, dtype=torch.int64).to(torch.int16)
    zbuf = sent.cuda()
    off = lambda t: t.data_ptr() + G * t.stride(0) * t.element_size()
    arr, keys = item_array(items)
    rc = ctx.lib.tvr_attention_knockout(ctx.h, fmt, off(qkv), off(cache), seq_array(lay.seqs), lay.n_seq, rows,
                                        lay.cache_rows, arr, len(items), keys.ctypes.data, len(keys), off(zbuf),
                                        ctx.d_cos.data_ptr() if tables else 0, ctx.d_sin.data_ptr() if tables else 0,
                                        ctx.stream())
    L.check(rc, "tvr_attention_knockout")
    flag = ctx.lib.tvr_model_range_status(ctx.h, ctx.stream())
    assert flag == (L.TVR_ERR_RANGE if expect_range else L.TVR_OK), f"range flag {flag} ({FMT_NAME[fmt]})"
    listed = np.zeros((rows, K2), dtype=bool)
    where = []
    for it in items:
        sd = lay.seqs[it.seq]
        r, c = sd.row0 + sd.n - 1, slice(it.head * DH, (it.head + 1) * DH)
        assert not listed[r, c].any()
        listed[r, c] = True
        where.append((r, c))
    got, was = zbuf.cpu().numpy(), sent.numpy()
    assert np.array_equal(got[:G], was[:G]) and np.array_equal(got[-G:], was[-G:]), "z guard rows written"
    if fmt == F32:
        a, b = got[G:-G], was[G:-G]
        assert np.array_equal(a[~listed], b[~listed]), "bytes outside the listed slices changed"
        return np.stack([a[r, c].view(np.float32) for r, c in where]), zbuf
    a, b = logical(got[G:-G].view(np.uint16), fmt, K2), logical(was[G:-G].view(np.uint16), fmt, K2)
    for pl in (0, 1):
        keep = ~listed if (pl == 0 or fmt != BF16) else np.ones_like(listed)
        assert np.array_equal(a[:, pl][keep], b[:, pl][keep]), f"plane {pl}: bytes outside the listed slices changed"
    return np.stack([a[r][:, c] for r, c in where]), zbuf


def act_rows_of(ctx, fmt, zbuf32, items, lay):
    """tvr_act_rows(fmt) of the fp32-format z (device buffer of ``launch``), the items' slices [n][2][DH]."""
    rows = zbuf32.shape[0] - 2 * G
    clean = torch.nan_to_num(zbuf32.view(torch.float32), nan=0.0, posinf=0.0, neginf=0.0).clamp(-1e3, 1e3).contiguous()
    o = torch.zeros((rows, 2 * ctx.d), dtype=torch.int16, device="cuda")
    L.check(ctx.lib.tvr_act_rows(fmt, clean.data_ptr() + G * ctx.K2 * 4, ctx.K2, o.data_ptr(), rows, ctx.d, 0,
                                 ctx.stream()), "tvr_act_rows")
    torch.cuda.synchronize()
    lg = logical(o.cpu().numpy().view(np.uint16), fmt, ctx.d)
    out = []
    for it in items:
        sd = lay.seqs[it.seq]
        out.append(lg[sd.row0 + sd.n - 1][:, it.head * ctx.DH:(it.head + 1) * ctx.DH])
    return np.stack(out)


def x2_value(planes):
    """x2f16 halves [.., 2, DH] -> fp64 values (split.hpp: (h0 + h1) / 16)."""
    h = planes.view(np.float16).astype(np.float64)
    return (h[..., 0, :] + h[..., 1, :]) / 16.0


def bf16_value(planes):
    return (planes[..., 0, :].astype(np.uint32) << 16).view(np.float32).astype(np.float64)


# ------------------------------------------------------------------ 1, 2: accuracy, formats, untouched bytes
@pytest.mark.parametrize("family", K.FAMILIES)
def test_primitive_against_fp64(ctx, family):
    model = (ctx.DH, ctx.H)
    worst = 0.0
    for T in K.ALL_T:
        case, items, z64, bar = _ref(model, T, family)
        if not items:
            continue
        z, zbuf = launch(ctx, case, items)
        err = np.abs(z.astype(np.float64) - z64)
        err = float("inf") if np.isnan(err).any() else float(err.max())
        print(f"knockout {family} dh {ctx.DH} h {ctx.H} T {T}: err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
        worst = max(worst, err / bar)
        assert err <= bar, (family, T, err, bar)
        for fmt in (X2F16, IL, BF16):
            p, _ = launch(ctx, case, items, fmt=fmt)
            want = act_rows_of(ctx, fmt, zbuf, items, case.lay)
            npl = 1 if fmt == BF16 else 2
            assert np.array_equal(p[:, :npl], want[:, :npl]), (family, T, FMT_NAME[fmt])
            if fmt == BF16:
                e, b = np.abs(bf16_value(p) - z64).max(), bar + BF16_EPS * np.abs(z64).max()
            else:
                e, b = np.abs(x2_value(p) - z64).max(), bar
            assert e <= b, (family, T, FMT_NAME[fmt], e, b)
    print(f"knockout {family} dh {ctx.DH} h {ctx.H}: worst max |dz| / bar {worst:.3f}")


def test_model_tables_and_several_heads_per_item(ctx):
    """cos_t = sin_t = NULL reads the model's own tables (within the bar plus attention's table allowance is
    test_gpu_attention.py's business: here only that the two agree to 1e-5 max |V|), and one item that lists
    every head equals one item per head bit for bit."""
    model = (ctx.DH, ctx.H)
    case, items, z64, bar = _ref(model, 33, "every_other")
    z, _ = launch(ctx, case, items)
    own, _ = launch(ctx, case, items, tables=False)
    assert np.abs(own.astype(np.float64) - z).max() <= 1e-5 * case.max_v()
    lay = case.lay
    rows = np.asarray([(s, (1 << ctx.H) - 1, 0, len(items[0].keys)) for s in range(lay.n_seq)], dtype=np.int64)
    assert all(it.keys == items[0].keys for it in items)
    keys = np.asarray(items[0].keys, dtype=np.int32)
    zb = torch.full((lay.rows + 2 * G, ctx.K2), float("nan"), device="cuda")
    qkv, cache = case.dev
    off = lambda t: t.data_ptr() + G * t.stride(0) * t.element_size()
    arr = (L.CKnockoutItem * len(rows))(*[L.CKnockoutItem(int(a), int(b), int(c), int(d)) for a, b, c, d in rows])
    L.check(ctx.lib.tvr_attention_knockout(ctx.h, F32, off(qkv), off(cache), seq_array(lay.seqs), lay.n_seq, lay.rows,
                                           lay.cache_rows, arr, len(rows), keys.ctypes.data, len(keys), off(zb),
                                           ctx.d_cos.data_ptr(), ctx.d_sin.data_ptr(), ctx.stream()), "knockout")
    got = zb.cpu().numpy()[G:-G]
    for it, want in zip(items, z):
        sd = lay.seqs[it.seq]
        assert np.array_equal(got[sd.row0 + sd.n - 1, it.head * ctx.DH:(it.head + 1) * ctx.DH].view(np.int32),
                              want.view(np.int32))


def test_range_flag(ctx):
    """A V row at 5000 that the knocked query still sees raises the x2f16 flag; fp32 and bf16 do not."""
    model = (ctx.DH, ctx.H)
    base = _case(model, 15)
    hot = A.Case("range", ctx.DH, ctx.H, base.lay, base.qkv.copy(), base.cache)
    sd = hot.lay.seqs[0]
    hot.qkv[sd.row0:sd.row0 + sd.n, 2 * ctx.d:] = 5000.0
    items = [K.Item(0, h, (0,)) for h in range(ctx.H)]
    for fmt in (F32, X2F16, IL, BF16):
        launch(ctx, hot, items, fmt=fmt, expect_range=fmt in (X2F16, IL))


# ------------------------------------------------------------------------------ 3: exact selection
def test_select_is_bitwise(ctx):
    model = (ctx.DH, ctx.H)
    for T in (15, 33, 65, 300):
        case, items, expect = K.make_select(model, T)
        z, zbuf = launch(ctx, case, items)
        assert np.array_equal(z.view(np.int32), expect.view(np.int32)), (T, np.abs(z - expect).max())
        p, _ = launch(ctx, case, items, fmt=IL)
        assert np.array_equal(p, act_rows_of(ctx, IL, zbuf, items, case.lay)), T


# ------------------------------------------------------------------------------ 4: independence
def test_an_item_does_not_depend_on_the_launch(ctx):
    model = (ctx.DH, ctx.H)
    for T, family in ((17, "argmax"), (65, "word_boundary"), (300, "every_other")):
        case, items, _, _ = _ref(model, T, family)
        full, _ = launch(ctx, case, items)
        again, _ = launch(ctx, case, items, seed=6)
        assert np.array_equal(full.view(np.int32), again.view(np.int32)), "a launch run twice differs"
        for x in (0, len(items) // 2, len(items) - 1):
            alone, _ = launch(ctx, case, [items[x]])
            assert np.array_equal(alone[0].view(np.int32), full[x].view(np.int32)), (T, family, x)
    # one item among 33: a wide layout of 33 single-row sequences that share one cache prefix
    T = 40
    lay = A.Layout()
    for _ in range(33):
        lay.add(T, p0=T - 1)
    lay.row_from = 0
    case = A.make("random", ctx.DH, ctx.H, lay, seed=9)
    items = [K.Item(s, s % ctx.H, tuple(range(s % 7, T - 1, 3))) for s in range(33)]
    full, _ = launch(ctx, case, items)
    for x in (0, 16, 32):
        alone, _ = launch(ctx, case, [items[x]])
        assert np.array_equal(alone[0].view(np.int32), full[x].view(np.int32)), x
    z64 = K.reference(case, items, ctx.cos, ctx.sin)
    assert np.abs(full - z64).max() <= K.bar(case, items, ctx.cos, ctx.sin, z64)[0]


def test_invalid_arguments_launch_nothing():
    ctx = _ctx(K.MODELS[0])
    case = _case(K.MODELS[0], 17)
    lay = case.lay
    qkv, cache = torch.from_numpy(case.qkv).cuda(), torch.from_numpy(case.cache).cuda()
    z = torch.full((lay.rows, ctx.K2), float("nan"), device="cuda")
    keys = np.asarray([0, 3, 16], dtype=np.int32)

    def call(msg, items=((0, 1, 0, 2),), status=L.TVR_ERR_INVALID, **kw):
        arr = (L.CKnockoutItem * len(items))(*[L.CKnockoutItem(*i) for i in items])
        a = dict(model=ctx.h, fmt=F32, qkv=qkv.data_ptr(), cache=cache.data_ptr(), seqs=seq_array(lay.seqs),
                 n_seq=lay.n_seq, rows=lay.rows, cache_rows=lay.cache_rows, items=arr, n_items=len(items),
                 keys=keys.ctypes.data, n_keys=len(keys), z=z.data_ptr(), cos=ctx.d_cos.data_ptr(),
                 sin=ctx.d_sin.data_ptr())
        if "arr" in kw:
            a["items"] = kw.pop("arr")
        a.update(kw)
        rc = ctx.lib.tvr_attention_knockout(a["model"], a["fmt"], a["qkv"], a["cache"], a["seqs"], a["n_seq"], a["rows"],
                                            a["cache_rows"], a["items"], a["n_items"], a["keys"], a["n_keys"], a["z"],
                                            a["cos"], a["sin"], ctx.stream())
        err = ctx.lib.tvr_last_error().decode()
        assert rc == status and err.startswith("tvr_attention_knockout: ") and msg in err, (msg, rc, err)

    call("null model", model=None)
    call("null qkv", qkv=None)
    call("null z", z=None)
    call("null seqs", seqs=None)
    call("null items", arr=None)
    call("n_seq must be positive", n_seq=0)
    call("n_items must be positive", n_items=0)
    call("keys is null", keys=None)
    call("unknown fmt", fmt=1)
    call("rows must be positive", rows=0)
    call("outside the qkv buffer", rows=lay.rows - 2)
    call("outside the cache buffer", cache_rows=1)
    call("null cache", cache=None)
    call("both be given or both be null", cos=None)
    call("16-byte aligned", z=z.data_ptr() + 8)
    call("seq out of range", items=((lay.n_seq, 1, 0, 1),))
    call("head mask names a head", items=((0, 1 << ctx.H, 0, 1),))
    call("key range outside the list", items=((0, 1, 2, 2),))
    call("blocked key outside", items=((1, 1, 0, 3),), keys=np.asarray([0, 3, 17], dtype=np.int32).ctypes.data)
    call("strictly increasing", items=((0, 1, 0, 3),), keys=np.asarray([3, 3, 5], dtype=np.int32).ctypes.data)
    all_keys = np.arange(17, dtype=np.int32)
    call("every key is blocked", items=((0, 1, 0, 17),), keys=all_keys.ctypes.data, n_keys=17)
    call("two items list the same head", items=((0, 3, 0, 1), (0, 2, 1, 1)))
    torch.cuda.synchronize()
    assert torch.isnan(z).all()
    call_ok = (L.CKnockoutItem * 1)(L.CKnockoutItem(0, 1, 0, 2))
    L.check(ctx.lib.tvr_attention_knockout(ctx.h, F32, qkv.data_ptr(), cache.data_ptr(), seq_array(lay.seqs), lay.n_seq,
                                           lay.rows, lay.cache_rows, call_ok, 1, keys.ctypes.data, len(keys),
                                           z.data_ptr(), ctx.d_cos.data_ptr(), ctx.d_sin.data_ptr(), ctx.stream()), "ok")
    torch.cuda.synchronize()
    assert int((~torch.isnan(z)).sum()) == ctx.DH


# ------------------------------------------------------------------------------ 5: the sweep against the oracle
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


@functools.lru_cache(maxsize=None)
def reference(name, fp16):
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    cfg = config(name)
    sd = tvr_amd.weights.synth_hf_state_dict(cfg, seed=0, std=0.15, fp16=fp16)
    tok = tvr_amd.tokenizer.SyntheticTokenizer(cfg.d_vocab)
    o32, o64 = make_oracle(cfg, sd, tok), make_oracle(cfg, sd, tok, torch.float64)
    prompts = K.e2e_prompts(cfg)
    cases = [(i, m, k) for i, p in enumerate(prompts) for m, k in K.e2e_cases(cfg, len(p))]
    ref32 = [K.knocked_logits(o32, prompts[i], m, k) for i, m, k in cases]
    vecs = torch.randn(cfg.n_layers * cfg.n_heads, cfg.d_model, generator=torch.Generator().manual_seed(3))
    return dict(cfg=cfg, sd=sd, tok=tok, o32=o32, o64=o64, prompts=prompts, cases=cases, ref32=ref32, vecs=vecs)


@functools.lru_cache(maxsize=None)
def engine(name, gemm, fp16):
    r = reference(name, fp16)
    m = tvr_amd.Model.from_hf_state_dict(r["cfg"], r["sd"], device="cuda", tokenizer=r["tok"], gemm=gemm)
    assert m.exact16 == fp16
    return m


def ko_tables(cases, prompts):
    """(sites, set_off, patches, key_off, keys) of the cases: one launch."""
    sites = tvr_amd.make_sites(len(cases))
    off, pat, koff, keys = [0], [], [0], []
    for k, (i, members, blocked) in enumerate(cases):
        sites[k]["seq"], sites[k]["kind"], sites[k]["target"] = i, KO, prompts[i][1]
        pat += [(l, h, -1) for l, h in members]
        keys += list(blocked)
        off.append(len(pat))
        koff.append(len(keys))
    return (sites, np.asarray(off, np.int32), np.asarray(pat, np.int32).reshape(-1, 3), np.asarray(koff, np.int32),
            np.asarray(keys, np.int32))


def filled(model, prompts, defer):
    trace = model.trace(len(prompts), sum(map(len, prompts)))
    model.forward_clean(prompts, trace=trace, defer=defer)
    return trace


def sweep(model, r, defer, **kw):
    sites, off, pat, koff, keys = ko_tables(r["cases"], r["prompts"])
    return model.patch_sweep_knockout(filled(model, r["prompts"], defer), sites, off, pat, koff, keys, **kw), sites


@pytest.mark.parametrize("name,gemm,fp16", CASES, ids=IDS)
def test_knockout_sweep_against_hooks(name, gemm, fp16):
    r = reference(name, fp16)
    model = engine(name, gemm, fp16)
    tol, ptol = (BF16_TOL, BF16_TOL) if gemm == "bf16" else (FP32_TOL, FP32_PROB_TOL)
    for defer in (False, True):
        out, sites = sweep(model, r, defer, topk=3, return_logits=True)
        worst = worst_p = 0.0
        for j, ref in enumerate(r["ref32"]):
            case = (defer, j, r["cases"][j])
            e = rel_err(out["logits"][j], ref)
            sm = torch.softmax(ref, 0)
            ep = abs(out["prob"][j].item() - sm[int(sites[j]["target"])].item()) / sm.max().item()
            worst, worst_p = max(worst, e), max(worst_p, ep)
            assert e < tol, (case, e)
            assert ep <= ptol, (case, ep)
            assert out["topk"][j].tolist() == torch.topk(out["logits"][j], 3).indices.tolist(), case
        print(f"knockout {name}-{gemm} fp16={fp16} defer={defer}: logits {worst:.2e} prob {worst_p:.2e}")


# ------------------------------------------------------------------------------ 6: bitwise properties
def _tiny4(gemm="x2f16"):
    return reference("tiny4", False), engine("tiny4", gemm, False)


def test_empty_lists_equal_site_none_bitwise():
    r, model = _tiny4()
    prompts, n = r["prompts"], len(r["prompts"])
    trace = filled(model, prompts, False)
    sites = tvr_amd.make_sites(3 * n)
    sites["seq"] = np.tile(np.arange(n), 3)
    sites["kind"] = np.repeat([0, KO, KO], n)
    sites["target"] = [p[1] for p in prompts] * 3
    # block 1: TVR_SITE_NONE; block 2: members but no keys; block 3: keys but no members
    off = np.concatenate([np.zeros(n + 1), np.arange(1, n + 1) * 2, np.full(n, 2 * n)]).astype(np.int32)
    pat = np.asarray([(1, 0, -1), (2, 3, -1)] * n, np.int32)
    koff = np.concatenate([np.zeros(2 * n + 1), np.arange(1, n + 1)]).astype(np.int32)
    keys = np.zeros(n, np.int32)
    model.profile(True)
    try:
        out = model.patch_sweep_knockout(trace, sites, off, pat, koff, keys, topk=3, return_logits=True)
        torch.cuda.synchronize()
        att = model.profile_hbm_stats()["attention"]["launches"]
        plain = model.patch_sweep(trace, sites[:n], None, topk=3, return_logits=True)
        torch.cuda.synchronize()
        att2 = model.profile_hbm_stats()["attention"]["launches"] - att
    finally:
        model.profile(False)
    for k in ("logits", "prob", "topk"):
        v = out[k].view(3, n, -1)
        assert torch.equal(v[0], v[1]) and torch.equal(v[0], v[2]), k
    assert torch.equal(plain["logits"], out["logits"][:n])
    assert att == att2, "empty knockout sites added attention launches"


@pytest.mark.parametrize("defer", [False, True])
def test_knockout_sweep_twice_is_bitwise_identical(defer):
    r, model = _tiny4()
    a, _ = sweep(model, r, defer, topk=3, return_logits=True)
    b, _ = sweep(model, r, defer, topk=3, return_logits=True)
    for k in ("logits", "prob", "topk"):
        assert torch.equal(a[k], b[k]), k


def _old_kind_sites(cfg, prompts):
    """Kinds 1, 2, 3, 6 and the two head-set kinds on every prompt, with their patches."""
    rows = []
    H = cfg.n_heads
    for i, p in enumerate(prompts):
        T = len(p)
        rows += [(dict(seq=i, kind=0), []),
                 (dict(seq=i, kind=1, layer=1 + i % 2, head=i % H, vec=i), []),
                 (dict(seq=i, kind=2, layer=i % cfg.n_layers, vec=2), []),
                 (dict(seq=i, kind=3, layer=(i + 1) % cfg.n_layers, pos=T // 2, src_seq=(i + 1) % len(prompts),
                       src_pos=len(prompts[(i + 1) % len(prompts)]) // 3), []),
                 (dict(seq=i, kind=4), [(0, 1, 1), (2, i % H, 5)]),
                 (dict(seq=i, kind=5), [(1, 2, 3), (3, 0, 7)]),
                 (dict(seq=i, kind=6, layer=2, pos=T - 1, vec=4), [])]
    sites = tvr_amd.make_sites(len(rows))
    off, pat = [0], []
    for s, (row, members) in zip(sites, rows):
        for k, v in row.items():
            s[k] = v
        s["target"] = prompts[row["seq"]][1]
        pat += members
        off.append(len(pat))
    return sites, off, pat


@pytest.mark.parametrize("defer", [False, True])
def test_old_kinds_in_a_knockout_launch_are_bitwise(defer):
    """Kinds 0-6 interleaved with knockout sites: the old kinds' results are those of tvr_patch_sweep_sets on
    them alone, the knockout sites' those of a knockout sweep without the old kinds (but one); and a knockout
    sweep of old kinds only equals tvr_patch_sweep_sets."""
    r, model = _tiny4()
    cfg, prompts, vecs = r["cfg"], r["prompts"], r["vecs"].cuda()
    old, o_off, o_pat = _old_kind_sites(cfg, prompts)
    k_sites, k_off, k_pat, k_koff, k_keys = ko_tables(r["cases"], prompts)
    n_old, n_ko = len(old), len(k_sites)
    order = sorted(range(n_old + n_ko), key=lambda k: (k if k < n_old else (k - n_old) * n_old / n_ko, k >= n_old))
    mixed = tvr_amd.make_sites(n_old + n_ko)
    off, pat, koff, keys = [0], [], [0], []
    for dst, k in enumerate(order):
        if k < n_old:
            mixed[dst] = old[k]
            pat += o_pat[o_off[k]:o_off[k + 1]]
        else:
            j = k - n_old
            mixed[dst] = k_sites[j]
            pat += k_pat[k_off[j]:k_off[j + 1]].tolist()
            keys += k_keys[k_koff[j]:k_koff[j + 1]].tolist()
        off.append(len(pat))
        koff.append(len(keys))
    is_old = torch.tensor([k < n_old for k in order])
    pat = np.asarray(pat, np.int32).reshape(-1, 3)

    def run(fn, *a):
        return fn(filled(model, prompts, defer), *a, topk=3, return_logits=True)

    o_pat_a = np.asarray(o_pat, np.int32).reshape(-1, 3)
    alone = run(model.patch_sweep_sets, old, o_off, o_pat_a, vecs)
    both = run(model.patch_sweep_knockout, mixed, off, pat, koff, keys, vecs)
    # the knockout sites without the other kinds, but for one all-positions site: a launch of one-row sites
    # alone sends them to the single-query attention kernel, another summation order for the untouched heads
    k_plus = np.concatenate([k_sites, old[1:2]])
    assert k_plus[-1]["kind"] == 1
    ko_alone = run(model.patch_sweep_knockout, k_plus, np.append(k_off, k_off[-1]), k_pat,
                   np.append(k_koff, k_koff[-1]), k_keys, vecs)
    old_only = run(model.patch_sweep_knockout, old, o_off, o_pat_a, np.zeros(n_old + 1, np.int32),
                   np.zeros(0, np.int32), vecs)
    for k in ("logits", "prob", "topk"):
        assert torch.equal(both[k][is_old], alone[k]), k
        assert torch.equal(both[k][~is_old], ko_alone[k][:n_ko]), k
        assert torch.equal(old_only[k], alone[k]), k


def test_sweeps_without_knockout_sites_add_no_launch():
    """The profiling counters of the same head-set sweep through tvr_patch_sweep_sets and through
    tvr_patch_sweep_knockout: equal launches of every kind; and the knockout sweep's own launches are one per
    layer with members."""
    r, model = _tiny4()
    cfg, prompts, vecs = r["cfg"], r["prompts"], r["vecs"].cuda()
    old, o_off, o_pat = _old_kind_sites(cfg, prompts)
    o_pat = np.asarray(o_pat, np.int32).reshape(-1, 3)

    def counted(fn, *a):
        trace = filled(model, prompts, False)
        model.profile(True)
        try:
            fn(trace, *a)
            torch.cuda.synchronize()
            return {k: v["launches"] for k, v in model.profile_hbm_stats().items()}
        finally:
            model.profile(False)

    a = counted(model.patch_sweep_sets, old, o_off, o_pat, vecs)
    b = counted(model.patch_sweep_knockout, old, o_off, o_pat, np.zeros(len(old) + 1, np.int32), np.zeros(0, np.int32),
                vecs)
    assert a == b, (a, b)
    # the knockout sweep's own launches: the same sites as last-position head-set sites (same members: the
    # same plan and rows) run the same attention launches, and the knockout adds one per layer with members
    k_sites, k_off, k_pat, k_koff, k_keys = ko_tables(r["cases"], prompts)
    c = counted(model.patch_sweep_knockout, k_sites, k_off, k_pat, k_koff, k_keys)
    h_sites, h_pat = k_sites.copy(), k_pat.copy()
    h_sites["kind"] = L.SITE_REPLACE_HEADSET_LASTPOS
    h_pat[:, 2] = 0
    h = counted(model.patch_sweep_sets, h_sites, k_off, h_pat, vecs)
    layers = {l for _, members, _ in r["cases"] for l, _ in members}
    assert c["attention"] == h["attention"] + len(layers), (c, h, layers)
    assert c["entry"] + len(layers) == h["entry"], (c, h)  # (the head-set patch launches are entry-kind spans)


# ------------------------------------------------------------------------------ 7: a linearised entry layer
@pytest.mark.parametrize("gemm", ["x2f16", "bf16"])
def test_linearised_entry_layer_with_knockout_members(gemm):
    """A fused sweep whose layer 1 is a linearised entry layer (only REPLACE_HEAD sites of layer 0 enter
    there) while knockout sites that entered at layer 0 have members at layer 1: the linearised block, then
    the knockout, then the O + MLP-out GEMM."""
    r, model = _tiny4(gemm)
    cfg, prompts, vecs, o32 = r["cfg"], r["prompts"], r["vecs"], r["o32"]
    H = cfg.n_heads
    from test_gpu_head_sets import hooked
    members = [(0, 2), (1, 2), (1, 0)]
    rows, want = [], []
    for i, p in enumerate(prompts):
        h = i % H
        rows.append((dict(seq=i, kind=1, layer=0, head=h, vec=h), [], []))  # enters at layer 1
        want.append(hooked(o32, p, [(0, h)], "all", vecs))
        blocked = list(range(0, len(p) - 1))
        rows.append((dict(seq=i, kind=KO), members, blocked))
        want.append(K.knocked_logits(o32, p, members, blocked))
    sites = tvr_amd.make_sites(len(rows))
    off, pat, koff, keys = [0], [], [0], []
    for site, (fields, s, b) in zip(sites, rows):
        for k, v in fields.items():
            site[k] = v
        site["target"] = prompts[fields["seq"]][1]
        pat += [(l, hh, -1) for l, hh in s]
        keys += b
        off.append(len(pat))
        koff.append(len(keys))
    trace = filled(model, prompts, True)
    model.profile(True)
    try:
        out = model.patch_sweep_knockout(trace, sites, off, np.asarray(pat, np.int32).reshape(-1, 3), koff, keys,
                                         vecs.cuda(), return_logits=True)
        torch.cuda.synchronize()
        hbm = model.profile_hbm_stats()
    finally:
        model.profile(False)
    assert hbm["lin_entry"]["launches"] >= 1, hbm["lin_entry"]
    tol = BF16_TOL if gemm == "bf16" else FP32_TOL
    errs = [rel_err(out["logits"][j], ref) for j, ref in enumerate(want)]
    print(f"lin entry + knockout {gemm}: worst logits {max(errs):.2e}")
    assert max(errs) < tol, errs


def test_bad_arguments_raise_value_error():
    r, model = _tiny4()
    prompts = r["prompts"]
    trace = filled(model, prompts, False)
    one = tvr_amd.make_sites(1)
    one["kind"] = KO
    T = len(prompts[0])
    ok = model.patch_sweep_knockout(trace, one, [0, 1], [(1, 0, -1)], [0, 1], [0])
    assert ok["prob"].shape == (1,)
    for args, msg in ((([0, 1], [(1, 0, -1)], [0, T], list(range(T))), "every key is blocked"),
                      (([0, 1], [(1, 0, -1)], [0, 2], [1, 1]), "strictly increasing"),
                      (([0, 1], [(1, 0, -1)], [0, 1], [T]), "blocked key outside"),
                      (([0, 1], [(9, 0, -1)], [0, 1], [0]), "member layer/head out of range"),
                      (([0, 2], [(1, 0, -1), (1, 0, -1)], [0, 1], [0]), "twice"),
                      (([0, 1], [(1, 0, -1)], [1, 0], [0]), "key_off"),
                      (([0, 1], [(1, 0, -1)], [0, 2], [0]), "key_off")):
        with pytest.raises(ValueError, match=msg):
            model.patch_sweep_knockout(trace, one, *args)
    with pytest.raises(ValueError, match="unknown kind"):
        model.patch_sweep_sets(trace, one, [0, 0], np.zeros((0, 3), np.int32))
    with pytest.raises(ValueError, match="unknown kind"):
        model.patch_sweep(trace, one)
    none = tvr_amd.make_sites(1)
    with pytest.raises(ValueError, match=r"only the knockout kind \(7\) owns keys"):
        model.patch_sweep_knockout(trace, none, [0, 0], np.zeros((0, 3), np.int32), [0, 1], [0])


# ------------------------------------------------------------------------------ 8: the façade
def _check_effect(got, ref, scale, tol, what):
    n = len(ref["p_clean"])
    d = ref["p_ko"] - ref["p_clean"][:, None]
    e = np.abs(got["dprob"].double().cpu().numpy() - d.mean(0)).max() / scale
    er = np.abs(got["rel_dprob"].double().cpu().numpy() - (d / ref["p_clean"][:, None]).mean(0)).max()
    rel_scale = scale / ref["p_clean"].min()
    print(f"{what}: dprob err {e:.2e} of the largest probability, rel_dprob err {er / rel_scale:.2e} (bar {tol:.0e})")
    assert e <= tol and er <= tol * rel_scale
    assert abs(got["clean_prob"] - ref["p_clean"].mean()) <= tol * scale
    # accuracy: the engine may differ from the reference only on the prompts the margin rule leaves out
    acc = got["accuracy"].double().cpu().numpy() * n
    lo = (ref["top_ko"] & ref["margin_ok"]).sum(0)
    hi = lo + (~ref["margin_ok"]).sum(0)
    assert ((lo - 1e-6 <= acc) & (acc <= hi + 1e-6)).all(), (acc, lo, hi)


def test_attention_knockout_effect_against_hooked_forwards():
    r, model = _tiny4()
    cfg, o64 = r["cfg"], r["o64"]
    prompts, answers, blocked, windows = K.facade_inputs(cfg, o64)
    scale = max(torch.softmax(o64(torch.tensor([p]))[0, -1], 0).max().item() for p in prompts)
    for heads in (None, [0, 2]):
        got = tvr_amd.attention_knockout_effect(prompts, [[a] for a in answers], blocked, windows, model=model,
                                                heads=heads)
        ref = K.oracle_effect(o64, prompts, answers, blocked, windows, heads)
        _check_effect(got, ref, scale, FP32_PROB_TOL, f"attention_knockout_effect heads={heads}")
    with pytest.raises(ValueError, match="every key"):
        tvr_amd.attention_knockout_effect(prompts[:1], answers[:1], [list(range(len(prompts[0])))], windows, model=model)


def test_attention_knockout_by_role_against_hooked_forwards():
    r, model = _tiny4()
    cfg, o64 = r["cfg"], r["o64"]
    contexts = list(tvr_amd.tasks.letter_to_caps)
    arrow = tvr_amd.tasks.ARROW
    random.seed(K.ROLE_SEED)
    prompts, roles, answers = tvr_amd.experiments.knockout_role_prompts(model, contexts, arrow, ",", K.ROLE_PROMPTS, 2)
    random.seed(K.ROLE_SEED)
    got = tvr_amd.attention_knockout_by_role(contexts, arrow, ",", model=model, num_contexts=K.ROLE_PROMPTS,
                                             len_contexts=2, roles=K.ROLE_NAMES, window=2, stride=2)
    assert got["roles"] == list(K.ROLE_NAMES) and got["windows"] == [(0, 1), (2, 3)]
    assert tuple(got["dprob"].shape) == (len(K.ROLE_NAMES), 2)
    scale = max(torch.softmax(o64(torch.tensor([p]))[0, -1], 0).max().item() for p in prompts)
    for x, name in enumerate(K.ROLE_NAMES):
        idx = tvr_amd.prompts.ROLES.index(name)
        blocked = [[j for j, c in enumerate(tr) if c == idx] for tr in roles]
        ref = K.oracle_effect(o64, prompts, answers, blocked, got["windows"], None)
        one = {k: (got[k][x] if k in ("dprob", "rel_dprob", "accuracy") else got[k]) for k in
               ("dprob", "rel_dprob", "accuracy", "clean_prob")}
        _check_effect(one, ref, scale, FP32_PROB_TOL, f"attention_knockout_by_role {name}")
