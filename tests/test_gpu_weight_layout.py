"""The row-pair-interleaved weight plane of the exact-fp16 GEMMs (csrc/w_layout.hpp, gemm_pingpong.hpp WIL):
the layout kernel, the kernel alone and the engine on it.

The interleaved plane holds the same values as the plain one and the kernel stages the same bytes to the same
LDS image, so every comparison here is bitwise (``torch.equal``): there is no tolerance.

* ``tvr_weight_rows_il`` against the numpy index formula, the zeroed partner row of an odd N included.
* ``tvr_gemm_launch`` with ``exact16 = 2`` against ``exact16 = 1`` on the same values: every output buffer whole
  (guard rows, pad columns and unnamed rows hold the same sentinels in both) and the range flag.  Both planes
  have row stride ldw = K + 32 with NaN in the columns [K, ldw), and the interleaved plane NaN in the partner row
  of an odd N (the engine's copy holds zeros there; the kernel must not use either).
  Shapes: M in {1, 255, 257, 513} x N in {2, 130, 254, 257, 514} x K in {32, 64, 96, 512}, each under the bias,
  GELU (n_split inside the range, raw_rows, mirror_rows) and residual epilogues, sliced and unsliced, plain and
  with gathered ``a_rows`` / scattered ``out_rows``, and a second A operand from column 256 where N reaches it.
  None of those N is a multiple of 4, which the forced split-K, split-tail and stream-K launches need (the
  vector epilogue): those forms run on N in {132, 516} at K = 512 (16 k-tiles: the smallest 2-way split) for
  every M, with the same epilogues, slicing, gather / scatter and second operand.
* the refusals of ``exact16 = 2``.
* the tiny exact-fp16 model of tests/test_gpu_exact16.py with the interleaved copies against one created under
  ``TVR_W_LAYOUT=rows`` in the same process: clean logits, probabilities and top-k, the REPLACE_HEAD CIE sweep
  over every site, an ADD_ATTN_OUT_LASTPOS sweep and ``forward_logits``.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import gemm_cases as G
import tvr_amd

pytestmark = [pytest.mark.gpu]

L = tvr_amd._lib
IL = G.IL
BIAS, GELU, RESID = G.EPI_BIAS, G.EPI_GELU, G.EPI_RESID
GUARD = 2
SENT32 = 0x7FC0BEEF
SENT16 = 0x7FFF
NAN16 = 0x7E00

MS, NS, KS = (1, 255, 257, 513), (2, 130, 254, 257, 514), (32, 64, 96, 512)
NS_VEC = (132, 516)


def weight_rows_il(w, ldw=None, pad_row=0):
    """numpy: one plane [N][K] (uint16) -> halves [ceil(N / 2)][ldw / 32][2][32]; columns [K, ldw) NaN, the
    partner row of an odd N ``pad_row``."""
    N, K = w.shape
    ldw = K if ldw is None else ldw
    P = (N + 1) // 2
    full = np.full((2 * P, ldw), NAN16, np.uint16)
    full[N:, :K] = pad_row
    full[:N, :K] = w
    return np.ascontiguousarray(full.reshape(P, 2, ldw // 32, 32).transpose(0, 2, 1, 3)).reshape(-1)


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


class Ctx:
    def __init__(self):
        cfg = tvr_amd.config.PythiaConfig(1, 64, 4, 32, 64, n_ctx=32, name="w-layout")
        w = tvr_amd.weights.synth_engine_weights(cfg, seed=1, device="cuda")
        self.model = tvr_amd.Model(cfg, w, tokenizer=tvr_amd.tokenizer.SyntheticTokenizer(512), device="cuda", gemm="f32")
        self.lib, self.h = self.model._lib, self.model._h

    def stream(self):
        return self.model._stream()


@functools.lru_cache(maxsize=None)
def _ctx():
    return Ctx()


@pytest.fixture(scope="module")
def ctx():
    yield _ctx()
    _ctx.cache_clear()
    _ops.cache_clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ the layout kernel
@pytest.mark.parametrize("N", [2, 7, 256, 258])
@pytest.mark.parametrize("K", [32, 96])
def test_weight_rows_il_is_the_index_formula(ctx, N, K):
    rng = np.random.default_rng([N, K])
    w = rng.integers(1, 0x7BFF, size=(N, K)).astype(np.uint16)
    want = weight_rows_il(w)  # the partner row of an odd N: zeros
    # by the formula of include/tvr.h, element by element
    n, k = np.arange(N)[:, None], np.arange(K)[None, :]
    assert np.array_equal(want[(n // 2) * 2 * K + (k // 32) * 64 + (n % 2) * 32 + k % 32], w)
    out = torch.full((want.size + 64,), SENT16, dtype=torch.int16, device="cuda")
    assert ctx.lib.tvr_weight_rows_il(dev16(w).data_ptr(), out.data_ptr(), N, K, ctx.stream()) == L.TVR_OK
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    assert np.array_equal(got[:want.size], want)
    assert (got[want.size:] == SENT16).all()  # nothing past ceil(N / 2) pairs
    if N % 2:
        assert (want.reshape(-1, K // 32, 2, 32)[-1, :, 1] == 0).all()


def test_weight_rows_il_refusals(ctx):
    buf = torch.zeros(4096, dtype=torch.int16, device="cuda")
    for w, out, N, K in ((0, buf.data_ptr(), 2, 32), (buf.data_ptr(), 0, 2, 32), (buf.data_ptr(), buf.data_ptr(), 0, 32),
                         (buf.data_ptr(), buf.data_ptr(), 2, 48), (buf.data_ptr(), buf.data_ptr(), 2, 0)):
        assert ctx.lib.tvr_weight_rows_il(w, out, N, K, ctx.stream()) == L.TVR_ERR_INVALID


# ------------------------------------------------------------------ the kernel alone
@functools.lru_cache(maxsize=None)
def _ops(M, N, K):
    """Device operands of one shape, shared by its launches: A and a second A [M + 3][2 lda] interleaved, the
    weight plane plain and row-pair interleaved (ldw = K + 32), bias, residual source values."""
    rng = np.random.default_rng([M, N, K])
    rows = M + 3  # (gathers read a few rows more)
    lda, ldw = K + 32, K + 32
    a = (rng.standard_normal((rows, K)) * 10.0 ** rng.uniform(-2.0, 1.0, size=K)[None, :]).astype(np.float32)
    a2 = rng.standard_normal((rows, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float16).view(np.uint16)
    plain = np.full((N, ldw), NAN16, np.uint16)
    plain[:, :K] = w
    return dict(A=dev16(G.act_buffer(G.split_act(a, G.X2F16), IL, lda)),
                A2=dev16(G.act_buffer(G.split_act(a2, G.X2F16), IL, lda)), lda=lda, ldw=ldw, rows=rows,
                W1=dev16(plain), W2=dev16(weight_rows_il(w, ldw, pad_row=NAN16)),
                bias=torch.from_numpy(rng.standard_normal(N).astype(np.float32)).cuda(),
                resid=rng.standard_normal((rows, N)).astype(np.float32))


def launch(ctx, M, N, K, exact16, epi, form=(L.FORM_PLAIN, 0, 0), slicing=L.SLICE_OFF, gather=False, a2=False,
           rc_want=L.TVR_OK, fmt=IL, W=None):
    """One tvr_gemm_launch on sentinel-filled outputs; returns every output buffer and the range flag."""
    o = _ops(M, N, K)
    vec = N % 4 == 0
    ld0 = N + 4 if vec else N + 1
    orows = M + 3 if gather else M
    a_rows = out_rows = None
    if gather:
        a_rows = [(5 * r + 1) % o["rows"] for r in range(M)]
        out_rows = [(r + 2) % orows for r in range(M)]
    outs = {"out0": torch.full((orows + GUARD, ld0), SENT32, dtype=torch.int32, device="cuda")}
    args = L.CGemmArgs(fmt=fmt, exact16=exact16, epi=epi, form=form[0], form_n=form[1], form_tile=form[2],
                       slicing=slicing, skinny=0, M=M, N=N, K=K, lda=o["lda"], ldw=o["ldw"], ld0=ld0,
                       a_buf_rows=o["rows"], out_buf_rows=orows if gather else 0, w_scale=1.0, wps=0,
                       A=o["A"].data_ptr(), W=(o["W2"] if exact16 == 2 else o["W1"]).data_ptr() if W is None else W,
                       bias=o["bias"].data_ptr(), out0=outs["out0"].data_ptr())
    keep = []
    if a2:
        args.a2, args.a2_col = o["A2"].data_ptr(), 256
    if gather:
        for name, rows in (("a_rows", a_rows), ("out_rows", out_rows)):
            arr = (ctypes.c_int32 * M)(*rows)
            setattr(args, name, ctypes.cast(arr, ctypes.c_void_p))
            keep.append(arr)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    if epi == RESID:
        ldr = N + 8 if vec else N + 2
        r = np.full((orows + GUARD, ldr), np.nan, np.float32)
        r[out_rows if gather else np.arange(M), :N] = o["resid"][:M]
        keep.append(torch.from_numpy(r).cuda())
        args.resid, args.ldr = keep[-1].data_ptr(), ldr
    if epi == GELU:
        n_split = (N // 2 // 8 * 8) if vec else N // 2  # inside the range: fp32 columns below it, GELU from it on
        ng = N - n_split
        ld1h = 64 * ((ng + 31) // 32)
        outs["out1h"] = torch.full((orows + GUARD, ld1h), SENT16, dtype=torch.int16, device="cuda")
        args.n_split, args.out1h, args.ld1h, args.ps1h, args.range_flag = n_split, outs["out1h"].data_ptr(), ld1h, 0, flag.data_ptr()
        if not gather:  # raw is addressed by launch row: not with out_rows
            ld_raw = (ng + 3) // 4 * 4 + 4 if vec else ng + 1
            outs["raw"] = torch.full((M + GUARD, ld_raw), SENT32, dtype=torch.int32, device="cuda")
            args.raw, args.raw_rows, args.ld_raw = outs["raw"].data_ptr(), (M + 1) // 2, ld_raw
    if epi != RESID:
        outs["out0m"] = torch.full((orows + GUARD, ld0), SENT32, dtype=torch.int32, device="cuda")
        args.out0m, args.mirror_rows = outs["out0m"].data_ptr(), (orows + 1) // 2
    rc = ctx.lib.tvr_gemm_launch(ctx.h, ctypes.byref(args), ctx.stream())
    assert rc == rc_want, (rc, ctx.lib.tvr_last_error())
    if rc != L.TVR_OK:
        return None
    torch.cuda.synchronize()
    outs["flag"] = flag
    return outs


def same(ctx, M, N, K, epi, what, **kw):
    """exact16 = 2 writes bit for bit what exact16 = 1 writes, and both wrote something."""
    a = launch(ctx, M, N, K, 1, epi, **kw)
    b = launch(ctx, M, N, K, 2, epi, **kw)
    assert a.keys() == b.keys()
    for name in a:
        assert torch.equal(a[name], b[name]), (what, name, M, N, K, epi, kw)
    written = a["out0"] != SENT32
    assert written.any(), (what, "nothing written")
    assert not torch.isnan(a["out0"].view(torch.float32)[written]).any(), (what, "a NaN of the pads was read")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_interleaved_plane_is_bitwise_the_plain_plane(ctx, M, N, K):
    for epi in (BIAS, GELU, RESID):
        for slicing in (L.SLICE_OFF, L.SLICE_ON):
            same(ctx, M, N, K, epi, "plain", slicing=slicing)
            same(ctx, M, N, K, epi, "gathered", slicing=slicing, gather=True)
            if N > 256:
                same(ctx, M, N, K, epi, "second operand", slicing=slicing, a2=True)
                same(ctx, M, N, K, epi, "second operand, gathered", slicing=slicing, a2=True, gather=True)
        same(ctx, M, N, K, epi, "the engine's plan", form=(L.FORM_PLAN, 0, 0), slicing=L.SLICE_MODEL)


@pytest.mark.parametrize("N", NS_VEC)
@pytest.mark.parametrize("M", MS)
def test_interleaved_plane_in_the_split_forms(ctx, M, N):
    K = 512
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    forms = {"plain": (L.FORM_PLAIN, 0, 0), "plan": (L.FORM_PLAN, 0, 0), "split-K": (L.FORM_SPLITK, 2, 0),
             "stream-K": (L.FORM_STREAMK, tiles + 1, 0), "stream-K, 2 k-tiles a block": (L.FORM_STREAMK, min(256, tiles * 8), 0)}
    if tiles > 1:
        forms["split tail"] = (L.FORM_TAIL, 2, tiles - 1)
        forms["stream-K tail"] = (L.FORM_STREAMK, 3, tiles - 1)
    for what, form in forms.items():
        for epi in (BIAS, GELU, RESID):
            for slicing in (L.SLICE_OFF, L.SLICE_ON):
                same(ctx, M, N, K, epi, what, form=form, slicing=slicing)
            same(ctx, M, N, K, epi, what + ", gathered", form=form, gather=True)
            if N > 256:
                same(ctx, M, N, K, epi, what + ", second operand", form=form, a2=True)


def test_exact16_2_refusals(ctx):
    M, N, K = 255, 130, 64
    o = _ops(M, N, K)
    launch(ctx, M, N, K, 2, BIAS, fmt=G.X2F16, rc_want=L.TVR_ERR_INVALID)  # planar A
    launch(ctx, M, N, K, 2, BIAS, fmt=G.BF16, rc_want=L.TVR_ERR_INVALID)
    launch(ctx, M, N, K, 2, BIAS, W=o["W2"].data_ptr() + 8, rc_want=L.TVR_ERR_INVALID)  # not 16-byte aligned
    launch(ctx, M, N, K, 3, BIAS, rc_want=L.TVR_ERR_INVALID)
    launch(ctx, M, N, K, 2, BIAS)  # and the same arguments are accepted


# ------------------------------------------------------------------ the engine
def _tiny(tiny_cfg, tokenizer, layout):
    sd = tvr_amd.weights.synth_hf_state_dict(tiny_cfg, seed=0, std=0.3, fp16=True)
    old = os.environ.get("TVR_W_LAYOUT")
    try:
        if layout is None:
            os.environ.pop("TVR_W_LAYOUT", None)
        else:
            os.environ["TVR_W_LAYOUT"] = layout
        return tvr_amd.Model.from_hf_state_dict(tiny_cfg, sd, device="cuda", tokenizer=tokenizer, gemm="x2f16")
    finally:
        if old is None:
            os.environ.pop("TVR_W_LAYOUT", None)
        else:
            os.environ["TVR_W_LAYOUT"] = old


def _engine_run(model, prompts, answers, mean, vecs):
    cfg = model.cfg
    out = {}
    clean = model.forward_clean(prompts, targets=answers, topk=5, return_logits=True)
    fused = model.forward_clean(prompts, targets=answers, topk=5)  # the fused-statistics unembed (the raw W_U)
    out.update(logits=clean["logits"], prob=clean["prob"], topk=clean["topk"], prob_fused=fused["prob"],
               topk_fused=fused["topk"])
    # REPLACE_HEAD at every (layer, head) of every prompt
    out["cie"] = tvr_amd.experiments.causal_indirect_effect_sums(mean, prompts, answers, model).clone()
    trace = model.trace(len(prompts), sum(len(p) for p in prompts))
    model.forward_clean(prompts, trace=trace)
    sites = tvr_amd.make_sites(len(prompts) * cfg.n_layers)
    for i in range(len(prompts)):
        for l in range(cfg.n_layers):
            s = sites[i * cfg.n_layers + l]
            s["seq"], s["kind"], s["layer"], s["vec"], s["target"] = i, L.SITE_ADD_ATTN_OUT_LASTPOS, l, (i + l) % len(vecs), answers[i]
    for fusedsweep in (False, True):
        sw = model.patch_sweep(trace, sites, vecs, topk=3, return_logits=not fusedsweep)
        for k, v in sw.items():
            out[f"add_attn_out{'_fused' if fusedsweep else ''}_{k}"] = v.clone()
    out["forward_logits"] = model.forward(prompts[1]).clone()
    return out


def test_engine_on_interleaved_weights_is_bitwise_the_plain_engine(tiny_cfg, tokenizer):
    rows = _tiny(tiny_cfg, tokenizer, "rows")
    il = _tiny(tiny_cfg, tokenizer, None)
    assert rows.exact16 and il.exact16 and (3 * tiny_cfg.d_model) % 256 != 0
    assert rows.weight_layout == 0
    assert il.weight_layout == L.W_IL_LAYERS | L.W_IL_UNEMBED
    g = torch.Generator().manual_seed(5)
    prompts = [[0] + torch.randint(1, tiny_cfg.d_vocab, (int(n),), generator=g).tolist() for n in (5, 9, 12)]
    answers = [int(x) for x in torch.randint(0, tiny_cfg.d_vocab, (3,), generator=g)]
    mean = torch.randn(tiny_cfg.n_layers, tiny_cfg.n_heads, tiny_cfg.d_model, generator=g).cuda() * 0.3
    vecs = (torch.randn(4, tiny_cfg.d_model, generator=g) * 0.5).cuda()
    a = _engine_run(rows, prompts, answers, mean, vecs)
    b = _engine_run(il, prompts, answers, mean, vecs)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # the copies follow the path: gone off the exact-fp16 path and in another GEMM mode, back with it
    il.set_exact16(False)
    assert il.weight_layout == 0
    il.set_exact16(True)
    assert il.weight_layout == L.W_IL_LAYERS | L.W_IL_UNEMBED
    il.set_gemm("f32")
    assert il.weight_layout == 0
    il.set_gemm("x2f16")
    assert il.weight_layout == L.W_IL_LAYERS | L.W_IL_UNEMBED
    c = _engine_run(il, prompts, answers, mean, vecs)
    for k in a:
        assert torch.equal(a[k], c[k]), ("after a rebind", k)
