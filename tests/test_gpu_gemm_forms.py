"""``gemm_pingpong_kernel``, its launch forms (``launch_pp``, ``launch_pp_partial``
for split-K and stream-K, the two reduce kernels; the kernels picked by
``pp_kernel`` / ``pp_reduce_kernel``) and ``gemm_skinny_kernel`` alone,
through ``tvr_gemm_launch``, against the fp64 reference of tests/gemm_cases.py.

The primitive runs ``launch_gemm`` itself on one tiny model (its weights are
never used): the engine's own plan, or a forced plain / split-K / split-tail /
stream-K launch, with the sliced accumulation on or off.  Variants: ``x2`` two
x2f16 weight planes, ``x2w1`` one exact fp16 plane, ``il1`` the same with A in
the k-tile-interleaved layout, ``il2`` that layout on two planes (plain bias
launch only) and ``bf16``.

Every launch (``launch``) checks what must NOT be written, bit for bit: two
guard rows after every output buffer, the columns [N, ld) of every row, the
rows ``out_rows`` does not name, the fp32 columns from n_split on under the
GELU epilogue, raw rows from raw_rows on, mirror rows from mirror_rows on, the
bf16 GELU buffer's unused plane; that out0m equals out0 where it is due; that
no output holds a NaN; and that the x2f16 range flag is raised exactly when a
GELU value reaches the format's limit.  The inputs carry NaN in the columns
[K, lda) of A and [K, ldw) of W, in the gather source's rows that ``a_rows``
does not name, and in the residual's rows that ``out_rows`` does not name.

Bars: integer and one-hot cases are bit-exact in every form.  Graded cases are
judged per element by gemm_cases.Case.bar (4 x the worse of two fp32
restatements, floored at one fp32 ulp of the result); GELU planes by
gemm_cases.gelu_bar against erf-GELU in fp64 of the device's own raw row.

Bit equalities asserted (each read from the source first):
  * interleaved = planar layout: the same fragments, products and k order
    (pp_tile_wt AIL: "same bytes, piece counts, fragments, k order");
  * gather / scatter = the same launch's rows without them: a_rows / out_rows
    change addresses only (pp_tile src[], pp_epilogue_lds orow[]); plain and
    split-K.  Not under stream-K, where a tile's k range is cut at the block
    boundaries that fall in it: a row gathered into another row tile is summed
    in other pieces (bar; the first version of this test asserted it bitwise
    and failed by 1-3 ulp on exactly those launches);
  * the head tiles of a split-tail or stream-K launch = the plain launch's same
    tiles (launch_pp over a tile window: the same kernel per tile).  A window
    of its own is not reachable through launch_gemm, so "two windows = the
    whole launch" is asserted in this form;
  * row r of a launch = the same row with every other row changed: an output
    element is a sum over its own A row and W column only;
  * out0m = out0 (the same register stored twice);
  * one plane = two planes on weights whose residual plane is zero, UNSLICED
    only: the a0 w1 product adds +0 to the running sum.  Sliced, the two forms
    add the same numbers as well (t = a1 w0 + 0 + a0 w0), asserted too;
  * skinny at M = 17 = the pingpong launch (SK_USE_M = 16: the opt-in is
    ignored).  At M <= 16 the skinny kernel sums four k-ranges in another
    order (and its epilogue may fuse the scale and the bias): judged by the
    bar, not bitwise.
Split-K, stream-K and the sliced form add in other orders than the plain launch:
bar, not bitwise.

Measured on an MI355X by this file (printed at its end), worst err / bar over
every graded case of a form, x2 / x2w1 = il1 / bf16 (il2 plain 0.37):
  plain 0.50 / 0.60 / 0.46 (gathered rows 0.56 / 0.67 / 0.47), sliced 0.17 / 0.21;
  element-wise epilogue 0.24 / 0.23 / 0.24;
  split-K 0.35 / 0.30 / 0.32 (gathered 0.41 / 0.29 / 0.49), sliced 0.15 / 0.20;
  split tail 0.43 / 0.60 / 0.40, sliced 0.17 / 0.20;
  stream-K 0.50 / 0.46 / 0.39 (gathered 0.56 / 0.41 / 0.58), sliced 0.17 / 0.23;
  the engine's own split plan 0.48 / 0.21 / 0.38; skinny 0.48 (x2), 0.33 (bf16);
  K = 16384 sliced (the model's rule) 0.18 / 0.25, forced unsliced 0.49 / 0.43;
  GELU planes 0.79 (every x2f16 variant), 0.996 (bf16: the bar's main term is
  bf16's own rounding, 2^-8 |g|, which a value just above a power of two uses up).
Every integer and one-hot case in every form is bit-exact and every sentinel
intact.  The whole file (104 tests) runs in about 9 s.

The tests bite: four mutants of gemm_pingpong.hpp that change arithmetic only
(not committed), each built and run once against this file (failing tests of 104):
  * splitk_reduce_kernel starting at partial 1: 51 — forced forms split2 / split3 /
    split16 / tail1 / tail3 (20), the engine's split and split-tail plans (6),
    gather / scatter, range flag, raw / mirror rows, row independence, second
    operand (4, 3, 4, 4, 4: their split-K launches), skinny (2: the M = 17 and
    planned launches), K 16384 under the plan (3), workspace poison (1);
  * splitk_sk_reduce_kernel skipping a block's second segment: 40 — forced forms
    sk5 / sk9 / sk7from1 / sk256 (16; sk4 passes, as it must: 4 blocks on 4
    tiles, no second segment), the stream-K plans (4), and the stream-K launches
    of the epilogue / row tests above (gather / scatter 4, range flag 3, raw /
    mirror rows 4, row independence 4, second operand 4, workspace poison 1);
  * the tile's a2_col comparison made strict: 4 — test_second_operand_by_column,
    every variant (a2_col at 256 and at the last tile);
  * the sliced form's carried final add dropped (pp_tile and pp_tile_wt): 31 —
    every forced form sliced (30) and the sliced layout / plane-count equality (1).
    The K = 16384, M = 1 launches do not see it: one row runs the K loop's
    partial-tile copy, which has no carried add.
"""
import collections
import ctypes
import functools
import gc
import time

import numpy as np
import pytest
import torch

import gemm_cases as G
import tvr_amd

pytestmark = [pytest.mark.gpu]

L = tvr_amd._lib
X2F16, IL, BF16 = G.X2F16, G.IL, G.BF16
BIAS, GELU, RESID = G.EPI_BIAS, G.EPI_GELU, G.EPI_RESID
PLAN, PLAIN, SPLITK, TAIL, STREAMK = L.FORM_PLAN, L.FORM_PLAIN, L.FORM_SPLITK, L.FORM_TAIL, L.FORM_STREAMK
VARIANTS = {"x2": (X2F16, 0), "x2w1": (X2F16, 1), "il1": (IL, 1), "il2": (IL, 0), "bf16": (BF16, 0)}
FULL = ("x2", "x2w1", "il1", "bf16")   # every epilogue and form
EPIS = (BIAS, GELU, RESID)
GUARD = 2
SENT32 = 0x7FC0BEEF  # int32 view of a NaN with a payload no kernel produces
SENT16 = 0x7FFF

_worst = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _module():
    t0 = time.time()
    yield
    for form, r in sorted(_worst.items()):
        print(f"\ngemm forms, worst err / bar: {form:34s} {r:.3f}", end="")
    print(f"\ngemm form tests: {time.time() - t0:.1f} s from the first test to the last")
    for cache in (_case, _ctx):
        cache.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


class Ctx:
    def __init__(self):
        cfg = tvr_amd.config.PythiaConfig(1, 64, 4, 32, 64, n_ctx=32, name="gemm-forms")
        w = tvr_amd.weights.synth_engine_weights(cfg, seed=1, device="cuda")
        self.model = tvr_amd.Model(cfg, w, tokenizer=tvr_amd.tokenizer.SyntheticTokenizer(512), device="cuda", gemm="f32")
        self.lib, self.h = self.model._lib, self.model._h

    def stream(self):
        return self.model._stream()


@functools.lru_cache(maxsize=None)
def _ctx():
    return Ctx()


@pytest.fixture()
def ctx():
    return _ctx()


@functools.lru_cache(maxsize=None)
def _case(kind, fam, M, N, K, one=False, zero_w_rows=()):
    return G.Case(kind, fam, M, N, K, one_plane=one, seed=3, zero_w_rows=zero_w_rows)


def case_for(kind, v, M, N, K):
    fmt, x16 = VARIANTS[v]
    return _case(kind, BF16 if fmt == BF16 else X2F16, M, N, K, bool(x16) and kind != "int")


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def operands(case, fmt, x16):
    """Device A [M][2 lda] and W [planes][N][ldw] (padded, NaN in the pad), once per case and layout."""
    if not hasattr(case, "dev"):
        case.dev = {}
    key = (fmt, x16)
    if key not in case.dev:
        K, N = case.K, case.N
        lda, ldw = K + 32, K + 8
        A = dev16(G.act_buffer(case.ap, fmt, lda))
        wp = case.wp[:1] if (x16 or fmt == BF16) else case.wp
        wps = N * ldw + 8
        W = np.full((wp.shape[0], wps), G.NAN16[fmt], np.uint16)
        W[:, :N * ldw].reshape(wp.shape[0], N, ldw)[:, :, :K] = wp
        case.dev[key] = (A, lda, dev16(W), ldw, wps)
    return case.dev[key]


def sentinel32(rows, ld):
    return torch.full((rows, ld), SENT32, dtype=torch.int32, device="cuda")


Out = collections.namedtuple("Out", "out0 raw gelu flag pre")


def launch(ctx, case, v, epi=BIAS, form=(PLAIN, 0, 0), slicing=L.SLICE_MODEL, n_split=None, raw_rows=None,
           mirror_rows=None, out_rows=None, out_buf_rows=None, a_rows=None, A=None, A_is_case=False, a2=None,
           a2_col=0, skinny=0, bias=None, pad=4, rc_want=L.TVR_OK):
    """One tvr_gemm_launch on sentinel-filled outputs.  A / a2: (device buffer, rows) to use instead of the
    case's own A (A_is_case: it holds the case's rows wherever a_rows reads); bias: an fp32 array instead of
    the case's.  Returns out0 [M][n_split or N] fp32 in launch
    row order, raw [raw_rows][N - n_split] or None, the decoded GELU planes [M][N - n_split] fp64 or None,
    the range flag, and pre = the fp64 pre-activation the outputs must equal (None if A was replaced)."""
    fmt, x16 = VARIANTS[v]
    N, K = case.N, case.K
    dA, lda, dW, ldw, wps = operands(case, fmt, x16)
    a_buf_rows = case.M
    if A is not None:
        dA, a_buf_rows = A
    M = len(a_rows) if a_rows is not None else case.M
    orows = out_buf_rows if out_rows is not None else M
    omap = np.asarray(out_rows) if out_rows is not None else np.arange(M)
    n_split = (N if epi != GELU else N // 2 // 8 * 8) if n_split is None else n_split
    nf, ng = (n_split, N - n_split) if epi == GELU else (N, 0)
    vec = N % 4 == 0
    ld0 = N + pad if vec else N + 1
    out0 = sentinel32(orows + GUARD, ld0)
    out0m = sentinel32(orows + GUARD, ld0) if mirror_rows is not None else None
    bias_h = case.bias if bias is None else np.asarray(bias, np.float32)
    d_bias = torch.from_numpy(bias_h).cuda()
    args = L.CGemmArgs(fmt=fmt, exact16=x16, epi=epi, form=form[0], form_n=form[1], form_tile=form[2], slicing=slicing,
                       skinny=skinny, M=M, N=N, K=K, lda=lda, ldw=ldw, ld0=ld0, n_split=n_split if epi == GELU else 0,
                       a2_col=a2_col, a_buf_rows=a_buf_rows, out_buf_rows=orows if out_rows is not None else 0,
                       w_scale=case.wscale, wps=wps, A=dA.data_ptr(), W=dW.data_ptr(), bias=d_bias.data_ptr(),
                       out0=out0.data_ptr())
    keep = [d_bias]
    if a2 is not None:
        args.a2 = a2[0].data_ptr()
    if a_rows is not None:
        arr = (ctypes.c_int32 * M)(*[int(r) for r in a_rows])
        args.a_rows = ctypes.cast(arr, ctypes.c_void_p)
        keep.append(arr)
    if out_rows is not None:
        arr = (ctypes.c_int32 * M)(*[int(r) for r in out_rows])
        args.out_rows = ctypes.cast(arr, ctypes.c_void_p)
        keep.append(arr)
    if out0m is not None:
        args.out0m, args.mirror_rows = out0m.data_ptr(), mirror_rows
    resid_h = None
    if epi == RESID:
        ldr = N + 2 * pad if vec else N + 2
        resid_h = case.resid[:M]
        r = np.full((orows + GUARD, ldr), np.nan, np.float32)
        r[omap, :N] = resid_h
        d_res = torch.from_numpy(r).cuda()
        args.resid, args.ldr = d_res.data_ptr(), ldr
        keep.append(d_res)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    out1h = raw = None
    if epi == GELU:
        if fmt == IL:
            ps1h, ld1h = 32, 64 * ((ng + 31) // 32)
        else:
            ps1h = (ng + 7) // 8 * 8 + 8 if vec else ng + 3
            ld1h = 2 * ps1h if vec else 2 * ps1h + 1
        out1h = torch.full((orows + GUARD, max(ld1h, 1)), SENT16, dtype=torch.int16, device="cuda")
        args.out1h, args.ld1h, args.ps1h, args.range_flag = out1h.data_ptr(), ld1h, 0 if fmt == IL else ps1h, flag.data_ptr()
        if raw_rows is not None:
            ld_raw = (ng + 3) // 4 * 4 + 4 if vec else ng + 1
            raw = sentinel32(M + GUARD, ld_raw)
            args.raw, args.raw_rows, args.ld_raw = raw.data_ptr(), raw_rows, ld_raw
    rc = ctx.lib.tvr_gemm_launch(ctx.h, ctypes.byref(args), ctx.stream())
    assert rc == rc_want, (rc, ctx.lib.tvr_last_error())
    if rc != L.TVR_OK:
        return None
    del keep
    named = np.zeros(orows + GUARD, bool)
    named[omap] = True
    o = out0.cpu().numpy()
    assert (o[~named] == SENT32).all(), "an output row nobody named was written"
    assert (o[:, nf:] == SENT32).all(), "columns past the fp32 columns were written"
    res = o[omap, :nf].view(np.float32)
    assert not np.isnan(res).any(), "NaN in out0"
    if out0m is not None:
        om = out0m.cpu().numpy()
        due = named & (np.arange(orows + GUARD) < mirror_rows)
        assert (om[~due] == SENT32).all() and (om[:, nf:] == SENT32).all(), "the mirror wrote past its rows"
        assert np.array_equal(om[due, :nf], o[due, :nf]), "out0m differs from out0"
    pre = None
    if (A is None or A_is_case) and a2 is None:
        pre = (case.ref if a_rows is None else case.ref[np.asarray(a_rows)]) + bias_h.astype(np.float64)[None, :]
        if epi == RESID:
            pre = pre + resid_h.astype(np.float64)
    rawv = gel = None
    want_flag = 0
    if epi == GELU:
        h = out1h.cpu().numpy().view(np.uint16)
        assert (h[~named] == SENT16).all(), "a GELU row nobody named was written"
        log = G.act_logical(h[:, :ld1h // 2 * 2], fmt, ld1h // 2) if fmt == IL else \
            np.stack([h[:, :ps1h], h[:, ps1h:2 * ps1h]])
        live = log[:, omap, :ng]
        if fmt == BF16:
            assert (log[1] == SENT16).all(), "the bf16 GELU buffer's second plane was written"
        assert (log[:, :, ng:] == SENT16).all(), "GELU columns past N - n_split were written"
        if fmt != IL:
            assert (h[:, 2 * ps1h:] == SENT16).all()
        gel = G.decode_act(live, fmt)
        if raw is not None:
            rw = raw.cpu().numpy()
            assert (rw[raw_rows:] == SENT32).all() and (rw[:, ng:] == SENT32).all(), "raw wrote past its rows"
            rawv = rw[:raw_rows, :ng].view(np.float32)
            assert not np.isnan(rawv).any(), "NaN in raw"
        if pre is not None and fmt != BF16:
            g32 = G.gelu_restate(pre[:, n_split:].astype(np.float32))
            want_flag = int((np.abs(g32) * np.float32(16.0) >= 65520.0).any())
            assert flag.item() == want_flag, "the x2f16 range flag"
    else:
        assert flag.item() == 0
    return Out(res, rawv, gel, flag.item(), pre)


def form_name(form, slicing=L.SLICE_MODEL):
    n = {PLAN: "plan", PLAIN: "plain", SPLITK: "split-K", TAIL: "split tail", STREAMK: "stream-K"}[form[0]]
    return n + (" sliced" if slicing == L.SLICE_ON else "")


def judge(case, v, epi, out, n_split, tag, two=None):
    """Exact cases bit for bit; graded ones per element against the bar; the GELU planes against gelu64 of
    the raw row (graded: the device's own; exact cases: the known integers)."""
    fmt, x16 = VARIANTS[v]
    nf = n_split if epi == GELU else case.N
    want = out.pre
    if case.kind in ("int", "onehot"):
        assert np.array_equal(out.out0.astype(np.float64), want[:, :nf]), f"{tag}: not bit-exact"
        if out.raw is not None:
            assert np.array_equal(out.raw.astype(np.float64), want[:out.raw.shape[0], nf:]), f"{tag}: raw not bit-exact"
    else:
        bar = case.bar(RESID if epi == RESID else BIAS, bool(x16) if two is None else two)[0]
        r = np.abs(out.out0.astype(np.float64) - want[:, :nf]) / bar[:, :nf]
        _worst[f"{v} {tag}"] = max(_worst[f"{v} {tag}"], float(r.max()) if r.size else 0.0)
        assert (r <= 1.0).all(), f"{tag}: worst err / bar {r.max():.3f}"
        if out.raw is not None:
            r = np.abs(out.raw.astype(np.float64) - want[:out.raw.shape[0], nf:]) / bar[:out.raw.shape[0], nf:]
            _worst[f"{v} {tag} raw"] = max(_worst[f"{v} {tag} raw"], float(r.max()) if r.size else 0.0)
            assert (r <= 1.0).all(), f"{tag}: raw, worst err / bar {r.max():.3f}"
    if epi == GELU and out.gelu.size:
        if case.kind == "graded":
            assert out.raw is not None and out.raw.shape[0] == out.gelu.shape[0]
            x = out.raw
        else:
            x = want[:, nf:].astype(np.float32)
        ok = np.abs(G.gelu_restate(x)) * np.float32(16.0) < 65520.0 if fmt != BF16 else np.ones(x.shape, bool)
        gbar, _ = G.gelu_bar(x, fmt)
        err = np.where(ok, np.abs(out.gelu - G.gelu64(x)), 0.0)
        r = np.divide(err, gbar, out=np.zeros_like(err), where=gbar > 0)
        _worst[f"{v} GELU planes"] = max(_worst[f"{v} GELU planes"], float(r.max()))
        assert (err <= gbar).all(), f"{tag}: GELU planes, worst err / bar {r.max():.3f}"


def run(ctx, kind, v, M, N, K, epi=BIAS, form=(PLAIN, 0, 0), slicing=L.SLICE_MODEL, n_split=None, tag=None, **kw):
    case = case_for(kind, v, M, N, K)
    ns = (N // 2 // 8 * 8) if n_split is None else n_split
    if epi == GELU and "raw_rows" not in kw:
        kw["raw_rows"] = M if "out_rows" not in kw else None
    if epi == GELU and kw.get("raw_rows") is None:
        kw.pop("raw_rows", None)
    out = launch(ctx, case, v, epi, form, slicing, n_split=ns if epi == GELU else None, **kw)
    if case.kind == "graded" and epi == GELU and out.raw is None:
        return out  # (graded GELU planes need the raw row: callers keep raw_rows = M)
    judge(case, v, epi, out, ns, tag or form_name(form, slicing))
    return out


# ------------------------------------------------------------------ the planes the kernel is given
def test_device_planes_are_the_host_emulation(ctx):
    """tvr_act_rows / tvr_weight_planes write the bits gemm_cases.split_act / split_w compute: the reference
    decodes what the kernel reads."""
    for fam, one in ((X2F16, False), (X2F16, True), (BF16, False)):
        c = _case("graded", fam, 300, 260, 512 if fam == X2F16 else 1024, one)
        a = torch.from_numpy(c.A).cuda()
        for fmt in ((X2F16, IL) if fam == X2F16 else (BF16,)):
            out = torch.zeros(c.M, 2 * c.K, dtype=torch.int16, device="cuda")
            L.check(ctx.lib.tvr_act_rows(fmt, a.data_ptr(), c.K, out.data_ptr(), c.M, c.K, None, ctx.stream()), "act_rows")
            torch.cuda.synchronize()
            want = G.act_buffer(c.ap, fmt, c.K, poison=False)
            got = out.cpu().numpy().view(np.uint16)
            if fmt == BF16:
                got, want = got[:, :c.K], want[:, :c.K]
            assert np.array_equal(got, want)
        w = torch.from_numpy(c.W).cuda()
        npl = 2 if fam == X2F16 else 1
        out = torch.zeros(npl, c.N * c.K, dtype=torch.int16, device="cuda")
        L.check(ctx.lib.tvr_weight_planes(fam, w.data_ptr(), c.wscale, out.data_ptr(), c.N * c.K, ctx.stream()), "planes")
        torch.cuda.synchronize()
        # (values, not bits: the device splits a weight of -0 into (+0, -0), numpy into (-0, +0))
        got = out.cpu().numpy().view(np.uint16).reshape(npl, c.N, c.K)
        assert np.array_equal(G.plane_values(got, fam), G.plane_values(c.wp, fam))


# ------------------------------------------------------------------ tile edges
EDGE_M = (1, 17, 129, 256, 257, 300, 513)
EDGE_N = (4, 256, 260, 516)


def edge_k(v):
    return (64, 128, 192) if v == "bf16" else (32, 64, 96, 160)


@pytest.mark.parametrize("v", list(VARIANTS))
def test_tile_edges_exact(ctx, v):
    """Every M x N x K of the edge sets, plain launch, the integer case: bit-exact, every epilogue in turn."""
    i = 0
    for M in EDGE_M:
        for N in EDGE_N:
            for K in edge_k(v):
                epi = BIAS if v == "il2" else EPIS[i % 3]
                i += 1
                run(ctx, "int", v, M, N, K, epi, mirror_rows=(M + 1) // 2 if epi != RESID else None)


@pytest.mark.parametrize("v", list(VARIANTS))
def test_tile_edges_onehot_and_graded(ctx, v):
    """One-hot rows pin the k addressing (every position of a 32- / 64-column group, every k-tile, both
    layouts and the swizzle); the graded case the arithmetic, at the largest K of the edge set."""
    K = edge_k(v)[-1]
    for M, N in ((300, 260), (513, 516), (129, 256)):
        run(ctx, "onehot", v, M, N, K, BIAS, bias=np.zeros(N, np.float32))
        for epi in ((BIAS,) if v == "il2" else EPIS):
            run(ctx, "graded", v, M, N, K, epi)


@pytest.mark.parametrize("v", FULL + ("il2",))
@pytest.mark.parametrize("N", (130, 257))
def test_elementwise_epilogue(ctx, v, N):
    """N not a multiple of 4: the element-wise (non-vector) epilogue with all three epilogues."""
    K = edge_k(v)[-2]
    for M in (17, 300):
        for epi in ((BIAS,) if v == "il2" else EPIS):
            ns = 64 if N == 130 else 129
            run(ctx, "int", v, M, N, K, epi, n_split=ns, mirror_rows=5 if epi != RESID else None, tag="element-wise")
            run(ctx, "graded", v, M, N, K, epi, n_split=ns, tag="element-wise")


@pytest.mark.parametrize("v", list(VARIANTS))
def test_wide_raster(ctx, v):
    """17 column tiles x 3 row tiles: group_m 4 with a last group of 3, and 51 tiles (not a multiple of 8)
    through the XCD remap."""
    M, N, K = 513, 4352, 64
    assert G.group_m(N) == 4 and (G.tile_grid(M, N)[0] * G.tile_grid(M, N)[1]) % 8 != 0
    for epi in ((BIAS,) if v == "il2" else (BIAS, RESID)):
        run(ctx, "int", v, M, N, K, epi)


# ------------------------------------------------------------------ forms
MF, NF = 300, 260   # 2 x 2 tiles


def forms_of(v):
    """(id, form, K in k-tiles) of every forced form on the 300 x 260 problem."""
    return [("split2", (SPLITK, 2, 0), 16), ("split3", (SPLITK, 3, 0), 24), ("split16", (SPLITK, 16, 0), 128),
            ("tail1", (TAIL, 2, 1), 16), ("tail3", (TAIL, 3, 3), 24),
            # stream-K over 4 tiles x 17 k-tiles = 68 iterations: 5 and 9 blocks do not divide them (blocks
            # straddle two tiles), 4 does (one segment each)
            ("sk4", (STREAMK, 4, 0), 17), ("sk5", (STREAMK, 5, 0), 17), ("sk9", (STREAMK, 9, 0), 17),
            # 256 blocks over 3 tiles x 128 = 384 iterations behind a plain head: every other block takes two
            # iterations, and block 85 takes the last of one tile and the first of the next.  (Over all 4 tiles
            # no block could straddle: block 64 t starts exactly at tile t.)
            ("sk256", (STREAMK, 256, 1), 128),
            # a plain head of one tile, then stream-K over 3 tiles x 17 = 51 iterations on 7 blocks
            ("sk7from1", (STREAMK, 7, 1), 17)]


FORM_IDS = [f[0] for f in forms_of("x2")]


@pytest.mark.parametrize("fid", FORM_IDS)
@pytest.mark.parametrize("v", FULL)
def test_forced_forms(ctx, v, fid):
    """Each form, both slicing choices, all three epilogues of the partial launch's reduce kernel: the integer
    case bit-exact, the graded case inside the bar; the head of a tail / stream-K launch bitwise the plain
    launch's tiles."""
    _, form, nkt = next(f for f in forms_of(v) if f[0] == fid)
    K = nkt * G.KTILE[VARIANTS[v][0]]
    for slicing in ((L.SLICE_OFF,) if v == "bf16" else (L.SLICE_OFF, L.SLICE_ON)):
        for epi in EPIS:
            for kind in ("int", "graded"):
                out = run(ctx, kind, v, MF, NF, K, epi, form, slicing, mirror_rows=150 if epi != RESID else None)
                if form[2] > 0 and kind == "graded":
                    plain = run(ctx, kind, v, MF, NF, K, epi, (PLAIN, 0, 0), slicing, tag="plain" + (
                        " sliced" if slicing == L.SLICE_ON else ""))
                    head = G.tile_mask(MF, NF, 0, form[2])[:, :out.out0.shape[1]]
                    assert np.array_equal(out.out0.view(np.int32)[head], plain.out0.view(np.int32)[head])
                    assert head.any()


def plan_of(ctx, M, N, K, v, epi):
    fmt, x16 = VARIANTS[v]
    out = (ctypes.c_int32 * 5)()
    flags = (1 if epi == GELU else 0) | (4 if x16 else 0)
    L.check(ctx.lib.tvr_gemm_plan(M, N, K, BF16 if fmt == BF16 else X2F16, flags, ctypes.cast(out, ctypes.c_void_p)), "plan")
    return list(out)


@pytest.mark.parametrize("v", FULL)
def test_engine_plan_split(ctx, v, monkeypatch):
    """The engine's own plan (plan_pp_cached as a block calls it) where it splits the whole launch."""
    monkeypatch.delenv("TVR_STREAM_K", raising=False)
    for M, N, K in ((300, 260, 1024), (257, 260, 1536), (17, 260, 4096)):
        for epi in (RESID, GELU):
            p = plan_of(ctx, M, N, K, v, epi)
            assert p[0] > 1 and p[1] == 0 and p[3] < 0, p  # the planner really splits: not a vacuous pass
            run(ctx, "int", v, M, N, K, epi, (PLAN, 0, 0), tag=f"plan split")
            run(ctx, "graded", v, M, N, K, epi, (PLAN, 0, 0), tag=f"plan split")


@pytest.mark.parametrize("v", ("x2", "il1"))
def test_engine_plan_tail_split(ctx, v, monkeypatch):
    """258 tiles: the planner runs 256 plain and splits the last two."""
    monkeypatch.delenv("TVR_STREAM_K", raising=False)
    M, N, K = 512, 33024, 512
    p = plan_of(ctx, M, N, K, v, RESID)
    assert p[0] == 1 and p[1] == 256 and p[2] >= 2, p
    run(ctx, "int", v, M, N, K, RESID, (PLAN, 0, 0), tag="plan split tail")


@pytest.mark.parametrize("v", FULL)
def test_engine_plan_stream_k(ctx, v, monkeypatch):
    """TVR_STREAM_K=1: 9 tiles x 128 (bf16: 120) k-tiles and 4 x 300 (280) on 256 blocks, which do not divide
    them."""
    monkeypatch.setenv("TVR_STREAM_K", "1")
    for M, N, K in (((513, 516, 7680), (300, 260, 17920)) if v == "bf16" else ((513, 516, 4096), (300, 260, 9600))):
        for epi in (RESID, GELU):
            p = plan_of(ctx, M, N, K, v, epi)
            assert p[3] == 0 and p[4] == 256, p
            tiles = G.tile_grid(M, N)[0] * G.tile_grid(M, N)[1]
            assert (tiles * (K // G.KTILE[VARIANTS[v][0]])) % 256 != 0
            run(ctx, "int", v, M, N, K, epi, (PLAN, 0, 0), tag="plan stream-K")


@pytest.mark.parametrize("v", ("x2", "x2w1", "il1"))
def test_true_sliced_shape(ctx, v):
    """K = 16384: the model's own rule slices the accumulation (launch_gemm: K >= PP_SLICE_MIN_K), plain and
    under the planner's split; against the same launch forced unsliced."""
    M, N, K = 1, 256, 16384
    for form in ((PLAIN, 0, 0), (PLAN, 0, 0)):
        for epi in (BIAS, RESID):
            run(ctx, "int", v, M, N, K, epi, form, tag="K 16384 model rule")
            a = run(ctx, "graded", v, M, N, K, epi, form, tag="K 16384 model rule")
            b = run(ctx, "graded", v, M, N, K, epi, form, L.SLICE_ON, tag="K 16384 sliced")
            run(ctx, "graded", v, M, N, K, epi, form, L.SLICE_OFF, tag="K 16384 unsliced")
            assert np.array_equal(a.out0.view(np.int32), b.out0.view(np.int32))  # the rule chose the sliced form


# ------------------------------------------------------------------ epilogue details
@pytest.mark.parametrize("v", FULL)
def test_gelu_split_raw_and_mirror_rows(ctx, v):
    """n_split inside a 256-column tile and on a tile boundary; raw_rows and mirror_rows at 0, inside a tile
    and at M; direct epilogue and both reduce kernels."""
    M, N = 300, 516
    K = 24 * G.KTILE[VARIANTS[v][0]]
    for form in ((PLAIN, 0, 0), (SPLITK, 3, 0), (STREAMK, 7, 0)):
        for ns in (136, 256):
            for rows in (0, 100, M):
                run(ctx, "int", v, M, N, K, GELU, form, n_split=ns, raw_rows=rows, mirror_rows=rows)
            run(ctx, "graded", v, M, N, K, GELU, form, n_split=ns, raw_rows=M, mirror_rows=M)


@pytest.mark.parametrize("v", FULL)
def test_gather_and_scatter(ctx, v):
    """out_rows as a permutation into a larger buffer, a_rows with repeats out of a source whose other rows
    are NaN.  Scatter and gather are bitwise the same form's launch without them (addresses only), in the
    plain and the split-K launch.  Under stream-K a gather that moves a row to another row tile is judged by
    the bar instead: each tile's k range is cut where the block boundaries g I / G fall in it, so the same
    row is summed in other pieces there (the integer case stays bit-exact)."""
    M, N = 300, 260
    K = 16 * G.KTILE[VARIANTS[v][0]]
    rng = np.random.default_rng(5)
    out_rows = rng.permutation(M + 37)[:M]
    a_rows = np.concatenate([rng.integers(0, 200, size=M - 40), np.full(40, 7)])  # rows 200 .. of the source: unused
    for kind in ("int", "graded"):
        case = case_for(kind, v, M, N, K)
        fmt = VARIANTS[v][0]
        src = G.act_buffer(case.ap[:, :200], fmt, K + 32, rows_total=M)  # rows [200, M): NaN
        src = (dev16(src), M)
        for form in ((PLAIN, 0, 0), (SPLITK, 2, 0), (STREAMK, 5, 0)):
            for epi in EPIS:
                plain = run(ctx, kind, v, M, N, K, epi, form, tag=form_name(form))
                sc = run(ctx, kind, v, M, N, K, epi, form, out_rows=out_rows, out_buf_rows=M + 37,
                         mirror_rows=150 if epi != RESID else None, tag=form_name(form) + " scatter")
                ga = run(ctx, kind, v, M, N, K, epi, form, a_rows=a_rows, A=src, A_is_case=True,
                         tag=form_name(form) + " gather")
                assert np.array_equal(sc.out0.view(np.int32), plain.out0.view(np.int32))
                same = run(ctx, kind, v, M, N, K, epi, form, a_rows=np.arange(M), tag=form_name(form))
                assert np.array_equal(same.out0.view(np.int32), plain.out0.view(np.int32))
                if epi == GELU:
                    assert np.array_equal(sc.gelu, plain.gelu) and np.array_equal(same.gelu, plain.gelu)
                    assert np.array_equal(same.raw.view(np.int32), plain.raw.view(np.int32))
                # (the residual belongs to the launch row, not the source row; stream-K: see the docstring)
                if epi != RESID and (kind == "int" or form[0] != STREAMK):
                    assert np.array_equal(ga.out0.view(np.int32), plain.out0.view(np.int32)[a_rows])
                    if epi == GELU:
                        assert np.array_equal(ga.gelu, plain.gelu[a_rows])
                        assert np.array_equal(ga.raw.view(np.int32), plain.raw.view(np.int32)[a_rows])


@pytest.mark.parametrize("v", ("x2", "x2w1", "il1", "bf16"))
def test_second_operand_by_column(ctx, v):
    """a2_col at 256 and at the last tile: tiles from a2_col on read a2 (here: A's rows reversed).  a2_col 0
    with A all NaN, and a2_col past N with a2 all NaN: the unused operand is never read."""
    M, N = 300, 516
    fmt = VARIANTS[v][0]
    K = 16 * G.KTILE[fmt]
    case = case_for("int", v, M, N, K)
    a2 = (dev16(G.act_buffer(case.ap[:, ::-1], fmt, K + 32)), M)
    nan = (dev16(np.full((M, 2 * (K + 32)), G.NAN16[fmt], np.uint16)), M)
    for form in ((PLAIN, 0, 0), (SPLITK, 2, 0), (STREAMK, 11, 0)):
        for epi in EPIS:
            ns = 256 if epi == GELU else None
            base = case.ref + case.bias[None, :] + (case.resid if epi == RESID else 0.0)
            for col in (256, 512):
                out = launch(ctx, case, v, epi, form, n_split=ns, a2=a2, a2_col=col, raw_rows=M if epi == GELU else None)
                want = base.copy()
                want[:, col:] = base[::-1][:, col:] if epi != RESID else (
                    case.ref[::-1] + case.bias[None, :] + case.resid)[:, col:]
                nf = out.out0.shape[1]
                assert np.array_equal(out.out0.astype(np.float64), want[:, :nf])
                if epi == GELU:
                    assert np.array_equal(out.raw.astype(np.float64), want[:, nf:])
            out = launch(ctx, case, v, epi, form, n_split=ns, A=nan, a2=a2, a2_col=0)
            rev = case.ref[::-1] + case.bias[None, :] + (case.resid if epi == RESID else 0.0)
            assert np.array_equal(out.out0.astype(np.float64), rev[:, :out.out0.shape[1]])
            out = launch(ctx, case, v, epi, form, n_split=ns, a2=nan, a2_col=768)
            assert np.array_equal(out.out0.astype(np.float64), base[:, :out.out0.shape[1]])


@pytest.mark.parametrize("v", ("x2", "x2w1", "il1"))
def test_gelu_range_flag(ctx, v):
    """One pre-activation at 4100 (16 x 4100 >= 65520: the flag rises) and then at 4000 (it does not), placed
    through the bias on a zero weight row (the whole column is then the bias), through the direct epilogue
    (its 8-column path in a whole GELU tile, its 4-column path in the partial last tile) and each reduce
    kernel.  Every other GELU column is pulled to -30000 by its bias: GELU = 0."""
    M, N, K = 300, 516, 24 * 32
    case = _case("int", X2F16, M, N, K, False, (300, 515))
    assert not case.ref[:, [300, 515]].any()
    for form in ((PLAIN, 0, 0), (SPLITK, 3, 0), (STREAMK, 7, 0)):
        for col in (300, 515):
            for x, want in ((4100.0, 1), (4000.0, 0)):
                bias = case.bias.copy()
                bias[256:] = -30000.0
                bias[col] = x
                out = launch(ctx, case, v, GELU, form, n_split=256, bias=bias, raw_rows=M)
                assert (out.raw[:, col - 256] == np.float32(x)).all() and out.flag == want
                judge(case, v, GELU, out, 256, "range flag")


@pytest.mark.parametrize("v", ("x2", "bf16"))
def test_skinny_kernel(ctx, v):
    """The skinny opt-in at M = 1, 15, 16 (gemm_skinny_kernel) and 17 (SK_USE_M = 16: the pingpong path,
    bitwise the launch without the opt-in)."""
    N = 260
    for K in ((64, 192, 4096) if v == "bf16" else (32, 160, 4096)):
        for M in (1, 15, 16, 17):
            run(ctx, "int", v, M, N, K, BIAS, (PLAN, 0, 0), skinny=1, tag="skinny")
            run(ctx, "onehot", v, M, N, K, BIAS, (PLAN, 0, 0), skinny=1, bias=np.zeros(N, np.float32), tag="skinny")
            a = run(ctx, "graded", v, M, N, K, BIAS, (PLAN, 0, 0), skinny=1, tag="skinny" if M <= 16 else "plan split")
            b = run(ctx, "graded", v, M, N, K, BIAS, (PLAN, 0, 0), skinny=0, tag="plan split")
            if M == 17:
                assert np.array_equal(a.out0.view(np.int32), b.out0.view(np.int32))
        rows = np.array([3, 3, 0, 14, 9])
        case = case_for("int", v, 16, N, K)
        out = launch(ctx, case, v, BIAS, (PLAN, 0, 0), skinny=1, a_rows=rows)
        assert np.array_equal(out.out0.astype(np.float64), out.pre)


# ------------------------------------------------------------------ bit equalities, poison
@pytest.mark.parametrize("slicing", (L.SLICE_OFF, L.SLICE_ON))
def test_layouts_and_plane_counts_agree_bitwise(ctx, slicing):
    """Graded fp16-valued weights (residual plane zero): interleaved = planar, and one plane = two planes, in the
    plain launch and under both reduce kernels; two planes: interleaved = planar (plain bias launch)."""
    M, N, K = 300, 260, 544
    one = _case("graded", X2F16, M, N, K, True)
    for form in ((PLAIN, 0, 0), (SPLITK, 2, 0), (STREAMK, 9, 0)):
        for epi in EPIS:
            ns = 128 if epi == GELU else None
            outs = {v: launch(ctx, one, v, epi, form, slicing, n_split=ns, raw_rows=M if epi == GELU else None)
                    for v in ("x2", "x2w1", "il1")}
            for v in ("x2w1", "il1"):
                assert np.array_equal(outs[v].out0.view(np.int32), outs["x2"].out0.view(np.int32)), (v, form, epi)
                if epi == GELU:
                    assert np.array_equal(outs[v].gelu, outs["x2"].gelu)
                    assert np.array_equal(outs[v].raw.view(np.int32), outs["x2"].raw.view(np.int32))
    two = _case("graded", X2F16, M, N, K, False)
    a, b = (launch(ctx, two, v, BIAS, (PLAIN, 0, 0), slicing) for v in ("x2", "il2"))
    assert np.array_equal(a.out0.view(np.int32), b.out0.view(np.int32))


@pytest.mark.parametrize("v", FULL)
def test_rows_are_independent_and_nan_stays_in_its_row(ctx, v):
    """Row r of a launch equals the same row with every other row changed (bitwise); a NaN in one used row of
    A reaches exactly that output row, in every form."""
    M, N = 300, 260
    fmt = VARIANTS[v][0]
    K = 16 * G.KTILE[fmt]
    case = case_for("graded", v, M, N, K)
    ident = np.arange(M)
    for form in ((PLAIN, 0, 0), (SPLITK, 2, 0), (STREAMK, 5, 0)):
        base = launch(ctx, case, v, BIAS, form, a_rows=ident)
        for r in (0, 127, 128, 256, 299):
            other = (ident[::-1] + 3) % M
            other[r] = r
            out = launch(ctx, case, v, BIAS, form, a_rows=other)
            assert np.array_equal(out.out0.view(np.int32)[r], base.out0.view(np.int32)[r])
    bad = 131
    buf = G.act_buffer(case.ap, fmt, K + 32)
    buf[bad, 5] = G.NAN16[fmt]  # one element of one used row (plane 0, first k-tile)
    src = dev16(buf)
    for form in ((PLAIN, 0, 0), (SPLITK, 2, 0), (STREAMK, 5, 0)):
        for epi in (BIAS, RESID):
            fmt_, x16 = VARIANTS[v]
            dA, lda, dW, ldw, wps = operands(case, fmt_, x16)
            out0 = torch.zeros(M, N, dtype=torch.float32, device="cuda")
            res = torch.from_numpy(case.resid).cuda()
            bias = torch.from_numpy(case.bias).cuda()
            args = L.CGemmArgs(fmt=fmt_, exact16=x16, epi=epi, form=form[0], form_n=form[1], form_tile=form[2],
                               slicing=L.SLICE_MODEL, M=M, N=N, K=K, lda=lda, ldw=ldw, ld0=N, ldr=N, w_scale=case.wscale,
                               wps=wps, A=src.data_ptr(), W=dW.data_ptr(), bias=bias.data_ptr(), out0=out0.data_ptr(),
                               resid=res.data_ptr() if epi == RESID else None)
            L.check(ctx.lib.tvr_gemm_launch(ctx.h, ctypes.byref(args), ctx.stream()), "gemm")
            nan = np.isnan(out0.cpu().numpy())
            assert nan[bad].all() and not np.delete(nan, bad, axis=0).any()


def test_workspace_poison_does_not_leak(ctx):
    """The split-K workspace only grows: a larger launch on NaN operands leaves NaN partials in every slot a
    later, smaller split-K / stream-K launch uses; that launch must overwrite every partial it reads."""
    M, N, K = 513, 516, 1024
    big = _case("int", X2F16, M, N, K)
    nan = (dev16(np.full((M, 2 * (K + 32)), G.NAN16[X2F16], np.uint16)), M)
    for poison in ((SPLITK, 4, 0), (STREAMK, 18, 0)):
        dA, lda, dW, ldw, wps = operands(big, X2F16, 0)
        out0 = torch.zeros(M, N, dtype=torch.float32, device="cuda")
        args = L.CGemmArgs(fmt=X2F16, epi=BIAS, form=poison[0], form_n=poison[1], M=M, N=N, K=K, lda=lda, ldw=ldw, ld0=N,
                           w_scale=big.wscale, wps=wps, A=nan[0].data_ptr(), W=dW.data_ptr(), out0=out0.data_ptr())
        L.check(ctx.lib.tvr_gemm_launch(ctx.h, ctypes.byref(args), ctx.stream()), "poison")
        assert np.isnan(out0.cpu().numpy()).all()  # every partial of the big launch is NaN
        for v in ("x2", "bf16"):
            kt = G.KTILE[VARIANTS[v][0]]
            for form, nkt in (((SPLITK, 2, 0), 16), ((SPLITK, 3, 0), 24), ((TAIL, 2, 3), 16), ((STREAMK, 5, 0), 17),
                              ((STREAMK, 9, 0), 17), ((STREAMK, 7, 1), 17)):
                for M2, N2 in ((300, 260), (17, 4)):
                    if form[0] != SPLITK and (M2, N2) == (17, 4):
                        continue
                    run(ctx, "int", v, M2, N2, nkt * kt, RESID, form)


def test_refusals_behind_a_real_model(ctx):
    """The checks of tests/test_gemm_cases.py hold with a real model too, and a refused launch writes nothing."""
    case = case_for("int", "x2", 300, 260, 512)
    assert launch(ctx, case, "x2", BIAS, (SPLITK, 3, 0), rc_want=L.TVR_ERR_INVALID) is None
    assert launch(ctx, case, "x2", BIAS, (STREAMK, 3, 0), rc_want=L.TVR_ERR_INVALID) is None
    assert launch(ctx, case, "il2", RESID, rc_want=L.TVR_ERR_INVALID) is None
    assert launch(ctx, case, "x2", BIAS, (TAIL, 2, 4), rc_want=L.TVR_ERR_INVALID) is None
    assert launch(ctx, case, "x2", BIAS, a_rows=[0] * 299 + [300], rc_want=L.TVR_ERR_INVALID) is None
