"""The normalisation kernels on the GPU, alone: ``lnpre_kernel<FMT, NV>`` (four
output formats x the row in 10 or 20 float4 per lane or three passes) through
``tvr_lnpre_rows`` — one launch_lnpre call with every option a block or the
unembed uses: gathered rows, the (mean, scale) side output, the copy of the
input rows, gamma-scaled x2f16 rows (one output or two), the range flag — and
``center_rows_kernel<V4>`` through ``tvr_center_rows`` (launch_center_rows, the
engine's own choice of the float4 or the element-wise form), against the fp64
reference, the exact prediction and the bars of tests/norm_cases.py.

Every output buffer is filled with the format's NaN and has guard rows on both
sides; x's padding columns [d, ldx) and the rows no row_idx names hold another
NaN.  A NaN in a result is a stray read; a changed guard, padding column
[d, ldy) or unwritten row is a stray store: whole buffers are compared, not the
written region alone.

Exact prediction: with the device's (mean, scale) read back, every output bit
is predicted on the host, o = fl32(fl32(x - mean) / scale), then the format's
conversion, the gammas (fl32(o g)) and the layout (norm_cases.expected).  (mean,
scale) themselves are graded against fp64 at the restatement bars, the decoded
outputs too (norm_cases.Bars, fmt_round).

Widths: 4, 64, 100, 252, 256, 260 (three passes; 256 one float4 per lane in
registers) in the full cross product of rows 1 / 3 / 4 / 5 / 9 (four waves per
block), ldx = ldy = d and d + 32 (all four stride pairs at 5 rows), eps 1e-5 /
1e-2; 768, 2560 (NV 10 full), 2816 (NV 20, one float4 into the second gamma
group), 5120 (NV 20 full), 5376 and 6144 (three passes) with 5 rows and one
stride and eps each; the interleaved format at the multiples of 32 of these and
32, 96, 288.

The exact output prediction held as specified on an MI355X: all 1,255
LayerNormPre launches of this file (fp32 302, x2f16 346, interleaved 305, bf16
302) returned the predicted buffers bit for bit, so fp32 division is correctly
rounded in this build and no one-ulp grading of o is used anywhere.

Measured there by this file (worst err / bar, printed at its end), on the
paths three passes / NV 10 / NV 20:
                        randn           offset          decades         spike           small
  mean                  .250 .190 .073  .250 .250 .250  .250 .141 .036  .250 .087 .250  .089 .029 .007
  scale                 .250 .259 .250  .250 .096 .170  .250 .250 .130  .250 .250 .250  .109 .109 .109
  y fp32                .250 .405 .250  .250 .250 .250  .250 .250 .179  .250 .250 .107  .250 .250 .250
  y x2f16 (2 layouts)   .306 .349 .295  .250 .250 .250  .279 .197 .267  .204 .187 .067  .667 .696 .667
  y g, x2f16            .279 .316 .296  .250 .250 .251  .291 .250 .258  .283 .164 .106  .718 .972 .993
  y bf16, plane 0       .994 .985 .995  .936 .919 .926  .992 .973 .980  .705 .701 .644  .995 .977 .995
  y bf16, fp16 plane    .975 .988 .978  .774 .708 .761  .954 .933 .962  .799 .732 .438  .038 .032 .037
  centring, both forms  .250            .250
0.250 = 1 / 4 means the device's value is the worse restatement's own, bit for
bit (the kernel-order restatement reproduces the device except where the
squares' multiply-adds are fused).  The bf16 rows are near 1 because the bar's
main term there is the format's unit roundoff, which a correct conversion
attains (with 2^-9 and 2^-12 in its place the worst ratios would be 1.99 and
1.98, for the correctly rounded host conversion as for the device: the planes
are bit-identical); ``small`` with gammas because |16 y g| just under half the
smallest fp16 subnormal rounds to zero, an error just under the bar's 2^-29.
The whole file (89 tests, 216 centring calls besides) takes 1.1 s from the
first test to the last.
"""
import collections
import ctypes
import functools
import gc
import time

import numpy as np
import pytest
import torch

import norm_cases as N
import tvr_amd
from tvr_amd import _lib as L

pytestmark = [pytest.mark.gpu]

G = N.GUARD
X2 = (N.X2F16, N.IL)
FMT_IDS = [N.FMT_NAME[f] for f in N.FMTS]
SMALL = set(N.D_SMALL) | {32, 96, 288}
EPS = (1e-5, 1e-2)

_worst = collections.defaultdict(float)
_count = collections.Counter()


def note(what, err, bar):
    """err <= bar for every element; the worst ratio is recorded for the table."""
    err, bar = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bar, np.float64))
    ok = err <= bar           # (False for a NaN)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err == 0, 0.0, np.inf))
    _worst[what] = max(_worst[what], float(np.nanmax(q)) if q.size else 0.0)
    return bool(ok.all())


@pytest.fixture(scope="module", autouse=True)
def _module():
    t0 = time.time()
    yield
    for what, r in sorted(_worst.items()):
        print(f"\nnorm, worst err / bar: {str(what):44s} {r:.3f}", end="")
    print(f"\nnorm launches: {dict(_count)}")
    print(f"norm tests: {time.time() - t0:.1f} s from the first test to the last")
    _ctx.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


class Ctx:
    """A tiny model: the owner of the range flag of the gamma-scaled launches."""

    def __init__(self):
        cfg = tvr_amd.config.PythiaConfig(2, 64, 4, 32, 64, n_ctx=32, name="norm")
        self.w = tvr_amd.weights.synth_engine_weights(cfg, seed=1, device="cuda", std=0.2)
        self.model = tvr_amd.Model(cfg, self.w, tokenizer=tvr_amd.tokenizer.SyntheticTokenizer(512), device="cuda",
                                   gemm="f32")
        self.h = self.model._h

    def range_status(self):
        return lib().tvr_model_range_status(self.h, stream())


@functools.lru_cache(maxsize=None)  # one model for the module: _module clears it
def _ctx():
    return Ctx()


def lib():
    return L.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    """A numpy array of 16- or 32-bit words on the device (as int16 / int32)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize])).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


class Bufs:
    """The device buffers of one launch: x, and NaN-filled guarded y / y2 / stats / copy."""

    def __init__(self, Ln, alloc_y2=None, alloc_copy=None):
        self.L = Ln
        self.x = dev(Ln.x_buffer())
        wide = Ln.fmt != N.F32
        self.ydt = np.uint16 if wide else np.uint32
        self.yfill = N.NAN16[Ln.fmt] if wide else N.NAN32
        self.yw = 2 * Ln.ldy if wide else Ln.ldy
        n = Ln.rows + 2 * G
        mk = lambda: dev(np.full((n, self.yw), self.yfill, dtype=self.ydt))
        self.y = mk()
        self.y2 = mk() if (Ln.g2 is not None if alloc_y2 is None else alloc_y2) else None
        self.stats = dev(np.full((n, 2), N.NAN32, dtype=np.uint32)) if Ln.stats else None
        self.copy = dev(np.full((n, Ln.ldx), N.NAN32, dtype=np.uint32)) if (Ln.copy_rows is not None if alloc_copy is None else alloc_copy) else None
        self.g1 = None if Ln.g1 is None else dev(np.asarray(Ln.g1, np.float32))
        self.g2 = None if Ln.g2 is None else dev(np.asarray(Ln.g2, np.float32))
        self.idx = None if Ln.idx is None else (ctypes.c_int32 * Ln.rows)(*Ln.idx.tolist())

    def body(self, t):
        """Pointer to the first row after the guard."""
        return 0 if t is None else t.data_ptr() + G * t.shape[1] * t.element_size()

    def args(self, **over):
        Ln = self.L
        a = L.CLnpreArgs(fmt=Ln.fmt, rows=Ln.rows, d=Ln.d, ldx=Ln.ldx, ldy=Ln.ldy, x_rows=Ln.x_rows,
                         copy_rows=Ln.copy_rows or 0, eps=Ln.eps, x=self.x.data_ptr(),
                         row_idx=None if self.idx is None else ctypes.cast(self.idx, ctypes.c_void_p),
                         y=self.body(self.y), stats=self.body(self.stats) or None, copy=self.body(self.copy) or None,
                         g1=None if self.g1 is None else self.g1.data_ptr(),
                         g2=None if self.g2 is None else self.g2.data_ptr(), y2=self.body(self.y2) or None)
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def read(self):
        out = {"y": host(self.y, self.ydt), "y2": None if self.y2 is None else host(self.y2, self.ydt),
               "copy": None if self.copy is None else host(self.copy, np.uint32), "stats": None}
        if self.stats is not None:
            s = host(self.stats, np.uint32)
            assert (s[:G] == N.NAN32).all() and (s[-G:] == N.NAN32).all(), "stats: a guard row was written"
            out["stats"] = s[G:-G].view(np.float32).copy()
        return out

    def untouched(self):
        r = self.read_raw()
        return all((v == fill).all() for v, fill in r)

    def read_raw(self):
        out = [(host(self.y, self.ydt), self.yfill)]
        if self.y2 is not None:
            out.append((host(self.y2, self.ydt), self.yfill))
        if self.stats is not None:
            out.append((host(self.stats, np.uint32), N.NAN32))
        if self.copy is not None:
            out.append((host(self.copy, np.uint32), N.NAN32))
        return out


def run(Ln, model=False):
    """One tvr_lnpre_rows call: the whole buffers read back."""
    b = Bufs(Ln)
    torch.cuda.synchronize()
    h = _ctx().h if (model or Ln.g1 is not None) else None
    rc = lib().tvr_lnpre_rows(h, ctypes.byref(b.args()), stream())
    L.check(rc, "tvr_lnpre_rows")
    _count[N.FMT_NAME[Ln.fmt]] += 1
    return b.read()


def same(got, want, what, skip_rows=()):
    """Whole buffers bit for bit (rows of ``skip_rows``, body numbering, are left to the caller)."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    ne = got != want
    for r in skip_rows:
        ne[G + r] = False
    if ne.any():
        rc = np.argwhere(ne)
        first = [(int(r) - G, int(c), hex(int(got[r, c])), hex(int(want[r, c]))) for r, c in rc[:6]]
        ulp = ""
        if got.dtype == np.uint32:
            dist = np.abs(got[ne].astype(np.int64) - want[ne].astype(np.int64))
            ulp = f"; bit distance max {dist.max()} counts {np.bincount(np.minimum(dist, 3))}"
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.size} words differ, first (row, word, got, want) {first}{ulp}")


def check(Ln, pool_idx, out, label):
    """Everything one launch with statistics must satisfy: the statistics against fp64 at their bars, every
    buffer against the exact prediction, the decoded outputs against fp64 at theirs."""
    d, eps, fmt, path = Ln.d, Ln.eps, Ln.fmt, N.path_of(Ln.d)
    st = out["stats"]
    assert not np.isnan(st).any(), f"{label}: NaN statistics (a stray read, or a row not written)"
    b = N.pool_bars(d, eps)
    mean, scale, y = (v[pool_idx] for v in b.ref[:3])
    for r, i in enumerate(pool_idx):
        fam = N.GRADED[i]
        assert note(("mean", path, fam), abs(float(st[r, 0]) - mean[r]), b.mean[i]), (label, r, fam, st[r, 0], mean[r])
        assert note(("scale", path, fam), abs(float(st[r, 1]) - scale[r]), b.scale[i]), (label, r, fam, st[r, 1], scale[r])
    want = N.expected(Ln, st)
    for k in ("y", "y2", "copy"):
        assert (out[k] is None) == (want[k] is None), (label, k)
        if want[k] is not None:
            same(out[k], want[k], f"{label} {k}")
    # the outputs against fp64
    g = {"y": Ln.g1, "y2": Ln.g2}
    for k in ("y", "y2"):
        if out[k] is None:
            continue
        gam = np.ones(d) if g[k] is None else np.asarray(g[k], np.float64)
        ref = y * gam[None, :]
        for plane in (0, 1) if fmt == N.BF16 else (0,):
            err = np.abs(N.decode(fmt, out[k], Ln.ldy, Ln.rows, d, plane) - ref)
            bar = b.y[pool_idx][:, None] * np.abs(gam)[None, :] + N.fmt_round(fmt, ref, plane)
            if g[k] is not None:
                bar = bar + N.EPS24 * np.abs(ref)
            for r, i in enumerate(pool_idx):
                what = f"y {N.FMT_NAME[fmt]}" + (" fp16 plane" if plane else "") + ("" if g[k] is None else " gamma")
                assert note((what, path, N.GRADED[i]), err[r], bar[r]), (label, k, plane, r)


def pool_launch(fmt, d, n, shift=0, **kw):
    i = (np.arange(n) + shift) % len(N.GRADED)
    return N.Launch(fmt, N.pool(d)[i], **kw), i


def widths(fmt):
    return N.D_IL if fmt == N.IL else N.D_ALL


ROW_CASES = [(f, d) for f in N.FMTS for d in widths(f)]


@pytest.mark.parametrize("fmt,d", ROW_CASES, ids=[f"{N.FMT_NAME[f]}-{d}" for f, d in ROW_CASES])
def test_rows_against_the_exact_prediction_and_fp64(fmt, d):
    """Statistics at their bars; every word of y against the prediction; the launch without the statistics
    byte-identical."""
    if d in SMALL:
        cases = [(n, ldx, ldy, eps) for n in N.ROWS for eps in EPS
                 for ldx, ldy in ([(d, d), (d + 32, d + 32), (d, d + 32), (d + 32, d)] if n == 5 else [(d, d), (d + 32, d + 32)])]
    else:
        k = widths(fmt).index(d)
        ld = d + 32 * (k % 2)
        cases = [(5, ld, ld, EPS[k % 2])]
    for k, (n, ldx, ldy, eps) in enumerate(cases):
        Ln, i = pool_launch(fmt, d, n, shift=k, ldx=ldx, ldy=ldy, eps=eps)
        label = f"{N.FMT_NAME[fmt]} d {d} rows {n} ldx {ldx} ldy {ldy} eps {eps}"
        out = run(Ln, model=fmt in X2)
        check(Ln, i, out, label)
        if eps == EPS[0] or d not in SMALL:
            Ln.stats = False
            plain = run(Ln)
            assert plain["stats"] is None
            same(plain["y"], out["y"], label + " without the statistics")
    if fmt in X2:  # without gammas the range flag never rises
        assert _ctx().range_status() == L.TVR_OK


GATHER_D = {N.F32: (100, 256, 2816), N.X2F16: (100, 256, 2816), N.IL: (96, 256, 2816), N.BF16: (100, 256, 5376)}


@pytest.mark.parametrize("fmt", N.FMTS, ids=FMT_IDS)
def test_gathered_rows_copy_and_statistics_by_output_row(fmt):
    """x holds 7 rows, the launch names 5: identity, a reversal, repeats.  copy[r] is x[row_idx[r]] for
    r < min(rows, copy_rows) and untouched beyond; stats[r] belongs to output row r."""
    for d in GATHER_D[fmt]:
        pool7 = (np.arange(7) + 1) % len(N.GRADED)
        x = N.pool(d)[pool7]
        for name, idx in (("identity", [0, 1, 2, 3, 4]), ("reversed", [6, 5, 4, 3, 2]), ("repeats", [6, 0, 0, 3, 0])):
            base = None
            for copy_rows in (0, 1, 4, 5, 8):
                Ln = N.Launch(fmt, x, idx=idx, ldx=d + 32, ldy=d, copy_rows=copy_rows)
                out = run(Ln)
                label = f"{N.FMT_NAME[fmt]} d {d} {name} copy_rows {copy_rows}"
                check(Ln, pool7[idx], out, label)
                if base is None:
                    base = out
                    Ln.copy_rows, Ln.stats = None, False
                    same(run(Ln)["y"], out["y"], label + " without copy and statistics")
                else:
                    same(out["y"], base["y"], label + " y against copy_rows 0")
                    assert (out["stats"].view(np.uint32) == base["stats"].view(np.uint32)).all()


GAMMA_D = {N.X2F16: (64, 100, 256, 768, 2560, 2816, 5120, 5376), N.IL: (64, 96, 256, 288, 2560, 2816, 5120, 6144)}


@pytest.mark.parametrize("fmt", X2, ids=[N.FMT_NAME[f] for f in X2])
@pytest.mark.parametrize("two", [False, True], ids=["g1", "g1-g2"])
def test_gamma_scaled_rows(fmt, two):
    """y = LNPre(x) g1 (the final LayerNorm's use) and y, y2 = LNPre(x) g1, LNPre(x) g2 with gammas that
    differ per column and from each other, every register and gamma group."""
    for k, d in enumerate(GAMMA_D[fmt]):
        g1, g2 = N.gammas(d)
        Ln, i = pool_launch(fmt, d, 5, shift=k, ldx=d, ldy=d + 32 * (k % 2), eps=EPS[k % 2], g1=g1, g2=g2 if two else None)
        out = run(Ln)
        check(Ln, i, out, f"{N.FMT_NAME[fmt]} d {d} gammas {'g1 g2' if two else 'g1'}")
    assert _ctx().range_status() == L.TVR_OK
    # the interleaved buffers are the planar ones permuted
    if fmt == N.IL:
        for d in (64, 2816):
            g1, g2 = N.gammas(d)
            a = run(pool_launch(N.X2F16, d, 5, g1=g1, g2=g2 if two else None)[0])
            b = run(pool_launch(N.IL, d, 5, g1=g1, g2=g2 if two else None)[0])
            for k in ("y", "y2") if two else ("y",):
                assert (N.act_logical(a[k], N.X2F16, d) == N.act_logical(b[k], N.IL, d)).all(), (d, k)
        assert _ctx().range_status() == L.TVR_OK


@pytest.mark.parametrize("fmt,d", [(N.X2F16, 256), (N.X2F16, 100), (N.IL, 2816), (N.IL, 5376)],
                         ids=["x2f16-256-nv10", "x2f16-100-3pass", "x2f16i-2816-nv20", "x2f16i-5376-3pass"])
@pytest.mark.parametrize("second", [False, True], ids=["through-g1", "through-g2"])
def test_range_flag(fmt, d, second):
    """The gammas are ones but one column, the column of a randn row's largest |y| (known from the
    reference), scaled to put max |y g| at 0.9 x 4095 — no flag — and at 1.1 x 4095 — TVR_ERR_RANGE, once."""
    ctx = _ctx()
    ctx.range_status()  # clear
    x = np.stack([N.pool(d)[0]] * 5)
    y = N.pool_bars(d, 1e-5).ref[2][0]
    c = int(np.abs(y).argmax())
    for factor, want in ((0.9, L.TVR_OK), (1.1, L.TVR_ERR_RANGE)):
        g = np.ones(d, np.float32)
        g[c] = factor * 4095.0 / abs(y[c])
        ones = np.ones(d, np.float32)
        Ln = N.Launch(fmt, x, g1=ones if second else g, g2=g if second else None, stats=False)
        run(Ln)
        assert ctx.range_status() == want, (factor, second)
        assert ctx.range_status() == L.TVR_OK  # reading clears it


@pytest.mark.parametrize("d", [4, 64, 256, 4096])
def test_const_rows_are_plus_zero_in_every_plane(d):
    x = np.stack([N.row("const", d, 0)] * 5)
    g1, g2 = N.gammas(d)
    for fmt in N.FMTS:
        if fmt == N.IL and d % 32:
            continue
        for eps in EPS:
            for a, b in [(None, None)] + ([(g1, None), (g1, g2)] if fmt in X2 else []):
                Ln = N.Launch(fmt, x, eps=eps, ldy=d + 32, g1=a, g2=b)
                out = run(Ln)
                st = out["stats"]
                assert (st[:, 0] == np.float32(1.5)).all() and (st[:, 1] == np.sqrt(np.float32(eps))).all(), (fmt, eps, st)
                want = N.expected(Ln, st)
                for k in ("y", "y2"):
                    if want[k] is not None:
                        same(out[k], want[k], f"const {N.FMT_NAME[fmt]} d {d} {k}")
                        body = out[k][G:-G]
                        used = body[:, :d] if fmt == N.F32 else N.act_logical(body, fmt, d + 32)[:, :, :d]
                        assert not used.any(), (fmt, k)


def plane_nan(fmt, buf, ldy, d):
    """[rows] bool per plane: every used word of the row is a NaN of its format."""
    body = buf[G:-G]
    if fmt == N.F32:
        return [np.isnan(body.view(np.float32)[:, :d]).all(-1)]
    p = np.ascontiguousarray(N.act_logical(np.ascontiguousarray(body), fmt, ldy)[:, :, :d])
    p0 = np.isnan(N.G.bf16_value(p[0])) if fmt == N.BF16 else np.isnan(p[0].view(np.float16))
    return [p0.all(-1), np.isnan(p[1].view(np.float16)).all(-1)]


@pytest.mark.parametrize("fmt", N.FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_nan_or_inf_row_stays_in_its_row(fmt, bad):
    """Six rows (two blocks), row 1 holds one NaN / Inf: that row is NaN throughout, every other word of the
    buffers is what the launch without it writes."""
    for d in (96 if fmt == N.IL else 100, 256, 2816):
        Ln, i = pool_launch(fmt, d, 6, ldy=d + 32)
        clean = run(Ln)
        x = Ln.x.copy()
        x[1, d // 3] = bad
        Lb = N.Launch(fmt, x, ldy=d + 32)
        out = run(Lb)
        assert np.isnan(out["stats"][1]).any() and (N.nan_rows(x) == [False, True] + [False] * 4).all()
        same(out["y"], clean["y"], f"{N.FMT_NAME[fmt]} d {d} beside the {bad} row", skip_rows=(1,))
        keep = np.ones(6, bool)
        keep[1] = False
        assert (out["stats"][keep].view(np.uint32) == clean["stats"][keep].view(np.uint32)).all()
        for p in plane_nan(fmt, out["y"], d + 32, d):
            assert p.tolist() == [False, True] + [False] * 4, (fmt, d, bad, p)
        row1 = out["y"][G + 1]
        pad = row1[d:] if fmt == N.F32 else N.act_logical(row1[None], fmt, d + 32)[:, 0, d:]
        assert (pad == (N.NAN32 if fmt == N.F32 else N.NAN16[fmt])).all(), "the NaN row's padding columns were written"


# ------------------------------------------------------------------------------ centring
def center_call(x, off, in_place):
    """tvr_center_rows on x [rows][d] at a view offset by ``off`` floats: (result rows, the source after)."""
    rows, d = x.shape
    n = (rows + 2 * G) * d

    def buf(fill_rows):
        flat = np.full(n + 8, N.XPAD32 if fill_rows is not None else N.NAN32, dtype=np.uint32)
        if fill_rows is not None:
            flat[off + G * d:off + (G + rows) * d] = fill_rows.reshape(-1).view(np.uint32)
        return dev(flat)

    src = buf(x)
    dst = src if in_place else buf(None)
    sp = src.data_ptr() + 4 * (off + G * d)
    dp = dst.data_ptr() + 4 * (off + G * d)
    torch.cuda.synchronize()
    L.check(lib().tvr_center_rows(sp, dp, rows, d, stream()), "tvr_center_rows")
    _count["center"] += 1
    got = host(dst, np.uint32)
    fill = N.XPAD32 if in_place else N.NAN32
    assert (got[:off + G * d] == fill).all() and (got[off + (G + rows) * d:] == fill).all(), "written outside the rows"
    if not in_place:
        s = host(src, np.uint32)
        assert (s[off + G * d:off + (G + rows) * d] == x.reshape(-1).view(np.uint32)).all(), "the source was changed"
    return got[off + G * d:off + (G + rows) * d].view(np.float32).reshape(rows, d).copy()


@pytest.mark.parametrize("d", N.CENTER_D)
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset-view"])
def test_center_rows(d, off):
    v4 = off == 0 and d % 4 == 0
    for rows in N.CENTER_ROWS:
        for fam in N.CENTER_FAMILIES:
            x = N.center_x(fam, d, rows)
            out = center_call(x, off, in_place=False)
            inp = center_call(x, off, in_place=True)
            assert (out.view(np.uint32) == inp.view(np.uint32)).all(), (d, off, rows, fam, "in place differs")
            assert not np.isnan(out).any(), (d, off, rows, fam)
            if fam == "const":
                assert not out.view(np.uint32).any(), (d, off, rows)  # exactly +0
                continue
            bar, _, _, ref = N.center_bars(x, v4)
            err = N.row_err(out, ref)
            assert note(("centre", "float4" if v4 else "element-wise", fam), err, bar), (d, off, rows, fam, err / bar)


def test_center_rows_refusals():
    t = dev(np.full(64, N.NAN32, dtype=np.uint32))
    p = t.data_ptr()
    for args, msg in (((0, p, 1, 4), b"null"), ((p, 0, 1, 4), b"null"), ((p, p, 0, 4), b"rows and d"),
                      ((p, p, 1, 0), b"rows and d"), ((p, p, -1, 4), b"rows and d"), ((p + 2, p, 1, 4), b"float aligned"),
                      ((p, p + 16, 2, 8), b"overlap"), ((p + 32, p, 4, 4), b"overlap")):
        assert lib().tvr_center_rows(*args, stream()) == L.TVR_ERR_INVALID, args
        assert msg in lib().tvr_last_error(), (args, lib().tvr_last_error())
    assert (host(t, np.uint32) == N.NAN32).all()


# ------------------------------------------------------------------------------ refusals
def test_lnpre_refusals_leave_the_outputs_untouched():
    """Every TVR_ERR_INVALID of tvr_lnpre_rows: refused on the host, so no kernel runs and every NaN-filled
    output stays as it was.  (Each call's buffers are valid and large enough for what it names.)"""
    h = _ctx().h
    d = 96
    g1, g2 = N.gammas(d)
    x = N.pool(d)

    def refused(f, msg, model=None, gam=(None, None), launch=None, alloc_y2=None, null_args=False, **over):
        kw = dict(ldx=d + 32, ldy=d + 32, copy_rows=2, g1=gam[0], g2=gam[1])
        kw.update(launch or {})
        b = Bufs(N.Launch(f, x, **kw), alloc_y2=alloc_y2)
        torch.cuda.synchronize()
        a = b.args()
        for k, v in over.items():
            setattr(a, k, v(a) if callable(v) else v)
        rc = lib().tvr_lnpre_rows(model, None if null_args else ctypes.byref(a), stream())
        err = lib().tvr_last_error()
        assert rc == L.TVR_ERR_INVALID and msg in err, (msg, rc, err)
        assert b.untouched(), msg

    F, X, I, B = N.F32, N.X2F16, N.IL, N.BF16
    refused(F, b"null args", null_args=True)
    refused(F, b"null x", x=None)
    refused(F, b"null y", y=None)
    refused(F, b"unknown fmt", fmt=1)
    refused(F, b"rows must be positive", rows=0)
    refused(F, b"rows must be positive", rows=-3)
    refused(F, b"multiples of 4", d=94)
    refused(F, b"multiples of 4", d=0)
    refused(F, b"multiples of 4", ldx=d + 2)
    refused(B, b"multiples of 4", ldy=d + 6)
    refused(F, b"at least d", ldx=d - 4)
    refused(X, b"at least d", ldy=d - 4)
    refused(I, b"multiples of 32", d=92)               # (ldy d + 32 = 128)
    refused(I, b"multiples of 32", ldy=d + 4)
    refused(I, b"multiples of 32", launch=dict(ldy=d + 36), d=d + 4)
    refused(F, b"16-byte aligned", x=lambda a: a.x + 4)
    refused(F, b"16-byte aligned", y=lambda a: a.y + 8)
    refused(F, b"16-byte aligned", copy=lambda a: a.copy + 4)
    refused(X, b"16-byte aligned", model=h, gam=(g1, g2), g1=lambda a: a.g1 + 4)
    refused(X, b"16-byte aligned", model=h, gam=(g1, g2), g2=lambda a: a.g2 + 8)
    refused(I, b"16-byte aligned", model=h, gam=(g1, g2), y2=lambda a: a.y2 + 2)
    refused(F, b"stats must be 8-byte aligned", stats=lambda a: a.stats + 4)
    refused(F, b"x_rows must be positive", x_rows=0)
    refused(F, b"exceeds x_rows", x_rows=4)
    past, neg = (ctypes.c_int32 * 4)(0, 1, 5, 2), (ctypes.c_int32 * 2)(-1, 1)
    refused(F, b"row_idx[2] outside", launch=dict(idx=[0, 1, 4, 2]), row_idx=ctypes.cast(past, ctypes.c_void_p))
    refused(F, b"row_idx[0] outside", launch=dict(idx=[0, 1]), row_idx=ctypes.cast(neg, ctypes.c_void_p))
    refused(F, b"row_idx[3] outside", launch=dict(idx=[0, 1, 2, 3]), x_rows=3)
    refused(F, b"copy_rows is negative", copy_rows=-1)
    refused(F, b"null copy", copy=None)
    refused(F, b"x2f16 formats only", model=h, gam=(g1, None))
    refused(B, b"x2f16 formats only", model=h, gam=(g1, None))
    refused(X, b"needs a model", gam=(g1, None))
    refused(X, b"y2 needs g1 and g2", model=h, alloc_y2=True)
    refused(I, b"y2 needs g1 and g2", model=h, gam=(g1, None), alloc_y2=True)
    refused(X, b"g2 needs y2", model=h, gam=(g1, g2), y2=None)
    # the same buffers are still fine for a good call afterwards
    Ln, i = pool_launch(N.IL, d, 5, ldx=d + 32, ldy=d + 32, g1=g1, g2=g2)
    check(Ln, i, run(Ln), "after the refusals")
    assert _ctx().range_status() == L.TVR_OK
