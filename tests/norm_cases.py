"""LayerNormPre and row-centring cases with known answers, their fp64 reference,
the exact prediction of every output bit and the bars (shared by
test_norm_cases.py and test_gpu_norm.py; a plain module, not a conftest).  Host
only, numpy.

The operation (csrc/kernels.hpp lnpre_kernel, one wave per row):

  mean = sum(x) / d,   scale = sqrt(sum((x - mean)^2) / d + eps),   y = (x - mean) / scale

optionally on gathered rows (``row_idx``), with a (mean, scale) side output, a
copy of the gathered input rows, and gamma-scaled x2f16 rows y g1 (and y g2).
``center_rows_kernel`` is the first line and x - mean alone.

Row families (``row(family, d, seed)``): ``randn`` 3 N(0, 1) + 1; ``offset``
1000 + N(0, 1) (a one-pass variance fails in fp32); ``decades`` column
magnitudes over 1e-6 .. 1e3; ``spike`` one element 1e4 among N(0, 1e-2) (the
output is close to sqrt(d)); ``small`` 1e-12 N(0, 1) (eps dominates; no
subnormal squares); ``const`` 1.5 everywhere (at power-of-two d the mean and the
centred values are exact: every output plane is +0 and scale = sqrt(eps)).
Every width has one row of each graded family (``pool``); a launch of n rows
takes them in turn (``take``), so few launches meet all of them, and the rows
the GPU file grades are the rows test_norm_cases.py judges.

``reference`` is fp64.  Two fp32 restatements of (mean, scale) stand for "a
correct fp32 implementation": ``stats_kernel_order`` follows the kernel (each
lane adds its float4s as (x + y) + (z + w), strided by 64, a 64-lane xor
butterfly, division by d, the second pass over the rounded x - mean; the device
may fuse the multiply-adds of the squares, which this does not), and
``stats_numpy`` is numpy's pairwise fp32 sum.

Bars, none taken from the engine, per row (``row_bars``):

  mean    max(4 x the worse restatement's error, 4 x 2^-24 x mean|x|)
  scale   max(4 x the worse restatement's error, 4 x 2^-24 x scale)
  y       max(4 x the worse restatement's largest error over the row's
          columns, 4 x 2^-24 x max(max|y|, |mean| / scale)): one rounding of the
          mean moves every output by |mean| / scale ulps of the mean
  + the format's own rounding per element (``fmt_round``): x2f16 2^-22 |y| +
  2^-29 (two fp16 roundings at unit roundoff 2^-11; half the fp16 subnormal
  spacing 2^-25 over the scale 16), bf16 plane 0 2^-8 |y| (8 significand bits),
  its fp16 plane 1 2^-11 |y| + 2^-25.  (Half of these two, 2^-9 and 2^-12, is
  what a correctly rounded conversion meets only on average: 1 + 2^-8 rounds
  to bf16 with an error of 2^-8, and test_norm_cases.py shows it.  The planes
  are pinned bit for bit by ``expected`` in any case.)  A gamma-scaled row's
  bar is the row's bar times |g| plus one more fp32 rounding 2^-24 |y g| (the
  single multiplication).

The margin 4 is the project's standing margin over a correct fp32 evaluation
in another order (attribution_cases.BAR_MARGIN).  test_norm_cases.py records
how often the floor sets a bar.

The outputs themselves are not graded at a bar where the device's (mean,
scale) are read back: ``expected`` predicts every bit of every buffer from
them, o = fl32(fl32(x - mean) / scale), then the format's conversion and layout
(a subtraction followed by a division, and a single multiplication, admit no
contraction; fp32 division is correctly rounded).  Its ``mutate`` argument
plants the addressing, layout and conversion mistakes that
test_norm_cases.py shows to be caught.
"""
from __future__ import annotations

import functools

import numpy as np

import gemm_cases as G
from attribution_cases import BAR_MARGIN, EPS24, FLOOR_ULPS
from gemm_cases import NAN16, act_logical, bf16_bits, split_act

F32, X2F16, IL, BF16 = 0, G.X2F16, G.IL, G.BF16   # include/tvr.h: 0, TVR_GEMM_X2F16, TVR_ACT_X2F16_IL, TVR_GEMM_BF16
FMTS = (F32, X2F16, IL, BF16)
FMT_NAME = {F32: "f32", X2F16: "x2f16", IL: "x2f16i", BF16: "bf16"}
GUARD = 2                    # guard rows before and after every output buffer
NAN32 = 0x7FC00000           # the fill of every fp32 output
XPAD32 = 0x7FC01234          # another NaN: x's padding columns and unnamed rows (a copied pad differs from the fill)
GRADED = ("randn", "offset", "decades", "spike", "small")
FAMILIES = GRADED + ("const",)
GAMMA_GROUP = 2560           # columns per gamma register group of the NV = 20 path (kernels.hpp LN_G_F4 * 256)

# the widths of the GPU file: the smallest reaching each path (engine.hip launch_lnpre)
D_SMALL = (4, 64, 100, 252, 256, 260)              # three passes but 256 (registers, one float4 per lane)
D_LARGE = (768, 2560, 2816, 5120, 5376, 6144)      # NV 10 (3 of 10, full), NV 20 (11 of 20, full), three passes
D_ALL = D_SMALL + D_LARGE
D_IL = tuple(sorted([d for d in D_ALL if d % 32 == 0] + [32, 96, 288]))
ROWS = (1, 3, 4, 5, 9)       # four waves per block: a partial block, a full one, one and five rows past it
CENTER_D = (4, 63, 64, 100, 257, 50304)
CENTER_ROWS = (1, 4, 5)
CENTER_FAMILIES = ("randn", "offset", "const")


def path_of(d):
    """The row path launch_lnpre picks."""
    return "3pass" if d % 256 != 0 or d > 5120 else "nv10" if d <= 2560 else "nv20"


# ------------------------------------------------------------------------------ rows
def row(family, d, seed):
    rng = np.random.default_rng([FAMILIES.index(family), d, seed])
    n = rng.standard_normal(d)
    if family == "randn":
        x = 3.0 * n + 1.0
    elif family == "offset":
        x = 1000.0 + n
    elif family == "decades":
        x = n * 10.0 ** rng.uniform(-6.0, 3.0, size=d)
    elif family == "spike":
        x = 1e-2 * n
        x[int(rng.integers(d))] = 1e4
    elif family == "small":
        x = 1e-12 * n
    elif family == "const":
        x = np.full(d, 1.5)
    else:
        raise ValueError(family)
    return x.astype(np.float32)


# The seed of each width's five graded rows.  test_norm_cases.py's condition is that the floor sets the output
# bar in at most a quarter of the graded (row, eps) pairs, so that the bars are mostly the restatements' and
# not the floor's.  With one seed for all widths it sets it in 56 of 120 (a correct fp32 evaluation is often
# within an ulp of the largest output), so each width takes the smallest seed in [0, 200) for which the floor
# sets at most 2 of its 10 output bars (3 at d = 32, the best there is): 28 of 150.  The bars of the mean and
# the scale are not under that condition: a fp32 sum in either order is usually within a fraction of an ulp of
# mean|x|, and the floor sets them in most rows whatever the seed (the counts are asserted all the same).
SEED = {4: 180, 32: 19, 64: 68, 96: 5, 100: 157, 252: 7, 256: 14, 260: 1, 288: 31, 768: 1, 2560: 2, 2816: 15,
        5120: 11, 5376: 5, 6144: 0}


@functools.lru_cache(maxsize=None)
def pool(d):
    """The width's graded rows, fp32 [5][d]: one of every family of GRADED, in that order."""
    x = np.stack([row(f, d, SEED.get(d, 0)) for f in GRADED])
    x.setflags(write=False)
    return x


def take(d, n, shift=0):
    """(x fp32 [n][d], the family of each row): the pool's rows in turn from ``shift`` (n > 5 repeats rows)."""
    i = (np.arange(n) + shift) % len(GRADED)
    return pool(d)[i], [GRADED[k] for k in i]


@functools.lru_cache(maxsize=None)
def pool_bars(d, eps):
    return Bars(pool(d), eps)


# ------------------------------------------------------------------------------ reference and restatements
def reference(x, eps, g1=None, g2=None):
    """fp64: (mean [n], scale [n], y [n][d], y g1 or None, y g2 or None)."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(-1)
    c = x - mean[:, None]
    scale = np.sqrt((c * c).mean(-1) + float(np.float32(eps)))
    y = c / scale[:, None]
    return (mean, scale, y, None if g1 is None else y * np.asarray(g1, np.float64)[None, :],
            None if g2 is None else y * np.asarray(g2, np.float64)[None, :])


def lane_sum(t):
    """fp32 [n][m] -> [n]: lane l adds t[l], t[l + 64], .. in order (from 0.f), then the xor butterfly of
    split.hpp wave_sum (every lane ends with the same value)."""
    t = np.asarray(t, dtype=np.float32)
    n, m = t.shape
    U = -(-m // 64)
    p = np.zeros((n, U * 64), np.float32)
    p[:, :m] = t
    p = p.reshape(n, U, 64)
    s = np.zeros((n, 64), np.float32)
    for u in range(U):
        s = s + p[:, u]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    assert s.dtype == np.float32
    return s[:, 0]


def f4_sum(t):
    """fp32 [n][d] (d % 4 == 0) -> [n][d / 4]: (x + y) + (z + w) of every float4."""
    v = np.asarray(t, dtype=np.float32).reshape(t.shape[0], -1, 4)
    return (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])


def mean_kernel_order(x, v4=True):
    """The kernels' mean in fp32: float4 partial sums (lnpre_kernel, center_rows_kernel<true>) or single
    elements (center_rows_kernel<false>) per lane."""
    x = np.asarray(x, dtype=np.float32)
    return lane_sum(f4_sum(x) if v4 else x) / np.float32(x.shape[1])


def stats_kernel_order(x, eps):
    """Restatement (a): (mean, scale) fp32 [n] in lnpre_kernel's order."""
    x = np.asarray(x, dtype=np.float32)
    d = np.float32(x.shape[1])
    mean = mean_kernel_order(x)
    c = x - mean[:, None]
    scale = np.sqrt(lane_sum(f4_sum(c * c)) / d + np.float32(eps))
    assert mean.dtype == scale.dtype == np.float32
    return mean, scale


def stats_numpy(x, eps, mutate=None, ldx=None):
    """Restatement (b): numpy's fp32 sums.  ``mutate`` plants a mistake of the statistics."""
    x = np.asarray(x, dtype=np.float32)
    n, d = x.shape
    xs = x[:, :d - 4] if mutate == "drop_last_f4" else x
    mean = xs.sum(-1, dtype=np.float32) / np.float32(ldx if mutate == "mean_over_ldx" else d)
    if mutate == "one_pass":
        var = (xs * xs).sum(-1, dtype=np.float32) / np.float32(d) - mean * mean
    else:
        c = xs - mean[:, None]
        var = (c * c).sum(-1, dtype=np.float32) / np.float32(d - 1 if mutate == "d_minus_1" else d)
    if mutate == "eps_outside":
        with np.errstate(invalid="ignore"):
            scale = np.sqrt(var) + np.float32(eps)
    else:
        with np.errstate(invalid="ignore"):
            scale = np.sqrt(var + np.float32(eps))
    assert mean.dtype == scale.dtype == np.float32
    return mean, scale


STAT_MUTATIONS = ("one_pass", "eps_outside", "d_minus_1", "mean_over_ldx", "drop_last_f4")


def normalise(x, mean, scale):
    """o = fl32(fl32(x - mean) / scale): what the kernel stores (before the format's conversion)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        c = x - np.asarray(mean, np.float32)[:, None]
        o = c / np.asarray(scale, np.float32)[:, None]
    assert o.dtype == np.float32
    return o


def row_err(got, ref):
    """Largest |got - ref| of every row (inf where a NaN or Inf appears)."""
    with np.errstate(invalid="ignore"):
        e = np.abs(np.asarray(got, dtype=np.float64) - ref)
    e = np.where(np.isfinite(e), e, np.inf)
    return e.reshape(e.shape[0], -1).max(-1)


class Bars:
    """Per-row bars of x [n][d] (module docstring): ``mean``, ``scale``, ``y`` [n]; ``floored`` [n][3] bool
    (the floor set the bar); ``err`` [n][3][2] the two restatements' errors; ``ref`` the fp64 reference."""

    def __init__(self, x, eps):
        x = np.asarray(x, dtype=np.float32)
        self.ref = mean, scale, y, _, _ = reference(x, eps)
        errs = []
        for m32, s32 in (stats_kernel_order(x, eps), stats_numpy(x, eps)):
            errs.append([np.abs(m32.astype(np.float64) - mean), np.abs(s32.astype(np.float64) - scale),
                         row_err(normalise(x, m32, s32), y)])
        self.err = np.asarray(errs).transpose(2, 1, 0)                       # [n][quantity][restatement]
        floor = FLOOR_ULPS * EPS24 * np.stack([np.abs(x.astype(np.float64)).mean(-1), scale,
                                               np.maximum(np.abs(y).max(-1), np.abs(mean) / scale)], 1)
        raised = BAR_MARGIN * self.err.max(-1)
        self.floored = floor >= raised
        bar = np.maximum(raised, floor)
        self.mean, self.scale, self.y = bar[:, 0], bar[:, 1], bar[:, 2]


def fmt_round(fmt, y, plane=0):
    """The format's own rounding of a value y (fp64 reference), per element: round to nearest of a p-bit
    significand errs by at most the unit roundoff 2^-p |y| (reached at 1 + 2^-p: test_norm_cases.py), bf16
    p = 8, fp16 p = 11 and half its subnormal spacing 2^-25 below 2^-14; x2f16 is two fp16 roundings of 16 y."""
    y = np.abs(y)
    if fmt == F32:
        return 0.0 * y
    if fmt == BF16:
        return 2.0 ** -8 * y if plane == 0 else 2.0 ** -11 * y + 2.0 ** -25
    return 2.0 ** -22 * y + 2.0 ** -29


def center_x(family, d, n):
    """The centring cases' rows, fp32 [n][d]."""
    return np.stack([row(family, d, r) for r in range(n)])


def center_bars(x, v4):
    """(bar [n], errs [n][2], floored [n], ref fp64 [n][d]) of the centred rows: the restatements are
    fl32(x - mean) with the kernel-order mean of the form that runs (``v4``) and with numpy's."""
    x = np.asarray(x, dtype=np.float32)
    x64 = x.astype(np.float64)
    mean = x64.mean(-1)
    ref = x64 - mean[:, None]
    errs = np.stack([row_err(x - m[:, None], ref) for m in (mean_kernel_order(x, v4),
                                                           x.sum(-1, dtype=np.float32) / np.float32(x.shape[1]))], 1)
    floor = FLOOR_ULPS * EPS24 * np.maximum(np.abs(ref).max(-1), np.abs(mean))
    raised = BAR_MARGIN * errs.max(-1)
    return np.maximum(raised, floor), errs, floor >= raised, ref


# ------------------------------------------------------------------------------ one launch and its buffers
def gammas(d):
    """Two gammas that differ per column and from each other: a swap or an offset by a group cannot pass."""
    c = np.arange(d, dtype=np.float64)
    return (1.0 + c / d).astype(np.float32), (2.0 - c / d).astype(np.float32)


class Launch:
    """One tvr_lnpre_rows call.  ``x`` fp32 [x_rows][d] (logical rows); ``idx`` the rows the launch reads
    (default: the first ``rows``); the device's x is ``x_buffer()``: stride ldx, the padding columns and the
    rows no idx names hold XPAD32."""

    def __init__(self, fmt, x, idx=None, rows=None, ldx=None, ldy=None, eps=1e-5, stats=True, copy_rows=None,
                 g1=None, g2=None):
        self.fmt, self.x = fmt, np.ascontiguousarray(x, dtype=np.float32)
        self.x_rows, self.d = self.x.shape
        self.idx = None if idx is None else np.asarray(idx, dtype=np.int32)
        self.rows = (self.x_rows if rows is None else rows) if idx is None else len(self.idx)
        self.ldx = self.d if ldx is None else ldx
        self.ldy = self.d if ldy is None else ldy
        self.eps, self.stats, self.copy_rows, self.g1, self.g2 = eps, stats, copy_rows, g1, g2

    def src(self):
        return np.arange(self.rows) if self.idx is None else self.idx

    def x_buffer(self):
        buf = np.full((self.x_rows, self.ldx), XPAD32, dtype=np.uint32)
        named = np.unique(self.src())
        buf[named, :self.d] = self.x[named].view(np.uint32)
        return buf

    def gathered(self):
        return self.x[self.src()]


def guarded(body, fill):
    """body [rows][w] between GUARD rows of ``fill`` on both sides."""
    g = np.full((GUARD, body.shape[1]), fill, dtype=body.dtype)
    return np.concatenate([g, body, g])


def planes_of(fmt, o, mutate=None):
    """[2][rows][d] uint16 planes of fp32 o in a 16-bit format."""
    if fmt == BF16:
        p1 = bf16_bits(o) if mutate == "bf16_plane1_bf16" else o.astype(np.float16).view(np.uint16)
        return np.stack([bf16_bits(o), p1])
    if mutate == "no_x16":
        p0 = o.astype(np.float16)
        return np.stack([p0.view(np.uint16), (o - p0.astype(np.float32)).astype(np.float16).view(np.uint16)])
    with np.errstate(over="ignore", invalid="ignore"):
        return split_act(o, X2F16)


def out_buffer(fmt, o, ldy, mutate=None):
    """The whole y buffer (guards included) holding o [rows][d]: uint32 [.][ldy] (fp32) or uint16 [.][2 ldy]."""
    n, d = o.shape
    if fmt == F32:
        body = np.full((n, ldy), NAN32, dtype=np.uint32)
        body[:, :d] = o.view(np.uint32)
        if mutate == "drop_last_f4" and (d // 4) % 64 != 0:  # (the partial last group's last float4)
            body[:, d - 4:d] = NAN32
        return guarded(body, NAN32)
    planes = planes_of(fmt, o, mutate)
    layout = X2F16 if fmt == IL and mutate == "il_written_planar" else fmt
    if mutate == "drop_last_f4" and (d // 4) % 64 != 0:
        planes[:, :, d - 4:] = NAN16[fmt]
    return guarded(G.act_buffer(planes, layout, ldy), NAN16[fmt])


def expected(L, stats, mutate=None):
    """Every buffer of launch L, bit for bit, given the device's (mean, scale) fp32 [rows][2] of its rows:
    dict y, y2 (or None), copy (or None; uint32 [GUARD + rows + GUARD][ldx]).  Rows whose input holds a NaN or
    an Inf are NaN in every plane (their bit patterns are not predicted: compare them with ``nan_rows``)."""
    xs = L.gathered()
    stats = np.asarray(stats, dtype=np.float32)
    o = normalise(xs, stats[:, 0], stats[:, 1])
    g1, g2 = L.g1, L.g2
    if mutate == "swap_gammas" and g2 is not None:
        g1, g2 = g2, g1
    if mutate == "gamma_group_repeat" and g1 is not None:
        c = np.arange(L.d)
        g1 = g1[np.where(c >= GAMMA_GROUP, c - GAMMA_GROUP, c)]
        g2 = None if g2 is None else g2[np.where(c >= GAMMA_GROUP, c - GAMMA_GROUP, c)]
    with np.errstate(invalid="ignore", over="ignore"):
        out = {"y": out_buffer(L.fmt, o if g1 is None else o * g1[None, :], L.ldy, mutate),
               "y2": None if g2 is None else out_buffer(L.fmt, o * g2[None, :], L.ldy, mutate), "copy": None}
    if L.copy_rows is not None:
        body = np.full((L.rows, L.ldx), NAN32, dtype=np.uint32)
        k = min(L.rows, L.copy_rows)
        src = np.arange(k) if mutate == "copy_from_r" else L.src()[:k]
        body[:k, :L.d] = L.x[src].view(np.uint32)
        out["copy"] = guarded(body, NAN32)
    return out


def expected_stats(L, stats64, mutate=None):
    """fp64 [rows][2] (mean, scale) in the order the launch stores them: by output row."""
    s = np.asarray(stats64)
    if mutate == "stats_by_source":  # row r's statistics stored at stats[row_idx[r]]
        out = np.full_like(s, np.nan)
        ok = L.src() < L.rows
        out[L.src()[ok]] = s[ok]
        return out
    return s


LAYOUT_MUTATIONS = ("drop_last_f4", "swap_gammas", "gamma_group_repeat", "il_written_planar", "copy_from_r",
                    "bf16_plane1_bf16", "no_x16")


def nan_rows(x):
    """Rows of x holding a NaN or an Inf: NaN throughout in every output."""
    return ~np.isfinite(np.asarray(x)).all(-1)


def decode(fmt, buf, ldy, rows, d, plane=0):
    """The values a y buffer (guards included) holds, fp64 [rows][d]; x2f16: (p0 + p1) / 16; bf16: ``plane``."""
    body = buf[GUARD:GUARD + rows]
    if fmt == F32:
        return body.view(np.float32)[:, :d].astype(np.float64)
    planes = act_logical(np.ascontiguousarray(body), fmt, ldy)[:, :, :d]
    if fmt == BF16:
        v = G.bf16_value(planes[0]) if plane == 0 else np.ascontiguousarray(planes[1]).view(np.float16)
        return v.astype(np.float64)
    return G.decode_act(np.ascontiguousarray(planes), X2F16)
