"""Planar-GEMM operands with known answers, their fp64 reference and the bars
(shared by test_gemm_cases.py and test_gpu_gemm_forms.py; a plain module, not
a conftest).  Everything here is numpy / torch on the CPU.

The operation is C = A W^T (+ bias, + residual, GELU on the columns from
n_split on) as ``gemm_pingpong_kernel`` and its launch forms compute it
(csrc/gemm_pingpong.hpp, engine.hip launch_gemm).  The reference works from
the values the kernel reads: the planes of the activation format
(``split_act``: what tvr_act_rows writes) and of the weights (``split_w``:
tvr_weight_planes) decoded to fp64, (p0 + p1) / 16 and (p0 + p1) / scale.  The
GPU file checks once that the device's planes are these bits, so the host
emulation and the device agree on what the kernel is given; the splits
themselves are judged elsewhere (tests/test_gpu_engine.py).

Three families of operands (``Case.kind``):

* ``int``     small signed integers from index formulas of (m, k), (n, k), (n)
              and (m, n).  Every plane is exact (fp16 of 16 a, fp16 of
              scale w with scale a power of two, bf16), the weights' residual
              plane is zero (so the same weights serve the one-plane form), and
              every partial sum in any order is an integer below 2^24
              (``int_bound``): every launch form, format, slicing choice and
              plane count must return the integer result bit for bit.
* ``onehot``  row m of A is e_k(m), k(m) = (37 m + m // 64) mod K walking
              through every position of a 32- / 64-column group and every
              k-tile: C[m, n] is the decoded W[n, k(m)] exactly (the sum of the
              two weight planes fits fp32: 22 significand bits).
* ``graded``  randn operands whose columns' magnitudes spread over six
              decades (A) with weights near 1e-3 of fp16's natural range (two
              planes) or fp16-valued (one plane); judged per element by
              ``Bar``.

The bar of a graded case is never taken from the engine: two fp32 restatements
of the same sum (``restate``: the three / two products of each 32-deep slice in
the kernel's order, then the slices serially — or pairwise), their worst error
against the fp64 reference relative to (|A| |W|)_ij + |bias_j| + |resid_ij|,
times 4, floored at one fp32 ulp of the result (the fp32 store alone rounds by
half an ulp).  The GELU planes are judged against erf-GELU in fp64 of the
device's own fp32 pre-activation (``gelu_bar``).
"""
from __future__ import annotations

import math

import numpy as np
import torch

X2F16, IL, BF16 = 2, 0x12, 3          # include/tvr.h TVR_GEMM_X2F16, TVR_ACT_X2F16_IL, TVR_GEMM_BF16
EPI_BIAS, EPI_GELU, EPI_RESID = 0, 1, 2
KTILE = {X2F16: 32, IL: 32, BF16: 64}
NAN16 = {X2F16: 0x7E00, IL: 0x7E00, BF16: 0x7FC0}   # a quiet NaN of the plane's number format
BAR_MARGIN = 4.0
INT_WSCALE = 1024.0                   # the integer cases' weight scale: 8 * 1024 is exact in fp16


# ------------------------------------------------------------------ number formats
def bf16_bits(x):
    """fp32 -> bf16 bits, round to nearest even (split.hpp bf16_bits; NaN stays NaN)."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def split_act(a, fmt):
    """Activation planes [2][...] (uint16 bits) of fp32 ``a`` as tvr_act_rows writes them: x2f16 plane 0 =
    fp16(16 a), plane 1 = fp16(16 a - plane 0); bf16 plane 0 = bf16(a), plane 1 unused (zero here)."""
    a = np.asarray(a, dtype=np.float32)
    if fmt == BF16:
        return np.stack([bf16_bits(a), np.zeros(a.shape, np.uint16)])
    x = a * np.float32(16.0)
    p0 = x.astype(np.float16)
    p1 = (x - p0.astype(np.float32)).astype(np.float16)
    return np.stack([p0.view(np.uint16), p1.view(np.uint16)])


def split_w(w, fmt, scale):
    """Weight planes as tvr_weight_planes writes them: x2f16 [2][...] of w * scale, bf16 [1][...]."""
    w = np.asarray(w, dtype=np.float32)
    if fmt == BF16:
        return bf16_bits(w)[None]
    x = w * np.float32(scale)
    p0 = x.astype(np.float16)
    p1 = (x - p0.astype(np.float32)).astype(np.float16)
    return np.stack([p0.view(np.uint16), p1.view(np.uint16)])


def plane_values(planes, fmt):
    """uint16 planes -> fp32 values of each plane."""
    if fmt == BF16:
        return bf16_value(planes)
    return np.asarray(planes, dtype=np.uint16).view(np.float16).astype(np.float32)


def engine_wscale(w):
    """The engine's x2f16 weight scale: 2^(15 - ceil log2 max|W|)."""
    return float(2.0 ** (15 - math.ceil(math.log2(float(np.abs(w).max())))))


# ------------------------------------------------------------------ layouts (halves)
def act_buffer(planes, fmt, ld, rows_total=None, poison=True):
    """[2][R][K] planes -> the device buffer [rows_total][2 ld] uint16 in layout ``fmt`` (planar: plane p of
    column c at p ld + c; interleaved: (c / 32) 64 + 32 p + c % 32).  Columns [K, ld) and rows [R, rows_total)
    hold NaN (poison)."""
    _, R, K = planes.shape
    rows_total = R if rows_total is None else rows_total
    buf = np.full((rows_total, 2 * ld), NAN16[fmt] if poison else 0, dtype=np.uint16)
    if fmt == IL:
        assert K % 32 == 0 and ld % 32 == 0
        v = buf.reshape(rows_total, ld // 32, 2, 32)
        v[:R, :K // 32] = planes.reshape(2, R, K // 32, 32).transpose(1, 2, 0, 3)
    else:
        v = buf.reshape(rows_total, 2, ld)
        v[:R, :, :K] = planes.transpose(1, 0, 2)
    return buf


def act_logical(buf, fmt, ld):
    """The device buffer [rows][2 ld] -> [2][rows][ld] planes in logical columns."""
    rows = buf.shape[0]
    if fmt == IL:
        return buf.reshape(rows, ld // 32, 2, 32).transpose(2, 0, 1, 3).reshape(2, rows, ld)
    return buf.reshape(rows, 2, ld).transpose(1, 0, 2)


def decode_act(planes, fmt):
    """[2][...] planes -> fp64 values: (p0 + p1) / 16, or the bf16 plane."""
    v = plane_values(planes, fmt).astype(np.float64)
    with np.errstate(invalid="ignore"):  # (a value past the x2f16 range decodes as inf + nan)
        return v[0] if fmt == BF16 else (v[0] + v[1]) / 16.0


def decode_w(planes, fmt, scale, one_plane=False):
    v = plane_values(planes, fmt).astype(np.float64)
    if fmt == BF16:
        return v[0]
    return v[0] / scale if one_plane else (v[0] + v[1]) / scale


# ------------------------------------------------------------------ operands
def int_operands(M, N, K):
    m, n, k = np.arange(M)[:, None], np.arange(N)[:, None], np.arange(K)[None, :]
    A = ((7 * m + 3 * k) % 13 - 6).astype(np.float32)
    W = ((5 * n + 11 * k) % 17 - 8).astype(np.float32)
    bias = ((np.arange(N) * 5) % 23 - 11).astype(np.float32)
    resid = ((3 * np.arange(M)[:, None] + 5 * np.arange(N)[None, :]) % 29 - 14).astype(np.float32)
    return A, W, bias, resid


def int_bound(K):
    """The largest magnitude any partial sum of an integer case can reach, in any order, with the bias and the
    residual: 6 * 8 per product."""
    return 6 * 8 * K + 11 + 14


def onehot_k(M, K):
    m = np.arange(M)
    return (37 * m + m // 64) % K


def graded_operands(M, N, K, seed, fp16_weights):
    rng = np.random.default_rng([seed, M, N, K])
    A = (rng.standard_normal((M, K)) * 10.0 ** rng.uniform(-4.0, 2.0, size=K)[None, :]).astype(np.float32)
    W = rng.standard_normal((N, K))
    if fp16_weights:  # the one-plane form: values exact in fp16 (as a released checkpoint's), around 0.02
        W = (W * 0.02).astype(np.float16).astype(np.float32)
    else:             # far below fp16's natural range: the residual plane and its subnormals matter
        W = (W * 1e-3 * 10.0 ** rng.uniform(-3.0, 0.0, size=K)[None, :]).astype(np.float32)
    scale = np.abs(A).astype(np.float64) @ np.abs(W).astype(np.float64).T
    bias = (rng.standard_normal(N) * np.median(scale)).astype(np.float32)
    resid = (rng.standard_normal((M, N)) * np.median(scale)).astype(np.float32)
    return A, W, bias, resid


class Case:
    """Operands of one (kind, fmt family, M, N, K): fp32 A [M][K], W [N][K], bias [N], resid [M][N]; the
    planes ``ap`` [2][M][K] (zero_w_rows: rows of an integer case's W set to zero), ``wp`` [planes][N][K]; ``wscale``; ``one_plane``: the weights' plane 0 alone is
    exact (the one-plane form may run); ``ref`` fp64 [M][N] = A W^T of the decoded planes (no bias)."""

    def __init__(self, kind, fmt, M, N, K, one_plane=False, seed=0, zero_w_rows=()):
        assert fmt in (X2F16, BF16) and K % KTILE[fmt] == 0
        self.kind, self.fmt, self.M, self.N, self.K, self.one_plane = kind, fmt, M, N, K, one_plane
        if kind == "int":
            self.A, self.W, self.bias, self.resid = int_operands(M, N, K)
            self.W[list(zero_w_rows)] = 0.0  # output columns that are the bias alone
            self.wscale = INT_WSCALE if fmt == X2F16 else 1.0
            self.one_plane = True
        elif kind == "onehot":
            _, self.W, _, _ = graded_operands(M, N, K, seed, one_plane)
            self.A = np.zeros((M, K), np.float32)
            self.A[np.arange(M), onehot_k(M, K)] = 1.0
            self.bias, self.resid = np.zeros(N, np.float32), np.zeros((M, N), np.float32)
            self.wscale = engine_wscale(self.W) if fmt == X2F16 else 1.0
        else:
            assert kind == "graded", kind
            self.A, self.W, self.bias, self.resid = graded_operands(M, N, K, seed, one_plane)
            self.wscale = engine_wscale(self.W) if fmt == X2F16 else 1.0
        self.ap = split_act(self.A, fmt)
        self.wp = split_w(self.W, fmt, self.wscale)
        if self.one_plane and fmt == X2F16:
            assert not plane_values(self.wp, fmt)[1].any(), "one-plane weights: the residual plane must be zero"
        self.Ad, self.Wd = decode_act(self.ap, fmt), decode_w(self.wp, fmt, self.wscale)
        self.ref = self.Ad @ self.Wd.T
        self._bar = {}

    def expect(self, epi=EPI_BIAS, a_rows=None):
        """fp64 result of the fp32 columns (bias added; the residual under EPI_RESID)."""
        r = self.ref if a_rows is None else self.ref[np.asarray(a_rows)]
        out = r + self.bias.astype(np.float64)[None, :]
        if epi == EPI_RESID:
            out = out + self.resid.astype(np.float64)
        return out

    def denom(self, epi=EPI_BIAS):
        d = np.abs(self.Ad) @ np.abs(self.Wd).T + np.abs(self.bias.astype(np.float64))[None, :]
        if epi == EPI_RESID:
            d = d + np.abs(self.resid.astype(np.float64))
        return d

    def bar(self, epi=EPI_BIAS, two_products=False):
        """(bar [M][N], worst relative error of the serial restatement, of the pairwise one)."""
        key = (epi, two_products)
        if key not in self._bar:
            want, den = self.expect(epi), self.denom(epi)
            errs = []
            for order in ("serial", "pairwise"):
                got = restate(self, order, epi, two_products).astype(np.float64)
                errs.append(float((np.abs(got - want) / den).max()))
            floor = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            self._bar[key] = (np.maximum(BAR_MARGIN * max(errs) * den, floor), errs[0], errs[1])
        return self._bar[key]


def restate(case, order, epi=EPI_BIAS, two_products=False):
    """The kernel's sum in fp32 on the CPU: per 32-deep slice the products a1 w0, a0 w1, a0 w0 (x2f16; two
    products without a0 w1: the one-plane form; bf16: the one product), each a fp32 matrix product of the
    slice; ``serial``: every product added to the running sum in that order, slice after slice;
    ``pairwise``: each slice's products summed first, then the slices in a binary tree.  Then * 1 / (16
    scale), + bias, + residual, each rounded to fp32 as the epilogue does."""
    fmt, M, N, K = case.fmt, case.M, case.N, case.K
    S = K // 32
    a = plane_values(case.ap, fmt).reshape(2, M, S, 32).transpose(0, 2, 1, 3)   # [2][S][M][32]
    w = plane_values(case.wp, fmt)
    w = w.reshape(w.shape[0], N, S, 32).transpose(0, 2, 3, 1)                   # [planes][S][32][N]
    if fmt == BF16:
        prods = [np.matmul(a[0], w[0])]
    elif two_products:
        prods = [np.matmul(a[1], w[0]), np.matmul(a[0], w[0])]
    else:
        prods = [np.matmul(a[1], w[0]), np.matmul(a[0], w[1]), np.matmul(a[0], w[0])]
    assert all(p.dtype == np.float32 for p in prods)
    if order == "serial":
        acc = np.zeros((M, N), np.float32)
        for s in range(S):
            for p in prods:
                acc = acc + p[s]
    else:
        t = prods[0]
        for p in prods[1:]:
            t = t + p
        parts = list(t)
        while len(parts) > 1:
            nxt = [parts[i] + parts[i + 1] for i in range(0, len(parts) - 1, 2)]
            if len(parts) % 2:
                nxt.append(parts[-1])
            parts = nxt
        acc = parts[0]
    acc_scale = np.float32(1.0) if fmt == BF16 else np.float32(1.0 / (case.wscale * 16.0))
    out = acc * acc_scale + case.bias[None, :]
    if epi == EPI_RESID:
        out = out + case.resid
    assert out.dtype == np.float32
    return out


# ------------------------------------------------------------------ GELU
GELU_P = np.float32(0.3275911 * 0.70710678118654752440)
GELU_Q = np.float32(-0.5 * 1.44269504088896341)
GELU_A = [np.float32(v) for v in (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)]
GELU_SPLIT_REL = {X2F16: 2.0 ** -22, IL: 2.0 ** -22, BF16: 2.0 ** -8}   # the format's rounding of the value (bf16: 8 bits)
GELU_SPLIT_ABS = {X2F16: 2.0 ** -25 / 16, IL: 2.0 ** -25 / 16, BF16: 0.0}  # half the fp16 subnormal spacing / 16


def gelu64(x):
    """torch.nn.functional.gelu (erf form) in fp64."""
    return torch.nn.functional.gelu(torch.as_tensor(np.asarray(x, dtype=np.float64))).numpy()


def gelu_restate(x):
    """gelu_erf2's formula (csrc/gemm_f32.hpp) in numpy fp32: every step rounded to fp32 (the device fuses
    the multiply-adds and uses its own reciprocal and exp2: the margin of 4 covers the difference)."""
    x = np.asarray(x, dtype=np.float32)
    ax = np.abs(x)
    t = np.float32(1.0) / (ax * GELU_P + np.float32(1.0))
    p = GELU_A[4]
    for c in (GELU_A[3], GELU_A[2], GELU_A[1], GELU_A[0]):
        p = p * t + c
    p = p * t
    with np.errstate(under="ignore"):
        h = p * np.exp2(ax * (ax * GELU_Q) - np.float32(1.0)).astype(np.float32)
    out = np.maximum(x, np.float32(0.0)) - ax * h
    assert out.dtype == np.float32
    return out


def gelu_bar(raw, fmt):
    """Per-element bar of the decoded GELU planes against gelu64(raw): 4 x the restatement's worst error over
    these values (relative to max(1, |x|), the form of the kernel's documented error) + the format's split."""
    raw = np.asarray(raw, dtype=np.float32)
    g = gelu64(raw)
    unit = np.maximum(1.0, np.abs(raw.astype(np.float64)))
    e = float((np.abs(gelu_restate(raw).astype(np.float64) - g) / unit).max()) if raw.size else 0.0
    return BAR_MARGIN * e * unit + GELU_SPLIT_REL[fmt] * np.abs(g) + GELU_SPLIT_ABS[fmt], e


# ------------------------------------------------------------------ the raster (gemm_pingpong.hpp)
def tile_grid(M, N):
    return (M + 255) // 256, (N + 255) // 256


def group_m(N):
    return 2 if (N + 255) // 256 <= 16 else 4  # engine.hip pp_group_m


def tile_coords(t, M, N):
    """(m0, n0) of tile t of the grouped raster (pp_tile_coords)."""
    nbm, nbn = tile_grid(M, N)
    gm = group_m(N)
    per = gm * nbn
    grp = t // per
    first = grp * gm
    gsz = min(nbm - first, gm)
    r = t - grp * per
    return (first + r % gsz) * 256, (r // gsz) * 256


def tile_mask(M, N, t0, t1):
    """[M][N] bool: the elements of tiles [t0, t1)."""
    mask = np.zeros((M, N), dtype=bool)
    for t in range(t0, t1):
        m0, n0 = tile_coords(t, M, N)
        mask[m0:m0 + 256, n0:n0 + 256] = True
    return mask
