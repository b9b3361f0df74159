"""CPU: the LayerNormPre and centring cases of tests/norm_cases.py judge themselves: both fp32 restatements pass
their own bars with the margin to spare, the floor sets the output bar in at most a quarter of the graded rows,
the const rows and the exact prediction are exact, and every planted mutation of the reference misses a bar or
an exact comparison."""
import numpy as np
import pytest

import attribution_cases as C
import gemm_cases as G
import norm_cases as N

EPS = (1e-5, 1e-2)
WIDTHS = tuple(sorted(set(N.D_ALL + N.D_IL)))
CONST_D = (4, 64, 256, 4096)


def stats32(x, eps):
    m, s = N.stats_kernel_order(x, eps)
    return np.stack([m, s], 1)


def test_constants_are_the_projects():
    assert N.BAR_MARGIN is C.BAR_MARGIN and N.FLOOR_ULPS is C.FLOOR_ULPS and N.EPS24 is C.EPS24
    assert N.split_act is G.split_act and N.bf16_bits is G.bf16_bits and N.act_logical is G.act_logical
    assert N.NAN16 is G.NAN16 and (N.X2F16, N.IL, N.BF16) == (G.X2F16, G.IL, G.BF16)
    assert sorted(N.SEED) == list(WIDTHS)
    assert {N.path_of(d) for d in N.D_SMALL} == {"3pass", "nv10"} and N.path_of(256) == "nv10"
    assert [N.path_of(d) for d in N.D_LARGE] == ["nv10", "nv10", "nv20", "nv20", "3pass", "3pass"]


def test_restatements_pass_their_own_bars_and_the_floor_share():
    floored = np.zeros(3, int)
    graded = 0
    for d in WIDTHS:
        for eps in EPS:
            b = N.pool_bars(d, eps)
            bars = np.stack([b.mean, b.scale, b.y], 1)
            assert (bars > 0).all() and (b.err.max(-1) <= bars / N.BAR_MARGIN).all(), (d, eps)
            floored += b.floored.sum(0)
            graded += len(N.GRADED)
    print(f"the floor sets the bar of the mean / the scale / the outputs in {floored} of {graded} graded rows")
    # the outputs' bar: the condition, and the exact count (norm_cases.SEED)
    assert (int(floored[2]), graded) == (28, 150) and floored[2] <= graded // 4
    # the statistics' bars are mostly the floor's (a fp32 sum is within a fraction of an ulp of mean|x|): recorded
    assert floored[:2].tolist() == [110, 100]


def test_centring_restatements_pass_their_own_bar():
    floored = graded = 0
    for d in N.CENTER_D:
        for v4 in (True, False) if d % 4 == 0 else (False,):
            for fam in ("randn", "offset"):
                x = N.center_x(fam, d, 5)
                bar, errs, fl, ref = N.center_bars(x, v4)
                assert (bar > 0).all() and (errs.max(-1) <= bar / N.BAR_MARGIN).all(), (d, v4)
                floored += int(fl.sum())
                graded += len(x)
    # one rounding of x - mean and the mean's own error: nearly always under 4 x 2^-24 of the larger of them,
    # so the floor sets most of these bars (recorded, not under the outputs' condition)
    print(f"centring: the floor sets the bar in {floored} of {graded} rows")
    assert (floored, graded) == (79, 100)
    # the two kernel forms add in different orders: at the logits width they differ
    x = N.center_x("offset", 50304, 5)
    assert (N.mean_kernel_order(x, True) != N.mean_kernel_order(x, False)).any()


def test_families_are_what_they_claim():
    for d in WIDTHS:
        x = N.pool(d).astype(np.float64)
        fam = dict(zip(N.GRADED, x))
        mean, scale, y, _, _ = N.reference(N.pool(d), 1e-5)
        ref = dict(zip(N.GRADED, zip(mean, scale, y)))
        assert abs(fam["offset"].mean() - 1000) < 3 and fam["offset"].std() < 3
        if d >= 64:
            assert np.abs(y[N.GRADED.index("spike")]).max() > 0.98 * np.sqrt(d - 1)
            a = np.abs(fam["decades"])
            assert a.max() / a[a > 0].min() > 1e6
        # small: eps dominates the scale, and no square of a centred value is subnormal
        m, s, _ = ref["small"]
        assert abs(s - np.sqrt(np.float32(1e-5))) < 1e-6 * s
        c = (N.pool(d)[N.GRADED.index("small")] - np.float32(m)).astype(np.float32)
        sq = (c * c)[c != 0]
        assert sq.dtype == np.float32 and (sq >= np.finfo(np.float32).tiny).all()
        # offset: the one-pass variance is wrong in fp32, the two-pass one is not
        if d >= 64:
            xo = N.pool(d)[[N.GRADED.index("offset")]]
            b = N.Bars(xo, 1e-5)
            bad = N.stats_numpy(xo, 1e-5, "one_pass")[1]
            assert not abs(float(bad[0]) - b.ref[1][0]) <= b.scale[0]


@pytest.mark.parametrize("d", CONST_D)
def test_const_rows_are_exactly_zero_in_every_format(d):
    x = np.stack([N.row("const", d, 0)] * 3)
    g1, g2 = N.gammas(d)
    for eps in EPS:
        for m, s in (N.stats_kernel_order(x, eps), N.stats_numpy(x, eps)):
            assert (m == np.float32(1.5)).all() and (s == np.sqrt(np.float32(eps))).all()
            assert s.dtype == np.float32
        st = stats32(x, eps)
        for fmt in N.FMTS:
            if fmt == N.IL and d % 32:
                continue
            gam = [(None, None)] + ([(g1, None), (g1, g2)] if fmt in (N.X2F16, N.IL) else [])
            for a, b in gam:
                out = N.expected(N.Launch(fmt, x, eps=eps, g1=a, g2=b, ldy=d + 32), st)
                for k in ("y", "y2"):
                    if out[k] is not None:
                        body = out[k][N.GUARD:-N.GUARD]
                        used = body[:, :d] if fmt == N.F32 else N.act_logical(body, fmt, d + 32)[:, :, :d]
                        assert not used.any(), (fmt, k)   # +0: every bit clear


def test_exact_prediction_helpers():
    d, eps = 288, 1e-5
    x, _ = N.take(d, 5)
    st = stats32(x, eps)
    o = N.normalise(x, st[:, 0], st[:, 1])
    b = N.pool_bars(d, eps)
    g1, g2 = N.gammas(d)
    ld = d + 32
    # fp32: the buffer holds o itself between the guards and the NaN padding
    y = N.expected(N.Launch(N.F32, x, ldy=ld), st)["y"]
    assert y.shape == (5 + 2 * N.GUARD, ld) and (y[N.GUARD:-N.GUARD, :d] == o.view(np.uint32)).all()
    assert (y[:N.GUARD] == N.NAN32).all() and (y[-N.GUARD:] == N.NAN32).all() and (y[:, d:] == N.NAN32).all()
    # the interleaved buffer is the planar one permuted by act_logical; bytes differ
    p = N.expected(N.Launch(N.X2F16, x, ldy=ld, g1=g1, g2=g2), st)
    i = N.expected(N.Launch(N.IL, x, ldy=ld, g1=g1, g2=g2), st)
    for k in ("y", "y2"):
        assert (N.act_logical(p[k], N.X2F16, ld) == N.act_logical(i[k], N.IL, ld)).all() and (p[k] != i[k]).any()
        assert (N.act_logical(p[k], N.X2F16, ld)[:, :, d:] == N.NAN16[N.X2F16]).all()
    # the decoded planes are the reference within the row's bar plus the format's rounding, in every format
    _, _, yr, y1, y2 = N.reference(x, eps, g1, g2)
    for fmt in N.FMTS:
        buf = N.expected(N.Launch(fmt, x, ldy=ld), st)["y"]
        for plane in (0, 1) if fmt == N.BF16 else (0,):
            err = np.abs(N.decode(fmt, buf, ld, 5, d, plane) - yr)
            assert (err <= b.y[:, None] + N.fmt_round(fmt, yr, plane)).all(), (fmt, plane)
    for k, ref, g in (("y", y1, g1), ("y2", y2, g2)):
        err = np.abs(N.decode(N.IL, i[k], ld, 5, d) - ref)
        assert (err <= b.y[:, None] * g[None, :] + N.EPS24 * np.abs(ref) + N.fmt_round(N.IL, ref)).all()
    # the formats' unit roundoffs are reached: no smaller rounding term holds for a correctly rounded conversion
    for fmt, plane, v, u in ((N.BF16, 0, 1 + 2.0 ** -8, 2.0 ** -8), (N.BF16, 1, 1 + 2.0 ** -11, 2.0 ** -11)):
        q = N.planes_of(N.BF16, np.full((1, 4), v, np.float32))[plane]
        val = G.bf16_value(q) if plane == 0 else q.view(np.float16)
        assert (np.abs(val.astype(np.float64) - v) == u).all() and u <= N.fmt_round(fmt, v, plane) < 1.01 * u + 2.0 ** -25
    # bf16 plane 1 is fp16(o), not bf16(o)
    planes = N.planes_of(N.BF16, o)
    assert (planes[1] == o.astype(np.float16).view(np.uint16)).all() and (planes[0] == G.bf16_bits(o)).all()
    # a gather: output row r is the row of x[idx[r]], the copy too, the statistics in output order
    xs = np.concatenate([x, x[:2] + np.float32(1)])
    idx = [6, 0, 0, 3]
    L = N.Launch(N.F32, xs, idx=idx, copy_rows=3, ldx=d + 4)
    assert (L.gathered() == xs[idx]).all() and L.rows == 4 and L.x_rows == 7
    xb = L.x_buffer()
    assert (xb[[1, 2, 4, 5]] == N.XPAD32).all() and (xb[:, d:] == N.XPAD32).all() and (xb[6, :d] == xs[6].view(np.uint32)).all()
    c = N.expected(L, stats32(xs[idx], eps))["copy"][N.GUARD:-N.GUARD]
    assert (c[:3, :d] == xs[idx[:3]].view(np.uint32)).all() and (c[3] == N.NAN32).all() and (c[:, d:] == N.NAN32).all()


@pytest.mark.parametrize("mutate", N.STAT_MUTATIONS)
def test_every_mutation_of_the_statistics_misses_a_bar(mutate):
    hits = total = 0
    for d in WIDTHS:
        if mutate == "drop_last_f4" and (d // 4) % 64 == 0:
            continue  # (the mistake is a partial last group's)
        for eps in EPS:
            b = N.pool_bars(d, eps)
            m, s = N.stats_numpy(N.pool(d), eps, mutate, ldx=d + 32)
            miss_m = ~(np.abs(m.astype(np.float64) - b.ref[0]) <= b.mean)
            miss_s = ~(np.abs(s.astype(np.float64) - b.ref[1]) <= b.scale)
            y = N.normalise(N.pool(d), m, s)
            miss_y = ~(N.row_err(y, b.ref[2]) <= b.y)
            miss = dict(zip(N.GRADED, miss_m | miss_s | miss_y))
            total += 1
            hits += any(miss.values())
            if mutate == "one_pass":
                # cancellation: certain where the mean dwarfs the spread
                assert miss["offset"] or d < 64, (d, eps)
            elif mutate == "eps_outside":
                assert miss["small"], (d, eps)          # eps dominates: sqrt(eps) against eps
                assert eps < 1e-3 or all(miss.values()), (d, eps)
            elif mutate == "d_minus_1":
                assert all(miss[f] for f in ("randn", "offset", "decades")) or d > 768, (d, eps)
                assert miss["randn"] or miss["offset"], (d, eps)
            elif mutate == "mean_over_ldx":
                assert all(miss[f] for f in ("randn", "offset", "spike")), (d, eps)
            else:
                assert all(miss[f] for f in ("randn", "offset")), (d, eps)
    assert hits == total and total > 0, (mutate, hits, total)


def _layout_launches():
    """Launches on which each layout mutation must show: (fmt, d, gammas, gather, copy)."""
    out = []
    for fmt in N.FMTS:
        for d in (100, 288, 2816):
            if fmt == N.IL and d % 32:
                continue
            x, _ = N.take(d, 7)
            g1, g2 = N.gammas(d) if fmt in (N.X2F16, N.IL) else (None, None)
            out.append(N.Launch(fmt, x, idx=[6, 5, 4, 3, 2, 1, 0][:5], ldx=d + 32, ldy=d + 32, copy_rows=4, g1=g1, g2=g2))
    return out


@pytest.mark.parametrize("mutate", N.LAYOUT_MUTATIONS)
def test_every_mutation_of_the_outputs_fails_the_exact_comparison(mutate):
    applies = {"swap_gammas": lambda L: L.g2 is not None, "gamma_group_repeat": lambda L: L.g1 is not None and L.d > N.GAMMA_GROUP,
               "il_written_planar": lambda L: L.fmt == N.IL, "bf16_plane1_bf16": lambda L: L.fmt == N.BF16,
               "no_x16": lambda L: L.fmt in (N.X2F16, N.IL), "drop_last_f4": lambda L: (L.d // 4) % 64 != 0}
    seen = 0
    for L in _layout_launches():
        st = stats32(L.gathered(), L.eps)
        good, bad = N.expected(L, st), N.expected(L, st, mutate)
        differs = any(good[k] is not None and (good[k] != bad[k]).any() for k in ("y", "y2", "copy"))
        if applies.get(mutate, lambda L: True)(L):
            assert differs, (mutate, L.fmt, L.d)
            seen += 1
            if mutate == "copy_from_r":
                assert (good["y"] == bad["y"]).all() and (good["copy"] != bad["copy"]).any()
        else:
            assert not differs, (mutate, L.fmt, L.d)
    assert seen > 0, mutate


def test_stats_indexed_by_source_row_miss_the_bar():
    d, eps = 100, 1e-5
    x, _ = N.take(d, 5)
    for idx in ([4, 3, 2, 1, 0], [0, 0, 3, 3, 1]):
        L = N.Launch(N.F32, x, idx=idx)
        b = N.Bars(L.gathered(), eps)
        ref = np.stack([b.ref[0], b.ref[1]], 1)
        assert (N.expected_stats(L, ref) == ref).all()
        bad = N.expected_stats(L, ref, "stats_by_source")
        miss = ~(np.abs(bad[:, 0] - ref[:, 0]) <= b.mean) | ~(np.abs(bad[:, 1] - ref[:, 1]) <= b.scale)
        assert miss.sum() >= 3, (idx, miss)   # every row that is not its own source
