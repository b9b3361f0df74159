"""The row-statistics reference and patterns of stats_cases.py, on the CPU.

* the reference on hand-written rows with known answers (ties, all-equal rows);
* every forced pattern has the winners it is meant to have;
* an fp32 emulation of the kernels' formula exp(x - max) / sum, with a blocked
  and with a pairwise summation, stays within a quarter of both probability
  bars of test_gpu_row_statistics.py on every pattern at V = 50304 — so the
  bars leave a correct kernel room, and a kernel that misses them is wrong.
  (A purely sequential 50k-term fp32 sum would not fit; no kernel sums so.)
"""
import numpy as np
import pytest

import stats_cases as S

V_BIG = 50304


def test_reference_hand_written_rows():
    p, top = S.reference(np.array([0.0, 0.0, 0.0, 0.0], dtype=np.float32), [0, 3, None], 4)
    assert p.tolist() == [0.25, 0.25, 0.0] and top.tolist() == [0, 1, 2, 3]
    # ties resolve to the lowest id, wherever they sit
    p, top = S.reference(np.array([1.0, 3.0, 2.0, 3.0, 1.0, 3.0], dtype=np.float32), [1], 5)
    assert top.tolist() == [1, 3, 5, 2, 0]
    assert p[0] == pytest.approx(np.e ** 3 / (3 * np.e ** 3 + np.e ** 2 + 2 * np.e), rel=1e-15)
    # log 2 steps: probabilities 4/7, 2/7, 1/7
    row = np.array([0.0, np.log(2.0), np.log(4.0)], dtype=np.float32)
    p, top = S.reference(row, [2, 1, 0], 1)
    assert top.tolist() == [2] and np.allclose(p, [4 / 7, 2 / 7, 1 / 7], rtol=1e-7)
    # a spike: the rest underflows to exactly 0 in fp64 as well; a common offset changes nothing
    p, top = S.reference(np.array([-3e4, 3e4, -3e4], dtype=np.float32), [1, 0], 3)
    assert p.tolist() == [1.0, 0.0] and top.tolist() == [1, 0, 2]
    a, _ = S.reference(np.array([1e6, 1e6 + 1, 1e6 - 2], dtype=np.float32), [0, 1, 2], 1)
    b, _ = S.reference(np.array([0.0, 1.0, -2.0], dtype=np.float32), [0, 1, 2], 1)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("V", [260, 509, 512, V_BIG])
def test_patterns_have_their_winners(V):
    nt = S.n_tiles(V)
    top = {n: S.pattern_ref(n, V).topk(16).tolist() for n in S.PATTERNS}
    assert top["zeros"] == list(range(16))
    assert top["increasing"] == list(range(V - 1, V - 17, -1))
    assert top["decreasing"] == list(range(16))
    cols = S.plateau_columns(V)
    assert len(cols) == 20 and top["plateau"] == cols[:16]
    assert {255, 256, V - 1} <= set(cols) and (V <= 512 or {511, 512} <= set(cols))
    if V == V_BIG:  # the tile pairs l / l + 64 share a lane of stats_merge_kernel
        assert {256 * 64 + 1, 256 * 65 + 1, 256 * 128 + 1, 256 * 129 + 1} <= set(cols)
        assert min(V - c for c in top["increasing"]) == 1 and all(c // 256 == nt - 1 for c in top["increasing"])
    c = S.tier_base(V)
    assert top["two_tiers"] == [c + o for o in S.TIER_A_OFF] + [c + o for o in sorted(S.TIER_B_OFF)[:6]]
    assert len({(c + o) // 256 for o in S.TIER_A_OFF + S.TIER_B_OFF}) == 1
    q = S.pattern_ref("quantised", V)
    assert len(np.unique(q.row)) < V // 4 and len(np.unique(q.row[top["quantised"]])) < 16  # ties inside the top 16
    assert not np.signbit(q.row[q.row == 0]).any()  # no -0: the forced logits are compared bit for bit
    assert top["spike"][0] == S.spike_column(V) and top["spike"][1:4] == [0, 1, 2]
    assert S.pattern_ref("spike", V).p[0] == 0.0
    assert float(S.pattern_ref("offset", V).row.min()) > 9e5
    w = S.pattern_ref("wide", V)
    if V == V_BIG:
        assert w.p.min() < 1e-40 and any(1e-30 <= w.p[t] < 1e-28 for t in S.row_targets(w, 70) if t is not None)
    # the targets cycle through every kind, differ between rows, and stay in range
    for n in S.PATTERNS:
        ref = S.pattern_ref(n, V)
        tg = S.row_targets(ref, 300)
        assert all(t is None or 0 <= t < V for t in tg) and tg[6] is None and tg[4] == V - 1
        assert tg[0] == top[n][0] and tg[2] % 256 == 0 and ((tg[3] + 1) % 256 == 0 or tg[3] == V - 1)
        assert len({t for t in tg if t is not None}) >= min(8, V // 64)


@pytest.mark.parametrize("V", [512, V_BIG])
def test_sliding_block_construction(V):
    a, b, block = S.sliding_block(V)
    assert a.dtype == b.dtype == np.float32 and set(np.unique(a)) == {0.0, 1.0}
    assert a.sum() == S.BLOCK_N and np.all(b[block] == 0) and np.all(a[block] == 1)
    j = b[a == 0] / S.RUNG
    assert np.all(j == np.round(j)) and set(j.astype(int)) == set(S.RUNG_J)  # every rung of the ladder is used
    tiles = {int(c) // 256 for c in block}
    assert tiles == set(S.regions(V))
    if V == V_BIG:
        assert {5, 69, 133, S.n_tiles(V) - 1, 0} <= tiles
    assert {int(c) % 4 for c in block} == {0, 1, 2, 3} or V == 512
    # the block is cut by k = 16 at a different place for every rung gap above -1.5, and left out below
    lists = set()
    for s in np.arange(-3.2, 6.3, 0.5):
        assert not S.near_rung(float(s))
        row = S.sliding_row(a, b, np.float32(s))
        top = S.RowRef(row).topk(16).tolist()
        n_block = len(set(top) & set(block.tolist()))
        above = int((row > np.float32(s)).sum())
        assert n_block == min(S.BLOCK_N, max(0, 16 - above))
        if n_block:
            assert sorted(set(top) & set(block.tolist())) == block[:n_block].tolist()  # lowest ids first
        lists.add(tuple(top))
    assert len(lists) >= 14
    assert S.near_rung(0.5004) and S.near_rung(-2.9995) and not S.near_rung(0.502)


@pytest.mark.parametrize("order", ["blocked", "pairwise"])
@pytest.mark.parametrize("name", list(S.PATTERNS))
def test_fp32_formula_fits_a_quarter_of_the_bars(name, order):
    ref = S.pattern_ref(name, V_BIG)
    got = S.emulate_fp32(ref.row, order).astype(np.float64)
    dp = np.abs(got - ref.p)
    worst_abs = float((dp / (S.ABS_BAR * ref.pmax)).max())
    live = ref.p >= S.REL_FLOOR
    bar = S.rel_bar(ref.p[live], ref.xmax, ref.row[live].astype(np.float64))
    worst_rel = float((dp[live] / bar).max())
    print(f"{name} {order}: worst |dp| / abs bar {worst_abs:.3f}, / rel bar {worst_rel:.3f}")
    assert worst_abs <= 0.25 and worst_rel <= 0.25
