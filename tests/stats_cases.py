"""Logit rows with known answers for the row-statistics kernels, and their
high-precision reference (shared by test_stats_cases.py and
test_gpu_row_statistics.py; a plain module, not a conftest).

The engine's ``prob`` / ``topk`` come from ``row_stats_kernel`` (materialised
logits) or from the fused unembed statistics (``pp_stats_rows`` per 256-column
tile + ``stats_merge_kernel``).  include/tvr.h promises "descending, lowest id
on ties"; ``torch.topk`` promises no tie order, so the reference here is
``np.lexsort((ids, -values))`` and an fp64 softmax of the fp32 row.

Two ways to make the engine produce a chosen row without touching it:

* forced rows   W_U = 0: every logit row is exactly ``b_unembed``
  (``PATTERNS``: functions of V returning an fp32 row);
* sliding block W_U[v, :] = a[v] e_0 with a in {0, 1}: logits[r, v] =
  a[v] s_r + b[v], s_r the first coordinate of row r's final LayerNorm.  The
  a = 1 columns (b = 0) form one exactly tied block at s_r, the a = 0 columns
  sit on a ladder of rungs 0.5 j, j = -12 .. 12, so the block lands between
  different rungs in different rows (``sliding_block``).
"""
from __future__ import annotations

import functools

import numpy as np

TILE = 256          # columns per EPI_STATS tile (gemm_pingpong.hpp)
MERGE_LANES = 64    # stats_merge_kernel: lane l merges tiles l, l + 64, ...
TOPK = (1, 2, 5, 16)

# ----------------------------------------------------------------- the bars
ABS_BAR = 1e-5       # |dp| <= ABS_BAR * max p: the project's probability bar
REL_CONST = 16.0     # expf, the division and a blocked summation, in units of 2^-22
REL_UNIT = 2.0 ** -22
REL_FLOOR = 1e-30    # below it only the absolute bar (denormal results may be flushed)


def rel_bar(p, xmax, x_t):
    """|dp| <= p (max - x_t + 16) 2^-22: rounding x - max to fp32 is a relative
    error |x - max| 2^-24 of the exponential; 16 units cover expf, the
    division and a blocked summation.  Derived, not fitted to a kernel."""
    return p * (xmax - x_t + REL_CONST) * REL_UNIT


# ------------------------------------------------------------ the reference
class RowRef:
    """fp64 softmax and the (value desc, id asc) order of one logit row: the
    fp32 row a kernel reads (or that row reconstructed in fp64)."""

    def __init__(self, row):
        row = np.asarray(row)
        assert row.dtype in (np.float32, np.float64) and row.ndim == 1
        self.row = row
        x = row.astype(np.float64)
        self.xmax = float(x.max())
        e = np.exp(x - self.xmax)
        self.p = e / e.sum()
        self.pmax = float(self.p.max())
        self.order = np.lexsort((np.arange(row.shape[0]), -x))

    def probs(self, targets):
        """p[target] per target, 0 for None (the engine writes 0 without a target)."""
        return np.asarray([0.0 if t is None else self.p[t] for t in targets], dtype=np.float64)

    def topk(self, k):
        return self.order[:k].astype(np.int64)


def reference(row_fp32, targets, k):
    """(fp64 softmax probabilities of ``targets``, top-k ids by value
    descending then id ascending) of one fp32 logit row."""
    r = RowRef(row_fp32)
    return r.probs(targets), r.topk(k)


class RowSet:
    """What a batch of rows is checked against: per row its target (-1: none),
    the reference probability, the target's logit, the row's max and largest
    probability, and the reference top 16."""

    def __init__(self, items):
        """items: (RowRef, target or None) per row."""
        n = len(items)
        self.targets = [t for _, t in items]
        self.tg = np.asarray([-1 if t is None else t for t in self.targets], dtype=np.int64)
        self.p = np.zeros(n)
        self.x_t = np.zeros(n)
        self.xmax = np.asarray([r.xmax for r, _ in items])
        self.pmax = np.asarray([r.pmax for r, _ in items])
        self.top = np.stack([r.topk(max(TOPK)) for r, _ in items])
        for i, (r, t) in enumerate(items):
            if t is not None:
                self.p[i], self.x_t[i] = r.p[t], float(r.row[t])

    def take(self, idx):
        """The rows ``idx`` (in that order)."""
        out = object.__new__(RowSet)
        idx = np.asarray(idx)
        out.targets = [self.targets[i] for i in idx]
        for f in ("tg", "p", "x_t", "xmax", "pmax", "top"):
            setattr(out, f, getattr(self, f)[idx])
        return out

    def prob_ratios(self, got):
        """Worst |dp| over the absolute bar and over the relative bar (targets
        with reference p >= 1e-30); rows without a target must hold 0."""
        got = np.asarray(got, dtype=np.float64)
        has = self.tg >= 0
        assert got.shape == has.shape and np.isfinite(got).all()
        assert np.all(got[~has] == 0.0), "no target: the engine writes probability 0"
        dp = np.abs(got - self.p)[has]
        r_abs = dp / (ABS_BAR * self.pmax[has])
        live = self.p[has] >= REL_FLOOR
        r_rel = dp[live] / rel_bar(self.p[has][live], self.xmax[has][live], self.x_t[has][live])
        return float(r_abs.max(initial=0.0)), float(r_rel.max(initial=0.0))


# ------------------------------------------------------- column placements
def n_tiles(V):
    return (V + TILE - 1) // TILE


def tile_width(V, t):
    return min(TILE, V - t * TILE)


def regions(V):
    """Tiles where winners are placed: tile 0, a middle tile, tiles l, l + 64
    and l + 128 (merged by the same lane of stats_merge_kernel) and the last,
    possibly partial, tile."""
    nt = n_tiles(V)
    want = [0, nt // 2, 5, 5 + MERGE_LANES, 5 + 2 * MERGE_LANES, nt - 1]
    out = []
    for t in want:
        if 0 <= t < nt and t not in out:
            out.append(t)
    return out


# offsets inside a tile: its edges, then every column phase 16 i + 4 q + e of a quad of pp_stats_rows
_OFFSETS = [0, 255, 1, 254, 16 + 4 + 1, 48 + 8 + 2, 112 + 12 + 3, 128]
_OFFSETS += [o for o in ((37 * i + 5) % TILE for i in range(64)) if o not in _OFFSETS]


def key_columns(V, n, skip=()):
    """``n`` distinct columns cycling over ``regions(V)`` and the tile offsets above."""
    out, seen = [], set(int(c) for c in skip)
    for o in _OFFSETS:
        for t in regions(V):
            c = t * TILE + o % tile_width(V, t)
            if c not in seen:
                seen.add(c)
                out.append(c)
                if len(out) == n:
                    return out
    raise ValueError(f"V = {V}: fewer than {n} placement columns")


def _rng(V, salt):
    return np.random.default_rng(1000 * salt + V)


# ------------------------------------------------------ the forced patterns
def zeros(V):
    """All equal: p = 1 / V, top-k = 0 .. k - 1."""
    return np.zeros(V, dtype=np.float32)


def increasing(V):
    """Strictly increasing, v 2^-10: every winner in the last (partial) tile."""
    return (np.arange(V, dtype=np.float32) * np.float32(2.0 ** -10)).astype(np.float32)


def decreasing(V):
    """Strictly decreasing: every winner in tile 0."""
    return increasing(V)[::-1].copy()


def plateau_columns(V):
    edge = [255, 256, 511, 512, TILE * 64 + 1, TILE * 65 + 1, TILE * 128 + 1, TILE * 129 + 1, V - 1, V - 2, 0]
    cols = []
    for c in edge:
        if 0 <= c < V and c not in cols:
            cols.append(c)
    cols += key_columns(V, 20 - len(cols), skip=cols)
    return sorted(cols[:20])


def plateau(V):
    """20 columns share 5.0 on tile edges, tile pairs l / l + 64 and the last
    column, over N(0, 1) noise clipped below 4: top 16 = the 16 lowest of them."""
    x = np.minimum(_rng(V, 4).standard_normal(V), 3.75).astype(np.float32)
    x[plateau_columns(V)] = 5.0
    return x


TIER_A_OFF = (0, 1, 3, 4, 16, 17, 20, 37, 100, 200)   # same thread another element, another quad lane, next chunk
TIER_B_OFF = (2, 5, 6, 18, 19, 36, 52, 101, 150, 240)


def tier_base(V):
    """First column of the two-tier block: inside one full tile (the l + 64 tile when V has one)."""
    nt = n_tiles(V)
    full = [t for t in range(nt) if tile_width(V, t) == TILE]
    t = 5 + MERGE_LANES if 5 + MERGE_LANES in full else full[-1]
    return t * TILE + 8


def two_tiers(V):
    """Ten columns at A = 9 and ten at B = 8 inside one tile, over noise clipped
    below 3: top 16 = the ten A columns ascending, then the six lowest B columns."""
    x = np.minimum(_rng(V, 5).standard_normal(V), 2.75).astype(np.float32)
    c = tier_base(V)
    x[[c + o for o in TIER_A_OFF]] = 9.0
    x[[c + o for o in TIER_B_OFF]] = 8.0
    return x


def quantised(V):
    """round(3 N(0, 1) * 4) / 4: ties everywhere."""
    return (np.round(3.0 * _rng(V, 6).standard_normal(V) * 4.0) / 4.0 + 0.0).astype(np.float32)  # (+ 0: no -0)


def spike_column(V):
    return V // 3


def spike(V):
    """+3e4 at one column, -3e4 elsewhere: every other column underflows."""
    x = np.full(V, -3e4, dtype=np.float32)
    x[spike_column(V)] = 3e4
    return x


def offset(V):
    """1e6 + round(8 N(0, 1)): a naive exp overflows."""
    return (1e6 + np.round(8.0 * _rng(V, 8).standard_normal(V))).astype(np.float32)


def wide(V):
    """20 N(0, 1): targets down to p ~ 1e-30 (and below, where only the absolute bar holds)."""
    return (20.0 * _rng(V, 9).standard_normal(V)).astype(np.float32)


PATTERNS = {"zeros": zeros, "increasing": increasing, "decreasing": decreasing, "plateau": plateau,
            "two_tiers": two_tiers, "quantised": quantised, "spike": spike, "offset": offset, "wide": wide}


@functools.lru_cache(maxsize=None)
def pattern_ref(name, V) -> RowRef:
    """The pattern's row and its reference, computed once per (pattern, V)."""
    ref = RowRef(PATTERNS[name](V))
    ref.row.setflags(write=False)
    ref.p.setflags(write=False)
    ref.order.setflags(write=False)
    return ref


# ------------------------------------------------------------------ targets
N_TARGET_KINDS = 7


def row_target(ref: RowRef, r):
    """Row r's target, cycling through: the argmax, a mid-probability column,
    the first and the last column of a tile, column V - 1, a column of tiny
    probability (around the smallest p >= 1e-30 when the row goes below it:
    the last two at or above it, the first below), None."""
    V = ref.row.shape[0]
    kind, i = r % N_TARGET_KINDS, r // N_TARGET_KINDS
    if kind == 0:
        return int(ref.order[0])
    if kind == 1:
        return int(ref.order[min(V - 1, 17 + i % 5)])  # just outside the top 16
    if kind == 2:
        return (i % n_tiles(V)) * TILE
    if kind == 3:
        t = i % n_tiles(V)
        return t * TILE + tile_width(V, t) - 1
    if kind == 4:
        return V - 1
    if kind == 5:
        ps = ref.p[ref.order]  # descending
        last = int(np.searchsorted(-ps, -REL_FLOOR, side="right")) - 1  # last rank with p >= 1e-30
        if i % 3 == 2 and last + 1 < V:
            return int(ref.order[last + 1])  # the first column below 1e-30
        return int(ref.order[max(0, last - i % 3)])
    return None


def row_targets(ref: RowRef, n):
    return [row_target(ref, r) for r in range(n)]


# ------------------------------------------------------------ sliding block
RUNG = 0.5
RUNG_J = tuple(range(-12, 13))
BLOCK_N = 12
RUNG_TOL = 1e-3      # a row whose s_r lies this close to a rung is dropped
MAX_DROP = 0.05      # expected share with rung spacing 0.5: 0.4 %


def sliding_block(V):
    """(a, b, block): a[v] in {0, 1} (fp32), the ladder b (fp32, 0 on the
    block), and the block's columns ascending.

    Block and upper ladder columns alternate over ``key_columns`` (tile 0, a
    middle tile, tiles l / l + 64 / l + 128, the last tile; tile edges and all
    quad phases).  Rungs j >= -2 hold one key column each — top-16 has to reach
    the block from the top rung, so 15 columns above s_r > -1.5 leave it 1 to 10
    of the 16 places — rungs -7 .. -3 three key columns each, and every other
    column sits on rungs -12 .. -8 (thousands of exact ties per rung)."""
    singles = [j for j in RUNG_J if j >= -2][::-1]          # 12 .. -2
    triples = [j for j in (-3, -4, -5, -6, -7) for _ in range(3)]
    keys = key_columns(V, 2 * BLOCK_N + len(singles) + len(triples) - BLOCK_N)
    nreg = len(regions(V))  # a checkerboard over (offset, region): block and ladder columns in every region
    in_block = [(i % nreg + i // nreg) % 2 == 0 for i in range(2 * BLOCK_N)]
    block = sorted(c for c, blk in zip(keys, in_block) if blk)
    ladder = [c for c, blk in zip(keys, in_block) if not blk] + keys[2 * BLOCK_N:]
    assert len(block) == BLOCK_N
    v = np.arange(V)
    b = (RUNG * (-8 - (v * 7 + v // TILE) % 5)).astype(np.float32)
    a = np.zeros(V, dtype=np.float32)
    for c, j in zip(ladder, singles + triples):
        b[c] = RUNG * j
    a[block] = 1.0
    b[block] = 0.0
    return a, b, np.asarray(block)


def sliding_row(a, b, s):
    """fl32(a s + b): s on the block (b = 0 there), b elsewhere (a = 0)."""
    return np.where(a != 0, np.float32(s), b).astype(np.float32)


def near_rung(s):
    return abs(s / RUNG - round(s / RUNG)) * RUNG < RUNG_TOL


# ----------------------------------------------- fp32 emulation of the formula
def _sum_blocked(e, lanes=256):
    """256 strided partial sums, each sequential in fp32, then a pairwise
    combine: the shape of row_stats_kernel's and the tile records' summation."""
    n = e.shape[0]
    pad = np.zeros((-n) % lanes, dtype=np.float32)
    m = np.concatenate([e, pad]).reshape(-1, lanes)
    acc = np.zeros(lanes, dtype=np.float32)
    for row in m:
        acc = (acc + row).astype(np.float32)
    return _sum_pairwise(acc)


def _sum_pairwise(e):
    n = 1
    while n < e.shape[0]:
        n *= 2
    x = np.concatenate([e.astype(np.float32), np.zeros(n - e.shape[0], dtype=np.float32)])
    while x.shape[0] > 1:
        h = x.shape[0] // 2
        x = (x[:h] + x[h:]).astype(np.float32)
    return np.float32(x[0])


def emulate_fp32(row, order="blocked"):
    """exp(x - max) / sum in fp32 with the given summation order: the whole
    probability vector as fp32."""
    row = np.asarray(row, dtype=np.float32)
    e = np.exp((row - row.max()).astype(np.float32)).astype(np.float32)
    s = {"blocked": _sum_blocked, "pairwise": _sum_pairwise}[order](e)
    return (e / s).astype(np.float32)
