"""``prob`` / ``topk`` of the engine on logit rows with known answers.

Every number a caller reads passes through ``row_stats_kernel`` (materialised
logits: f32, x3bf16, ``return_logits=True``, ``d_vocab % 4 != 0``) or through
the fused unembed statistics (``pp_stats_rows`` in the EPI_STATS epilogue +
``stats_merge_kernel``: x2f16, x2f16 on the exact-fp16 binding, bf16).  Random
weights never produce two equal logits, 16 winners inside one tile, a softmax
that overflows when computed naively, or ``d_vocab % 4 != 0``; the rows here do
(tests/stats_cases.py):

* forced rows    W_U = 0, so every logit row is ``b_unembed``, swapped in place
                 per pattern (the engine binds the bias by pointer);
* sliding block  W_U = -2 a e_0 with a in {0, 1}: a block of exactly tied
                 columns at s_r (-2 x row r's first final-LayerNorm coordinate)
                 between the rungs of a ladder, at a different place in
                 different rows;
* chunk offsets  1030 sites with logits (1024-row chunks of run_final) and
                 16390 without (16384-row chunks), targets differing per row.

300 ragged prompts: two 256-row GEMM tiles, both 128-row LDS halves of the
statistics epilogue, a partial row tile.  V = 260 (a last tile of 4 columns),
512, 50304 (197 tiles: lanes of stats_merge_kernel wrap, last tile 128 wide);
509 for row_stats_kernel (check_config accepts it): rows alternate between the
float4 branch with a 1-element tail and the scalar branch.

Bars.  Top-k ids: equal to ``np.lexsort((ids, -values))`` (value descending,
lowest id on ties).  Probabilities against the fp64 softmax of the fp32 row the
kernel reads: |dp| <= 1e-5 max p, and for p >= 1e-30 also
|dp| <= p (max - x_t + 16) 2^-22 (stats_cases.rel_bar; an fp32 evaluation of the
formula stays within 0.21 of it, tests/test_stats_cases.py).  Logits, where
returned, equal the forced row bit for bit.  On the exact-fp16 binding the
logits path subtracts each row's mean (center_rows_kernel), so its reference is
the returned row; the fused path there reads the uncentred row, which the
sliding-block test rebuilds in fp64 as returned + mean (exact outside the block,
within half an ulp of s_r on it).

Measured on an MI355X by this file (printed at its end), worst |dp| / bar over
every case of a path, absolute bar and relative bar:

    fused (pp_stats_rows + stats_merge_kernel)   x2f16            0.023  0.198
                                                 x2f16, exact fp16 0.037  0.198
                                                 bf16             0.023  0.198
    row_stats_kernel                             f32              0.025  0.203
                                                 x3bf16           0.017  0.191
                                                 x2f16 logits     0.025  0.203
                                                 exact fp16 logits 0.035  0.191
                                                 bf16 logits      0.022  0.203

The relative worst is the ``wide`` row's smallest targets (max - x_t near 69),
where the fp32 emulation of the formula gives 0.204: the kernels sit where a
correct fp32 evaluation sits, a fifth of the bar.

The tests bite: three mutants of the engine (not committed) each fail here.
Flipping the tie rule of argmax_merge (``oi > bi``) fails every forced pattern
with ties (zeros, plateau, two_tiers, quantised, spike, offset) on all 13
(path, V), all sliding-block and chunk cases; ``c >= pi`` in the successor rule
of pp_stats_rows fails every pattern at k > 1 on the nine fused (path, V), the
fused sliding-block cases and the 16390-site sweeps; stats_merge without its
rescale (``s = s + os``) fails every pattern but zeros everywhere, and all
sliding-block and chunk cases.
"""
import collections
import random

import numpy as np
import pytest
import torch

import stats_cases as S
import tvr_amd

pytestmark = [pytest.mark.gpu]

N_PROMPTS = 300
NONE = tvr_amd._lib.SITE_NONE
GAIN = -2.0

# (path, V).  x2f16e: x2f16 with fp16-valued weights, i.e. the exact-fp16 binding (wide-tile one-plane GEMM)
FUSED_V = (260, 512, 50304)
FORCED = ([(p, V) for p in ("x2f16", "x2f16e", "bf16") for V in FUSED_V] +
          [("f32", V) for V in (509, 512, 50304)] + [("x3bf16", 512)])
SLIDING = ([(p, V) for p in ("x2f16", "x2f16e", "bf16", "f32") for V in (512, 50304)] + [("x3bf16", 512)])
PLANAR = ("x2f16", "x2f16e", "bf16")

_worst = collections.defaultdict(lambda: [0.0, 0.0])


def _note(kernel, path, ratios):
    w = _worst[(kernel, path)]
    w[0], w[1] = max(w[0], ratios[0]), max(w[1], ratios[1])


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (kernel, path), (ra, rr) in sorted(_worst.items()):
        print(f"\nrow statistics, worst |dp| / bar: {kernel:9s} {path:7s} abs {ra:.4f} rel {rr:.4f}", end="")
    print()


class Ctx:
    """One engine model whose logit rows the test chooses, its prompts, a
    filled trace, and one SITE_NONE site per prompt."""

    def __init__(self, tiny_cfg, path, V, sliding):
        self.path, self.V, self.exact = path, V, path == "x2f16e"
        self.planar = path in PLANAR
        cfg = tiny_cfg.with_(n_layers=1, d_vocab=V)
        w = tvr_amd.weights.synth_engine_weights(cfg, seed=3, device="cuda", std=0.15, fp16=self.exact)
        d = cfg.d_model
        wu = torch.zeros(V, d, device="cuda")
        if sliding:
            self.a, self.b, self.block = S.sliding_block(V)
            # s_r = GAIN * (first coordinate of the final LayerNorm row): a power of two, so every product
            # stays exact; with it s_r spans about -3.4 .. 6.5 (median 2.3) over the 300 prompts and the
            # block meets k = 16 between many different rungs (the bare coordinate: -3.2 .. 1.7, median -1.1,
            # leaves the block out of the top 16 in a third of the rows and gives 7 distinct lists)
            wu[:, 0] = torch.from_numpy(self.a).cuda() * GAIN
        w.w_unembed_t = wu
        w.b_unembed = torch.zeros(V, device="cuda")
        if self.exact:
            assert w.raw16 is not None
            w.raw16_unembed = (wu.half().contiguous(), torch.ones(d, device="cuda"))
        self.model = tvr_amd.Model(cfg, w, device="cuda", gemm="x2f16" if self.exact else path)
        assert self.model.exact16 == self.exact and self.model.gemm == ("x2f16" if self.exact else path)
        rng = random.Random(11)
        self.prompts = [[0] + [rng.randrange(1, V) for _ in range(rng.randrange(1, 5))] for _ in range(N_PROMPTS)]
        assert {len(p) for p in self.prompts} == {2, 3, 4, 5}
        self.ntok = sum(map(len, self.prompts))
        self.trace = self.model.trace(N_PROMPTS, self.ntok)
        self.vecs = torch.zeros(1, d, device="cuda")
        if sliding:
            self.set_bias(self.b)
        self.model.forward_clean(self.prompts, trace=self.trace)
        self.sliding = {}  # sliding block: the per-row references per engine path (sliding_rows)

    def set_bias(self, row):
        """Swap b_unembed in place (the engine reads it through the pointer it was created with)."""
        torch.cuda.synchronize()
        self.model.weights.b_unembed.copy_(torch.from_numpy(np.array(row, dtype=np.float32)))
        torch.cuda.synchronize()

    def kernel(self, logits):
        return "fused" if self.planar and not logits else "row_stats"

    def sites(self, seqs, targets):
        s = tvr_amd.make_sites(len(seqs))
        s["seq"], s["kind"] = seqs, NONE
        s["target"] = [-1 if t is None else t for t in targets]
        return s


_models = {}


@pytest.fixture(scope="module")
def models(tiny_cfg):
    """ctx(path, V, sliding): the model of one (path, V), built on first use and kept for the module."""
    def get(path, V, sliding):
        key = (path, V, sliding)
        if key not in _models:
            _models[key] = Ctx(tiny_cfg, path, V, sliding)
        return _models[key]
    yield get
    for ctx in _models.values():
        del ctx.trace, ctx.model
    _models.clear()
    torch.cuda.empty_cache()


def _id(p):
    return f"{p[0]}-{p[1]}"


def check(ctx, out, rows: S.RowSet, k, logits, what):
    """prob and top-k of one engine call against the rows' references."""
    if k:
        top = out["topk"].cpu().numpy().astype(np.int64)
        assert top.shape == (len(rows.tg), k)
        bad = np.nonzero((top != rows.top[:, :k]).any(axis=1))[0]
        assert bad.size == 0, (what, ctx.path, ctx.V, k, f"{bad.size} rows differ, first {bad[0]}:",
                               top[bad[0]].tolist(), rows.top[bad[0], :k].tolist())
    ratios = rows.prob_ratios(out["prob"].cpu().numpy())
    _note(ctx.kernel(logits), ctx.path, ratios)
    assert ratios[0] <= 1.0 and ratios[1] <= 1.0, (what, ctx.path, ctx.V, k, "|dp| / (abs bar, rel bar)", ratios)
    return ratios


# ---------------------------------------------------------------- forced rows
@pytest.mark.parametrize("pattern", list(S.PATTERNS))
@pytest.mark.parametrize("case", FORCED, ids=_id)
def test_forced_rows(models, case, pattern):
    """Every logit row is the pattern: forward_clean without and with logits,
    SITE_NONE sweeps on a filled trace and with the clean forward deferred into
    the sweep, k = 1, 2, 5, 16, every row against the reference."""
    ctx = models(*case, sliding=False)
    m, V = ctx.model, ctx.V
    ref = S.pattern_ref(pattern, V)
    ctx.set_bias(ref.row)
    targets = S.row_targets(ref, N_PROMPTS)
    rows = S.RowSet([(ref, t) for t in targets])
    sites = ctx.sites(np.arange(N_PROMPTS), targets)
    bias_bits = m.weights.b_unembed.view(torch.int32)
    worst = [0.0, 0.0]

    def run(out, k, logits, what, rws=rows):
        r = check(ctx, out, rws, k, logits, what)
        worst[0], worst[1] = max(worst[0], r[0]), max(worst[1], r[1])

    lrows, centred = rows, None
    for k in S.TOPK:
        run(m.forward_clean(ctx.prompts, targets=targets, topk=k), k, False, "forward_clean")
        run(m.patch_sweep(ctx.trace, sites, ctx.vecs, topk=k), k, False, "patch_sweep")
        # the clean forward deferred into the sweep, with another k than the sweep's own
        k2 = S.TOPK[len(S.TOPK) - 1 - S.TOPK.index(k)]
        trace = m.trace(N_PROMPTS, ctx.ntok)
        clean = m.forward_clean(ctx.prompts, targets=targets, topk=k, trace=trace, defer=True)
        swept = m.patch_sweep(trace, sites, ctx.vecs, topk=k2)
        run(clean, k, False, "deferred forward_clean")
        run(swept, k2, False, "patch_sweep after a deferred forward")
        for what, out in (("forward_clean, logits", m.forward_clean(ctx.prompts, targets=targets, topk=k,
                                                                    return_logits=True)),
                          ("patch_sweep, logits", m.patch_sweep(ctx.trace, sites, ctx.vecs, topk=k,
                                                                return_logits=True))):
            lg = out["logits"]
            assert lg.shape == (N_PROMPTS, V)
            if not ctx.exact:
                assert bool((lg.view(torch.int32) == bias_bits).all()), (what, "logits != b_unembed bit for bit")
            else:
                # centred by center_rows_kernel: every row (of every call) the same, row - row[0] = b - b[0] up
                # to the rounding of x - mean; the reference is the returned row
                if centred is None:
                    centred = lg[0].clone()
                    lg0 = centred.cpu().numpy()
                    diff = (lg0.astype(np.float64) - lg0[0]) - (ref.row.astype(np.float64) - ref.row[0])
                    assert np.abs(diff).max() <= 2.0 ** -23 * np.abs(lg0).max()
                    cref = S.RowRef(lg0)
                    lrows = S.RowSet([(cref, t) for t in targets])
                assert bool((lg.view(torch.int32) == centred.view(torch.int32)).all()), (what, "centred rows differ")
            run(out, k, True, what, lrows)
    print(f"{ctx.path} V={V} {pattern}: worst |dp| / abs bar {worst[0]:.4f}, / rel bar {worst[1]:.4f}")


# -------------------------------------------------------------- sliding block
class Sliding:
    """The sliding-block model's rows as one engine path returns them: the kept
    rows (s_r not within 1e-3 of a rung), per kept row its reference for the
    logits path and for the no-logits path, and its target."""


def sliding_rows(ctx, via):
    """``via`` "forward": forward_clean(return_logits=True) (the trimmed last
    layer); "sweep": a SITE_NONE sweep with logits over the filled trace (the
    full last layer: s_r may differ from the forward's in the last bits).  The
    returned logits equal the expected fp32 rows fl32(a s_r + b) bit for bit,
    s_r read from the block's first column.  Once per (model, via)."""
    if via in ctx.sliding:
        return ctx.sliding[via]
    a, b, block, V = ctx.a, ctx.b, ctx.block, ctx.V
    if via == "forward":
        lg = ctx.model.forward_clean(ctx.prompts, return_logits=True)["logits"]
    else:
        lg = ctx.model.patch_sweep(ctx.trace, ctx.sites(np.arange(N_PROMPTS), [None] * N_PROMPTS), ctx.vecs,
                                   want_prob=False, return_logits=True)["logits"]
    lg = lg.cpu().numpy()
    probe = lg[:, block[0]]
    if not ctx.exact:
        s = probe.astype(np.float64)
        expected = np.where(a != 0, probe[:, None], b[None, :]).astype(np.float32)
        assert np.array_equal(lg.view(np.int32), expected.view(np.int32)), "logits != fl32(a s_r + b)"
    else:
        # centred rows: the rung-0 ladder column (a = 0, b = 0) holds -mean exactly
        zero = int(np.nonzero((a == 0) & (b == 0))[0][0])
        mean = -lg[:, zero]
        expected = np.where(a != 0, probe[:, None], (b[None, :] - mean[:, None]).astype(np.float32))
        assert np.array_equal(lg.view(np.int32), expected.astype(np.float32).view(np.int32))
        s = probe.astype(np.float64) + mean.astype(np.float64)  # s_r to half an ulp of the centred value
    keep = [r for r in range(N_PROMPTS) if not S.near_rung(float(s[r]))]
    assert len(keep) >= (1.0 - S.MAX_DROP) * N_PROMPTS, f"{N_PROMPTS - len(keep)} rows within 1e-3 of a rung"
    items_l, items_f = [], []
    for r in keep:
        ref = S.RowRef(lg[r])  # the row row_stats_kernel reads
        t = S.row_target(ref, r)
        items_l.append((ref, t))
        # the row the fused epilogue reads: the same, but uncentred on the exact-fp16 binding
        items_f.append((S.RowRef(np.where(a != 0, s[r], b.astype(np.float64))), t) if ctx.exact else (ref, t))
    q = np.quantile(s, [0, 0.05, 0.5, 0.95, 1])
    print(f"{ctx.path} V={V} ({via}): s_r min / 5 % / median / 95 % / max = " +
          " / ".join(f"{x:.2f}" for x in q) + f", {N_PROMPTS - len(keep)} rows dropped")
    out = Sliding()
    out.keep = np.asarray(keep)
    out.refs_l = [r for r, _ in items_l] if V <= 512 else None  # (the chunk test draws other targets)
    out.refs_f = [r for r, _ in items_f] if V <= 512 else None
    out.rows_l, out.rows_f = S.RowSet(items_l), S.RowSet(items_f)
    ctx.sliding[via] = out
    return out


@pytest.mark.parametrize("case", SLIDING, ids=_id)
def test_sliding_block(models, case):
    """A block of 12 exactly tied columns at s_r slides along a ladder of tied
    rungs from row to row: logits bit for bit, prob / top-k of the no-logits
    and of the logits path row by row, and at least 10 distinct top-16 lists."""
    ctx = models(*case, sliding=True)
    m = ctx.model
    sl = sliding_rows(ctx, "forward")
    rows_l, rows_f = sl.rows_l, sl.rows_f
    assert np.array_equal(rows_l.top, rows_f.top)
    lists = {tuple(t) for t in rows_l.top.tolist()}
    n_block = np.isin(rows_l.top, ctx.block).sum(axis=1)
    print(f"{ctx.path} V={ctx.V}: {len(lists)} distinct top-16 lists, block columns in the top 16: "
          f"{sorted(collections.Counter(n_block.tolist()).items())}")
    assert len(lists) >= 10
    prompts = [ctx.prompts[r] for r in sl.keep]
    for k in S.TOPK:
        check(ctx, m.forward_clean(prompts, targets=rows_f.targets, topk=k), rows_f, k, False, "forward_clean")
        check(ctx, m.forward_clean(prompts, targets=rows_l.targets, topk=k, return_logits=True), rows_l, k, True,
              "forward_clean, logits")


@pytest.mark.parametrize("path, n_sites, logits", [("f32", 1030, True), ("x2f16", 1030, True),
                                                   ("x2f16", 16390, False), ("bf16", 16390, False)])
def test_chunk_offsets(models, path, n_sites, logits):
    """More rows than one chunk of run_final (1024 with logits, 16384 on the
    fused path): targets, prob and top-k rows of the later chunks land at their
    own offsets.  Sliding-block model at V = 512, targets differing per row;
    the reference rows are those of a 300-site sweep with logits over the same
    trace (a row's only non-zero product is a s_r: the same in every launch)."""
    ctx = models(path, 512, sliding=True)
    sl = sliding_rows(ctx, "sweep")
    refs = sl.refs_l if logits else sl.refs_f
    idx = (np.arange(n_sites) * 7) % len(sl.keep)
    rows = S.RowSet([(refs[j], S.row_target(refs[j], i)) for i, j in enumerate(idx)])
    chunk = 1024 if logits else 16384  # the later chunk's targets are not the first chunk's again
    assert len(set(rows.targets)) >= 16 and rows.targets[chunk:] != rows.targets[:n_sites - chunk]
    out = ctx.model.patch_sweep(ctx.trace, ctx.sites(sl.keep[idx], rows.targets), ctx.vecs, topk=16,
                                return_logits=logits)
    check(ctx, out, rows, 16, logits, f"patch_sweep of {n_sites} sites")
    if logits:
        lg = out["logits"].cpu().numpy()
        want = np.stack([refs[j].row for j in idx])
        assert np.array_equal(lg.view(np.int32), want.view(np.int32))
