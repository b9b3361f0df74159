"""The site-entry and head-set patch kernels on the GPU, alone: ``entry_kernel``,
``entry_replace_mfma_kernel<16|64|80|128>`` and ``headset_patch_kernel<V4>``
through the test primitives ``tvr_site_entry`` (the sweep's own planner and entry
launches on caller-made rows) and ``tvr_headset_apply`` (one apply_headset
launch), against the fp64 reference and the exact expectations of
tests/entry_cases.py.

One three-layer model per (d_head, n_heads) of attention_cases.MODELS (d = 64,
256, 320, 256, 96, 384: a wave past d at 96, a partial second 256-column block
at 320 and 384, every DH instantiation), its w2 overwritten by the case's W.
Every call (``entry``) reads resid, z and vectors that are followed by NaN rows
and writes into a NaN-filled buffer with guard rows on both sides: a NaN in a
site's rows means a row past the end was read, a changed guard or a changed row
past the sites' rows means a store went astray.  REPLACE_HEAD rows are graded at
entry_cases.bar (4 x the worse of two fp32 restatements, floored at 4 x 2^-24 x
the largest sum of |terms|); select and integer cases, the z = 0 rows, kinds 0,
2, 3, 6 and the head-set sites' copies are compared bit for bit.  The forced
VALU branch (TVR_ENTRY_FORCE_VALU: entry_kernel's own REPLACE_HEAD code, which no
sweep reaches for the supported head sizes) runs the same cases at the same bar,
and T = 127 / 128 / 129 / 145 for its LDS chunk of 128 positions.

Head sets: every activation format, n_rows 1 / 7 / 8 / 9 / 17, lists of 1, 2 and
all heads in descending order, an empty range, two items sharing a vector,
vectors 16- and 4-byte aligned; a2 and resid whole buffers compared byte for
byte with entry_cases.headset_expect, rows that no item names included, and
the interleaved x2f16 result against the planar one permuted.

Not reachable through the planner, hence not covered: a patched position of
kinds 3 / 6 anywhere but the first row of its entry (the planner starts the
entry AT the patched position), and a REPLACE_HEAD site with vectors that are
not 16-byte aligned (refused by the primitive: the kernels load 16 bytes).

Measured on an MI355X by this file (worst err / bar, printed at its end), at
d_head 16 / 64 / 80 / 128:
  MFMA, T = 1 .. 33, six operand kinds   0.238 0.208 0.191 0.194
  MFMA, groups and mixed kinds           0.205 0.161 0.157 0.212
  MFMA, shared-prefix followers          0.225 0.143 0.172 0.156
  MFMA, T = 127 .. 145                   0.299   -   0.188   -
  forced VALU, T = 1 .. 33               0.215   -   0.284   -
  forced VALU, followers                 0.281   -   0.271   -
  forced VALU, T = 127 .. 145            0.259   -   0.353   -
every exact case bit for bit, every head-set buffer byte for byte.  The whole
file (98 tests) runs in about 2 s.
"""
import collections
import ctypes
import functools
import gc
import time

import numpy as np
import pytest
import torch

import attention_cases as A
import entry_cases as E
import tvr_amd
from tvr_amd import _lib as L

pytestmark = [pytest.mark.gpu]

G = 2                  # guard rows before and after every output
NAN_BITS = 0x7FC00000  # torch.full(nan)
N_LAYERS = 3
N_CTX = 160
MODEL_IDS = [f"dh{dh}h{h}" for dh, h in A.MODELS]
VALU_MODELS = ((16, 4), (80, 4))
LENS = (1, 15, 16, 17, 33)
FMT = {"f32": 0, "x2f16": L.GEMM_MODES["x2f16"], "x2f16i": L.ACT_X2F16_IL, "bf16": L.GEMM_MODES["bf16"]}

_worst = collections.defaultdict(float)


def note(form, err, bar):
    _worst[form] = max(_worst[form], err / bar)
    return err <= bar


@pytest.fixture(scope="module", autouse=True)
def _module():
    t0 = time.time()
    yield
    for form, r in sorted(_worst.items()):
        print(f"\nsite entry, worst err / bar: {form:44s} {r:.3f}", end="")
    print(f"\nsite entry tests: {time.time() - t0:.1f} s from the first test to the last")
    _ctx.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


class Ctx:
    def __init__(self, DH, H):
        self.DH, self.H, self.d, self.K2 = DH, H, DH * H, DH * H + E.D_MLP
        cfg = tvr_amd.config.PythiaConfig(N_LAYERS, self.d, H, E.D_MLP, 64, n_ctx=N_CTX, name=f"entry-{DH}x{H}")
        self.w = tvr_amd.weights.synth_engine_weights(cfg, seed=1, device="cuda", std=0.2)
        self.model = tvr_amd.Model(cfg, self.w, tokenizer=tvr_amd.tokenizer.SyntheticTokenizer(512), device="cuda", gemm="f32")
        self.lib, self.h = self.model._lib, self.model._h
        self.bound = None

    def stream(self):
        return self.model._stream()

    def bind(self, case):
        """The case's W as the model's w2 (the engine reads the caller's tensors) and its rows on the device."""
        if self.bound is not case:
            for l, lay in enumerate(self.w.layers):
                lay.w2.copy_(torch.from_numpy(case.W[l]))
            if not hasattr(case, "dev"):
                case.cap = case.tokens + 2  # two NaN rows behind every layer's rows
                case.dev = tuple(nan_padded(a, case.cap) for a in (case.resid, case.z))
                nv, d = case.vectors.shape
                v = torch.full(((nv + 1) * d + 4,), float("nan"), dtype=torch.float32, device="cuda")
                v4 = v.clone()
                v[:nv * d] = torch.from_numpy(case.vectors).reshape(-1)
                v4[1:1 + nv * d] = torch.from_numpy(case.vectors).reshape(-1)
                case.vec = (v, v4)
            torch.cuda.synchronize()
            self.bound = case


def nan_padded(a, cap):
    """a [n][rows][d] on the device as [n][cap][d], the rows beyond a's NaN."""
    t = torch.full((a.shape[0], cap, a.shape[2]), float("nan"), dtype=torch.float32, device="cuda")
    t[:, :a.shape[1]] = torch.from_numpy(a)
    return t


@functools.lru_cache(maxsize=None)  # one model per (d_head, n_heads) for the module: _module clears it
def _ctx(model):
    return Ctx(*model)


@pytest.fixture(params=A.MODELS, ids=MODEL_IDS)
def ctx(request):
    return _ctx(request.param)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class Guarded:
    """A NaN-filled [G + rows + G][d] buffer; the middle is the output."""

    def __init__(self, rows, d):
        self.rows, self.d = rows, d
        self.t = torch.full((rows + 2 * G, d), float("nan"), dtype=torch.float32, device="cuda")
        self.ptr = self.t.data_ptr() + 4 * G * d
        assert self.ptr % 16 == 0

    def read(self, used, what):
        h = self.t.cpu().numpy()
        b = h.view(np.int32)
        assert (b[:G] == NAN_BITS).all() and (b[G + used:] == NAN_BITS).all(), f"{what}: written outside the sites' rows"
        return h[G:G + used].copy()

    def untouched(self):
        return (self.t.cpu().numpy().view(np.int32) == NAN_BITS).all()


def c_sites(sites):
    return (L.CSite * len(sites))(*[L.CSite(*s) for s in sites])


def entry_call(ctx, case, sites, out, tokens=None, sets=None, flags=0, vec_shift=0, n_vectors=None, cap=None,
               resid=None, z=None, out_rows=None, model="h", lens=None):
    """The raw call: (rc, row0, rows, p0)."""
    n = len(sites)
    lens = case.seq_lens if lens is None else lens
    c_lens = (ctypes.c_int32 * len(lens))(*lens)
    c_tok = None if tokens is None else (ctypes.c_int32 * len(tokens))(*tokens)
    set_off = patches = None
    if sets is not None:
        flat = [p for s in sets for p in s]
        set_off = (ctypes.c_int32 * (n + 1))(*np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(int))
        patches = (L.CHeadPatch * max(len(flat), 1))(*[L.CHeadPatch(*p) for p in flat])
    rep = [(ctypes.c_int32 * n)() for _ in range(3)]
    vec = case.vec[vec_shift].data_ptr() + 4 * vec_shift
    rc = ctx.lib.tvr_site_entry(ctx.h if model == "h" else model, c_lens, len(lens), c_tok, case.cap if cap is None else cap,
                                case.dev[0].data_ptr() if resid is None else resid,
                                case.dev[1].data_ptr() if z is None else z, c_sites(sites), n, set_off, patches, vec,
                                case.vectors.shape[0] if n_vectors is None else n_vectors, flags, out.ptr,
                                out.rows if out_rows is None else out_rows, rep[0], rep[1], rep[2], ctx.stream())
    return rc, list(rep[0]), list(rep[1]), list(rep[2])


def entry(ctx, case, sites, **kw):
    """One tvr_site_entry call: [(p0, rows [n][d])] per site, guards checked."""
    ctx.bind(case)
    out = Guarded(sum(case.seq_lens[s.seq] for s in sites), case.d)
    rc, row0, rows, p0 = entry_call(ctx, case, sites, out, **kw)
    L.check(rc, "tvr_site_entry")
    used = sum(rows)
    got = out.read(used, "out")
    # the sites' rows tile [0, used) without overlap
    assert sorted(zip(row0, rows)) == [(a, b) for a, b in zip(np.concatenate([[0], np.cumsum(sorted_rows(row0, rows))[:-1]]),
                                                              sorted_rows(row0, rows))]
    res = [(p0[i], got[row0[i]:row0[i] + rows[i]]) for i in range(len(sites))]
    for i, (p, r) in enumerate(res):
        assert not np.isnan(r).any(), f"NaN in the rows of site {i}: a row past the end was read"
    return res


def sorted_rows(row0, rows):
    return [r for _, r in sorted(zip(row0, rows))]


def heads_of(H):
    return (0, H // 2, H - 1)


def make(kind, ctx, lens=LENS, seed=0):
    return E.make(kind, ctx.DH, ctx.H, lens, L=N_LAYERS, nv=ctx.H if kind == "cancel" else 3, seed=seed)


def replace_sites(ctx, case, layers=range(N_LAYERS), seqs=None):
    """REPLACE_HEAD at every given layer of every sequence, the head first / middle / last in turn."""
    hs = heads_of(ctx.H)
    seqs = range(len(case.seq_lens)) if seqs is None else seqs
    out = []
    for s in seqs:
        for l in layers:
            h = hs[(s + l) % 3]
            out.append(E.Site(s, E.REPLACE_HEAD, layer=l, head=h, vec=h if case.kind == "cancel" else (s + l) % 3))
    return out


def check_replace(ctx, case, sites, res, form):
    """The REPLACE_HEAD sites of one call against fp64 at the case's bar, the exact kinds and rows bit for bit."""
    refs = [E.replace_head_rows(case, s) for s in sites]
    bar = E.bar(case, sites, refs)[0]
    err = 0.0
    for s, ref, (p0, got) in zip(sites, refs, res):
        T = case.seq_lens[s.seq]
        assert got.shape[0] == T - p0
        err = max(err, E.max_err(got, ref[p0:]))
        if case.kind in ("select", "integer"):
            assert (bits(got) == bits(E.replace_head_exact(case, s)[p0:])).all(), (form, case.kind, s)
        if case.kind == "zero":
            rows = E.zero_positions(T)[p0:]
            assert (bits(got[rows]) == bits(E.replace_head_exact(case, s)[p0:][rows])).all(), (form, s)
    ok = note(f"{form} d_head {ctx.DH:3d}", err, bar)
    print(f"site entry {form} ({ctx.DH}, {ctx.H}) {case.kind:7s}: err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
    assert ok, (form, case.kind, err, bar)


# ------------------------------------------------------------------------------ 1: the MFMA entry
@pytest.mark.parametrize("kind", E.KINDS)
def test_mfma_entry_against_fp64(ctx, kind):
    """T = 1 / 15 / 16 / 17 / 33, sites at every layer (the last enters at L: the final norm's input), head
    first / middle / last; where the model is one of VALU_MODELS, the forced VALU branch on the same cases."""
    case = make(kind, ctx)
    sites = replace_sites(ctx, case)
    res = entry(ctx, case, sites)
    assert all(p0 == 0 for p0, _ in res)
    check_replace(ctx, case, sites, res, "mfma")
    again = entry(ctx, case, sites)
    assert all((bits(a[1]) == bits(b[1])).all() for a, b in zip(res, again)), "a second run gives other bits"
    if (ctx.DH, ctx.H) in VALU_MODELS:
        check_replace(ctx, case, sites, entry(ctx, case, sites, flags=L.ENTRY_FORCE_VALU), "valu")


# ------------------------------------------------------------------------------ 2: grouping
GROUP_LENS = (33, 1, 17, 16, 15, 2, 31, 18, 7)


def test_groups_give_every_site_the_bits_it_has_alone(ctx):
    """1, 4, 5 and 9 sites of one head (groups of 1 / 4 / 3 + 2 / 3 + 3 + 3) on prompts of different lengths,
    then with other heads and kinds 0 / 2 / 3 / 6 entering at the same layers (both launches run)."""
    case = make("random", ctx, GROUP_LENS, seed=4)
    h = ctx.H // 2
    one = [E.Site(s, E.REPLACE_HEAD, layer=1, head=h, vec=s % 3) for s in range(9)]
    alone = [entry(ctx, case, [s])[0][1] for s in one]
    ref_sites, ref_res = [], []
    for n in (1, 4, 5, 9):
        res = entry(ctx, case, one[:n])
        for i in range(n):
            assert (bits(res[i][1]) == bits(alone[i])).all(), (n, i)
        ref_sites, ref_res = one[:n], res
    check_replace(ctx, case, ref_sites, ref_res, "mfma groups")
    # layer 1's entry (2) also takes two other heads, a kind 2 of layer 1 and kinds 3 / 6 of layer 2;
    # the last entry layer a REPLACE_HEAD of layer 2 next to NONE
    T0 = GROUP_LENS[0]
    others = [E.Site(0, E.REPLACE_HEAD, layer=1, head=0, vec=1), E.Site(2, E.REPLACE_HEAD, layer=1, head=ctx.H - 1, vec=2),
              E.Site(6, E.ADD_LAST, layer=1, vec=0), E.Site(0, E.SET_POS, layer=2, pos=T0 - 9, src_seq=6, src_pos=30),
              E.Site(2, E.SET_VEC, layer=2, pos=3, vec=2), E.Site(3, E.REPLACE_HEAD, layer=2, head=h, vec=0),
              E.Site(4, E.NONE)]
    mixed = one + others
    res = entry(ctx, case, mixed)
    for i in range(9):
        assert (bits(res[i][1]) == bits(alone[i])).all(), i
    for s, (p0, got) in zip(others, res[9:]):
        if s.kind == E.REPLACE_HEAD:
            assert (bits(got) == bits(entry(ctx, case, [s])[0][1])).all(), s
        else:
            want_p0, want = E.site_rows(case, s)
            assert p0 == want_p0 and (bits(got) == bits(want)).all(), s
    rh = [(s, r) for s, r in zip(mixed, res) if s.kind == E.REPLACE_HEAD]
    check_replace(ctx, case, [s for s, _ in rh], [r for _, r in rh], "mfma groups")


# ------------------------------------------------------------------------------ 3: shared prefixes
def test_shared_prefix_followers(ctx):
    """With token ids the followers enter at p0 > 0; their rows are the reference's for those positions and,
    bit for bit, the rows of the same call without ids."""
    lens = (33, 17, 16, 20, 5)
    case = make("random", ctx, lens, seed=6)
    base = list(range(100, 133))
    toks = [base, base[:17], base[:5] + [7] * 11, [9] + base[1:20], base[:5]]
    want_p0 = [0, 16, 5, 0, 4]  # (capped at T - 1; another first token: no leader)
    flat = [t for seq in toks for t in seq]
    for layer in (0, N_LAYERS - 1):
        sites = [E.Site(s, E.REPLACE_HEAD, layer=layer, head=ctx.H - 1, vec=1) for s in range(5)]
        res = entry(ctx, case, sites, tokens=flat)
        assert [p0 for p0, _ in res] == want_p0
        check_replace(ctx, case, sites, res, "mfma followers")
        plain = entry(ctx, case, sites)
        for (p0, got), (q0, full) in zip(res, plain):
            assert q0 == 0 and (bits(got) == bits(full[p0:])).all()
    if (ctx.DH, ctx.H) in VALU_MODELS:
        res = entry(ctx, case, sites, tokens=flat, flags=L.ENTRY_FORCE_VALU)
        assert [p0 for p0, _ in res] == want_p0
        check_replace(ctx, case, sites, res, "valu followers")


# ------------------------------------------------------------------------------ 4: entry_kernel's copies
@pytest.mark.parametrize("vec_shift", (0, 1), ids=("vectors16", "vectors4"))
def test_entry_kernel_copy_kinds_bitwise(ctx, vec_shift):
    """Kinds 0, 2, 3, 6 and the head-set sites' copies: n = 1 / 7 / 8 / 9 / 17 rows (one batch of 8, its edges,
    a third batch), the source row in the site's own and in another sequence, vectors at a 16-byte and at a
    4-byte aligned base."""
    case = make("random", ctx, (33, 17, 9), seed=8)
    sites, sets = [], []
    for i, n in enumerate((1, 7, 8, 9, 17)):
        sites.append(E.Site(0, E.SET_POS, layer=i % N_LAYERS, pos=33 - n, src_seq=0 if i % 2 else 1, src_pos=(5 * i) % 17))
        sites.append(E.Site(0, E.SET_VEC, layer=(i + 1) % N_LAYERS, pos=33 - n, vec=i % 3))
        if n <= 17:
            sites.append(E.Site(1, E.SET_VEC, layer=(i + 2) % N_LAYERS, pos=17 - n, vec=(i + 1) % 3))
    for s in range(3):
        sites.append(E.Site(s, E.NONE))
        sites += [E.Site(s, E.ADD_LAST, layer=l, vec=(s + l) % 3) for l in range(N_LAYERS)]
    sets = [()] * len(sites)
    # head-set sites enter as copies of their clean rows at their lowest patched layer; an empty set is NONE
    H = ctx.H
    sites += [E.Site(0, E.SET_ALLPOS), E.Site(1, E.SET_ALLPOS), E.Site(2, E.SET_LASTPOS), E.Site(2, E.SET_ALLPOS)]
    sets += [((2, 0, 1), (1, H - 1, 0)), ((0, H // 2, 2),), ((2, 0, 0), (2, H - 1, 1)), ()]
    res = entry(ctx, case, sites, sets=sets, vec_shift=vec_shift)
    for s, ps, (p0, got) in zip(sites, sets, res):
        want_p0, want = E.site_rows(case, s, ps)
        assert p0 == want_p0 and got.shape == want.shape, (s, p0, want_p0)
        assert (bits(got) == bits(want)).all(), s
    if (ctx.DH, ctx.H) in VALU_MODELS:  # the switch leaves the other kinds' branch as it is
        forced = entry(ctx, case, sites, sets=sets, vec_shift=vec_shift, flags=L.ENTRY_FORCE_VALU)
        assert all((bits(a[1]) == bits(b[1])).all() for a, b in zip(res, forced))


# ------------------------------------------------------------------------------ 5: the forced VALU branch
@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("model", VALU_MODELS, ids=[f"dh{dh}h{h}" for dh, h in VALU_MODELS])
def test_forced_valu_branch_at_the_lds_chunk_edge(model, kind):
    """T = 127 / 128 / 129 / 145: one LDS chunk of 128 positions short of full, full, one position into the
    second, and a second chunk whose last group of 16 positions holds one; next to kinds 0 and 2."""
    ctx = _ctx(model)
    case = make(kind, ctx, (127, 128, 129, 145), seed=2)
    sites = replace_sites(ctx, case, layers=(0,), seqs=(0, 1)) + replace_sites(ctx, case, layers=(1,), seqs=(2,)) + \
        replace_sites(ctx, case, seqs=(3,))
    tail = [E.Site(1, E.NONE), E.Site(2, E.ADD_LAST, layer=0, vec=1)]
    res = entry(ctx, case, sites + tail, flags=L.ENTRY_FORCE_VALU)
    check_replace(ctx, case, sites, res[:len(sites)], "valu chunks")
    for s, (p0, got) in zip(tail, res[len(sites):]):
        assert (bits(got) == bits(E.site_rows(case, s)[1])).all()
    if kind in ("random", "select"):  # the MFMA kernel's ninth and tenth position tiles
        check_replace(ctx, case, sites, entry(ctx, case, sites), "mfma long")


# ------------------------------------------------------------------------------ 6: head sets
HS_ROWS = (1, 7, 8, 9, 17)


def hs_layout(H):
    """Items (row0, n_rows, first_patch, n_patches) with one free row before, between and after them, and
    the flat (head, vec) list: lists of 1, 2 and all heads (descending), an empty range, a shared vector."""
    lists = [[(H - 1, 0)], [(H - 1, 1), (0, 2)], [(h, h % 3) for h in range(H - 1, -1, -1)], [(H // 2, 1)],
             [(0, 3), (H - 1, 0)], []]
    rows = HS_ROWS + (3,)
    items, patches, at = [], [], 1
    for n, ps in zip(rows, lists):
        items.append((at, n, len(patches), len(ps)))
        patches += ps
        at += n + 1
    return items, patches, at


def hs_buffers(fmt, ctx, rows, items, seed=0):
    rng = np.random.default_rng([seed, ctx.DH, ctx.H, E.HS_FORMATS.index(fmt)])
    a2 = np.full((rows, ctx.K2), NAN_BITS, dtype=np.int32).view(np.uint8).reshape(rows, 4 * ctx.K2).copy()
    resid = np.full((rows, ctx.d), np.nan, dtype=np.float32)
    for row0, n, _, _ in items:
        a2[row0:row0 + n] = rng.integers(1, 256, size=(n, 4 * ctx.K2), dtype=np.uint8)  # no zero byte: a zeroed one shows
        resid[row0:row0 + n] = rng.standard_normal((n, ctx.d)).astype(np.float32)
    vectors = rng.standard_normal((4, ctx.d)).astype(np.float32)
    return a2, resid, vectors


def headset_call(ctx, fmt, a2, resid, vectors, items, patches, vec_shift=0, model="h", over=None):
    """(rc, a2 bytes, resid) after one tvr_headset_apply launch; G guard rows around both buffers.  over: raw
    arguments by name in place of the ones built here (a callable: applied to the one built here)."""
    rows = a2.shape[0]
    da2 = torch.full((rows + 2 * G, ctx.K2), float("nan"), dtype=torch.float32, device="cuda")
    dres = torch.full((rows + 2 * G, ctx.d), float("nan"), dtype=torch.float32, device="cuda")
    da2[G:G + rows] = torch.from_numpy(a2.view(np.float32).reshape(rows, ctx.K2).copy()).view(torch.int32).cuda().view(torch.float32)
    dres[G:G + rows] = torch.from_numpy(resid)
    dv = torch.full((vectors.size + 4 + ctx.d,), float("nan"), dtype=torch.float32, device="cuda")
    dv[vec_shift:vec_shift + vectors.size] = torch.from_numpy(vectors).reshape(-1)
    c_items = (L.CHeadsetItem * max(len(items), 1))(*[L.CHeadsetItem(*i) for i in items])
    c_patches = (L.CHeadsetPatch * max(len(patches), 1))(*[L.CHeadsetPatch(*p) for p in patches])
    args = dict(fmt=FMT[fmt], items=c_items, n_items=len(items), patches=c_patches, n_patches=len(patches),
                vectors=dv.data_ptr() + 4 * vec_shift, n_vectors=vectors.shape[0], a2=da2.data_ptr() + 16 * G * ctx.K2 // 4,
                resid=dres.data_ptr() + 4 * G * ctx.d, rows=rows)
    for k, v in (over or {}).items():
        args[k] = v(args[k]) if callable(v) else v
    torch.cuda.synchronize()
    rc = ctx.lib.tvr_headset_apply(ctx.h if model == "h" else model, args["fmt"], args["items"], args["n_items"],
                                   args["patches"], args["n_patches"], args["vectors"], args["n_vectors"], args["a2"],
                                   args["resid"], args["rows"], ctx.stream())
    torch.cuda.synchronize()
    ha2 = da2.view(torch.int32).cpu().numpy()
    hres = dres.cpu().numpy()
    for h in (ha2, hres.view(np.int32)):
        assert (h[:G] == NAN_BITS).all() and (h[G + rows:] == NAN_BITS).all(), "written outside the buffer's rows"
    return rc, ha2[G:G + rows].view(np.uint8).reshape(rows, 4 * ctx.K2).copy(), hres[G:G + rows].copy()


def deinterleave(a2, K2):
    """Interleaved halves [rows][K2 / 32][2][32] as planar [rows][2][K2] (tests/test_gpu_act_layout.py)."""
    return np.ascontiguousarray(a2.view(np.uint16).reshape(-1, K2 // 32, 2, 32).transpose(0, 2, 1, 3).reshape(-1, 2 * K2))


@pytest.mark.parametrize("fmt", E.HS_FORMATS)
def test_headset_patch_bytes_and_bits(ctx, fmt):
    items, patches, rows = hs_layout(ctx.H)
    a2, resid, vectors = hs_buffers(fmt, ctx, rows, items)
    want_a2, want_r = E.headset_expect(fmt, ctx.DH, ctx.K2, a2, resid, vectors, items, patches)
    empty = items[-1]
    assert empty[3] == 0
    for vec_shift in (0, 1):  # the float4 and the element-wise variant
        rc, got_a2, got_r = headset_call(ctx, fmt, a2, resid, vectors, items, patches, vec_shift)
        L.check(rc, "tvr_headset_apply")
        assert (got_a2 == want_a2).all(), (fmt, vec_shift, np.argwhere(got_a2 != want_a2)[:4])
        assert (got_r.view(np.int32) == want_r.view(np.int32)).all(), (fmt, vec_shift)
        # the empty range: bit-identical to the inputs (and so are the rows that no item names: NaN sentinels)
        assert (got_a2[empty[0]:empty[0] + empty[1]] == a2[empty[0]:empty[0] + empty[1]]).all()
        assert (bits(got_r[empty[0]:empty[0] + empty[1]]) == bits(resid[empty[0]:empty[0] + empty[1]])).all()
        if fmt == "x2f16i":  # the same logical planes in the planar layout give the same result, permuted
            rc, pl_a2, pl_r = headset_call(ctx, "x2f16", deinterleave(a2, ctx.K2).view(np.uint8), resid, vectors, items,
                                           patches, vec_shift)
            L.check(rc, "tvr_headset_apply")
            assert (deinterleave(got_a2, ctx.K2) == pl_a2.view(np.uint16)).all()
            assert (bits(pl_r) == bits(got_r)).all()


# ------------------------------------------------------------------------------ 7: refusals
def test_invalid_site_entry_arguments_launch_nothing():
    ctx = _ctx(A.MODELS[0])
    case = make("random", ctx)
    ctx.bind(case)
    ok = [E.Site(4, E.REPLACE_HEAD, layer=1, head=1, vec=0), E.Site(2, E.SET_VEC, layer=0, pos=3, vec=1)]
    out = Guarded(64, case.d)
    resid, z = case.dev[0].data_ptr(), case.dev[1].data_ptr()

    def refused(message, sites=ok, **kw):
        rc = entry_call(ctx, case, sites, out, **kw)[0]
        err = ctx.lib.tvr_last_error().decode()
        assert rc == L.TVR_ERR_INVALID and err.startswith("tvr_site_entry: ") and message in err, (message, rc, err)

    refused("null model", model=None)
    refused("16-byte aligned", resid=resid + 4)
    refused("16-byte aligned", z=z + 8)
    refused("exceeds tokens", cap=case.tokens - 1)
    refused("outside [1, n_ctx]", lens=[1, 0, 16, 17, 33])
    refused("outside [1, n_ctx]", lens=[1, 15, 16, 17, N_CTX + 1], cap=1000)
    refused("unknown flags", flags=2)
    refused("more than out_rows", out_rows=35)
    refused("needs 16-byte aligned vectors", vec_shift=1)
    refused("seq out of range", sites=[E.Site(5, E.NONE)])
    refused("layer/head out of range", sites=[E.Site(0, E.REPLACE_HEAD, layer=N_LAYERS)])
    refused("layer/head out of range", sites=[E.Site(0, E.REPLACE_HEAD, head=ctx.H)])
    refused("vector out of range", sites=[E.Site(0, E.REPLACE_HEAD, vec=3)])
    refused("vector out of range", n_vectors=0)
    refused("resid patch out of range", sites=[E.Site(2, E.SET_POS, pos=16, src_seq=0)])
    refused("resid patch out of range", sites=[E.Site(2, E.SET_POS, pos=1, src_seq=1, src_pos=15)])
    refused("tvr_patch_sweep_sets", sites=[E.Site(2, E.SET_ALLPOS)])
    refused("only head-set kinds", sets=[((0, 0, 0),), ()])
    refused("patch layer/head out of range", sites=[E.Site(2, E.SET_ALLPOS)], sets=[((0, ctx.H, 0),)])
    refused("twice in one set", sites=[E.Site(2, E.SET_LASTPOS)], sets=[((1, 1, 0), (1, 1, 2))])
    for null in ("seq_lens", "resid", "z", "sites", "out", "report"):
        n = 2
        a = [ctx.h, (ctypes.c_int32 * 5)(*case.seq_lens), 5, None, case.cap, resid, z, c_sites(ok), n, None, None,
             case.vec[0].data_ptr(), 3, 0, out.ptr, out.rows] + [(ctypes.c_int32 * n)() for _ in range(3)] + [ctx.stream()]
        a[{"seq_lens": 1, "resid": 5, "z": 6, "sites": 7, "out": 14, "report": 17}[null]] = None
        assert ctx.lib.tvr_site_entry(*a) == L.TVR_ERR_INVALID and b"null" in ctx.lib.tvr_last_error(), null
    torch.cuda.synchronize()
    assert out.untouched()
    res = entry(ctx, case, ok)  # the model is still usable
    assert (bits(res[1][1]) == bits(E.site_rows(case, ok[1])[1])).all()


def test_invalid_headset_arguments_launch_nothing():
    ctx = _ctx(A.MODELS[0])
    items, patches, rows = hs_layout(ctx.H)
    a2, resid, vectors = hs_buffers("f32", ctx, rows, items)

    def refused(message, items=items, patches=patches, over=None):
        rc, got_a2, got_r = headset_call(ctx, "f32", a2, resid, vectors, items, patches, over=over)
        err = ctx.lib.tvr_last_error().decode()
        assert rc == L.TVR_ERR_INVALID and err.startswith("tvr_headset_apply: ") and message in err, (message, rc, err)
        assert (got_a2 == a2).all() and (bits(got_r) == bits(resid)).all(), message  # nothing was launched

    rc = headset_call(ctx, "f32", a2, resid, vectors, items, patches, model=None)[0]
    assert rc == L.TVR_ERR_INVALID and ctx.lib.tvr_last_error().startswith(b"tvr_headset_apply: null model")
    for null in ("items", "vectors", "a2", "resid"):
        refused("null", over={null: None})
    refused("patches is null", over={"patches": None})
    refused("n_items must be positive", over={"n_items": 0})
    refused("n_patches is negative", over={"n_patches": -1})
    refused("rows must be positive", over={"rows": 0})
    refused("n_vectors is negative", over={"n_vectors": -1})
    refused("unknown fmt", over={"fmt": 7})
    refused("16-byte aligned", over={"a2": lambda p: p + 4})
    refused("16-byte aligned", over={"resid": lambda p: p + 8})
    refused("float aligned", over={"vectors": lambda p: p + 2})
    refused("n_rows must be at least 1", items=[(1, 0, 0, 1)])
    refused("outside the buffers", items=[(rows - 2, 3, 0, 1)])
    refused("outside the buffers", items=[(-1, 3, 0, 1)])
    refused("patch range outside the list", items=[(1, 3, len(patches), 1)])
    refused("patch range outside the list", items=[(1, 3, -1, 1)])
    refused("head out of range", items=[(1, 3, 0, 1)], patches=[(ctx.H, 0)])
    refused("head out of range", items=[(1, 3, 0, 1)], patches=[(-1, 0)])
    refused("vector out of range", items=[(1, 3, 0, 1)], patches=[(0, 4)])
    refused("two items share rows", items=[(1, 3, 0, 1), (3, 2, 0, 1)])
    rc, got_a2, got_r = headset_call(ctx, "f32", a2, resid, vectors, items, patches)  # the model is still usable
    L.check(rc, "tvr_headset_apply")
    want_a2, want_r = E.headset_expect("f32", ctx.DH, ctx.K2, a2, resid, vectors, items, patches)
    assert (got_a2 == want_a2).all() and (bits(got_r) == bits(want_r)).all()
