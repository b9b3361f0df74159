"""Site-entry and head-set patch cases with known answers, their fp64 reference
and the bar (shared by test_entry_cases.py and test_gpu_entry.py; a plain
module, not a conftest).  Host only, numpy.

A ``Case`` is what tvr_site_entry reads: ragged sequences laid out one after
another, ``resid`` [L + 1][tokens][d] (hook_resid_pre), ``z`` [L][tokens][d]
(attn.hook_z), one W [d][d + D_MLP] per layer (tvr_layer_weights.w2: columns
[0, d) are W_O in (head, d_head) order) and ``vectors`` [nv][d].  A ``Site`` has
the fields of tvr_site.  ``site_rows`` gives the rows a site materialises at its
entry layer, for ALL the positions the unshared site computes (a shared-prefix
follower's rows are the tail of them):

  kind 1  e = layer + 1, positions 0 .. T - 1:
          out[i][c] = resid[e][i][c] + v[c] - sum_k z[layer][i][h dh + k] W[layer][c][h dh + k]
  kind 0  e = L: the last row of resid[L]          (copy)
  kind 2  e = layer + 1: last row of resid[e] + v  (one fp32 addition)
  kind 3  e = layer, positions pos .. T - 1: copies of resid[e], position pos
          from (src_seq, src_pos)                  (copy)
  kind 6  the same with vectors[vec] at pos        (copy)
  kinds 4 / 5 (given the site's patches): copies of resid[e] at the lowest
          patched layer e, all positions / the last

Kinds 0, 2, 3, 6 (and 4 / 5) have ONE right answer in fp32 and are compared bit
for bit.  Kind 1 is graded against fp64 at
    bar = max(BAR_MARGIN x the worse of two fp32 restatements' max error, floor)
with the restatements
    a   snap + (v - dot), the dot summed sequentially in k
    b   (snap + v) - dot, the dot over k reversed, summed pairwise
and floor = FLOOR_ULPS x 2^-24 x the largest |snap| + |v| + sum_k |z w| over the
case's outputs: four roundings at the magnitude of the summands (BAR_MARGIN is
attention_cases', FLOOR_ULPS attribution_cases': the project's convention).

Operand kinds (``KINDS``): random; gain (z rows at 2^-12 .. 2^12, columns of W,
resid and v at 2^-6 .. 2^6); cancel (every position's z within 2^-17 of one
large row and v within a few ulps of that row's z W: v - dot cancels, the
mean-head-replacement regime); zero (z = 0 in two rows of three: those rows are
snap + v exactly, one addition); and two exact kinds, right in ANY summation
order:
    select   z rows one-hot: the dot is one column of W exactly, the answer
             fl(snap + fl(v - w)) (the kernels' association, restatement a's;
             restatement b's dot is that column too, its last two roundings
             associate the other way and are not compared)
    integer  small-integer z, W, resid and v: every partial sum is an integer
             below 2^24
With the seeds of test_entry_cases.py the floor sets the bar in 11 of the 72
graded cases (15 %, asserted there at no more than a quarter): where d_head is
16 the two restatements are sometimes within an ulp or two of fp64.

Head sets (``headset_expect``): the listed heads' columns of a2 zero in every
plane, every other byte as it was, and resid + s with s = ((0 + v0) + v1) + ..
in list order (fp32), stated from the formats' definitions in include/tvr.h
(tvr_act_rows), not from the kernel's byte arithmetic.

``MUTATIONS`` are subtly wrong references; test_entry_cases.py shows that each
misses the bar or the exact comparison.  ``clamp`` stands for a tile clamp that
is off by one: a kernel clamping at tn in place of tn - 1 changes only tile
rows that are never stored (it reads one row further, no more), so a host
restatement of that changes nothing; the mutation clamps at tn - 2, which
reaches a stored row.
"""
from __future__ import annotations

import collections

import numpy as np

from attention_cases import BAR_MARGIN
from attribution_cases import EPS24, FLOOR_ULPS, max_err

D_MLP = 32
KINDS = ("random", "gain", "cancel", "select", "integer", "zero")
GRADED = ("random", "gain", "cancel", "zero")
MUTATIONS = ("wrong_head", "clamp", "v_plus_acc", "drop_k_chunk")
NONE, REPLACE_HEAD, ADD_LAST, SET_POS, SET_ALLPOS, SET_LASTPOS, SET_VEC = 0, 1, 2, 3, 4, 5, 6

Site = collections.namedtuple("Site", "seq kind layer head pos src_seq src_pos vec target",
                              defaults=(0, 0, 0, 0, 0, 0, -1))


class Case:
    def __init__(self, kind, d_head, n_heads, L, seq_lens, resid, z, W, vectors):
        self.kind, self.d_head, self.n_heads, self.L, self.d = kind, d_head, n_heads, L, d_head * n_heads
        self.seq_lens = list(seq_lens)
        self.off = [int(x) for x in np.concatenate([[0], np.cumsum(self.seq_lens)[:-1]])]
        self.tokens = int(sum(self.seq_lens))
        self.resid, self.z, self.W, self.vectors = resid, z, W, vectors


def make(kind, d_head, n_heads, seq_lens, L=2, nv=3, seed=0):
    d, tok = d_head * n_heads, int(sum(seq_lens))
    rng = np.random.default_rng([seed, d_head, n_heads, tok, KINDS.index(kind)])
    f32 = np.float32
    resid = rng.standard_normal((L + 1, tok, d)).astype(f32)
    z = rng.standard_normal((L, tok, d)).astype(f32)
    W = (rng.standard_normal((L, d, d + D_MLP)) * 0.2).astype(f32)
    vectors = rng.standard_normal((nv, d)).astype(f32)
    if kind == "gain":
        col = np.exp2(rng.integers(-6, 6, size=d)).astype(f32)
        z *= np.exp2(rng.integers(-12, 12, size=(L, tok, 1))).astype(f32)
        W *= col[None, :, None]
        resid *= col
        vectors *= col
    elif kind == "cancel":
        # every head's z row nearly the same at every position, and vector h % nv the fp32 rounding of head
        # (h % nv)'s z W of layer 0 moved by up to 3 ulps: v - dot is a few ulps of a value near 100
        base = (rng.standard_normal((L, 1, d)) * 64.0).astype(f32)
        z = (base * (1.0 + np.arange(tok)[None, :, None] * 2.0 ** -17)).astype(f32)
        for v in range(nv):
            h = v % n_heads
            dot = z[0, 0, h * d_head:(h + 1) * d_head].astype(np.float64) @ \
                W[0, :, h * d_head:(h + 1) * d_head].astype(np.float64).T
            x = dot.astype(f32)
            step = np.spacing(np.abs(x)) * rng.integers(-3, 4, size=d).astype(f32)
            vectors[v] = x + step
    elif kind == "select":
        z[:] = 0.0
        k = (7 * np.arange(tok)[None, :] + 3 * np.arange(L)[:, None] + 5) % d_head
        for h in range(n_heads):  # one-hot in every head: dim k + h of the head's slice
            kk = (k + h) % d_head
            z[np.arange(L)[:, None], np.arange(tok)[None, :], h * d_head + kk] = 1.0
    elif kind == "integer":
        z = rng.integers(-8, 9, size=z.shape).astype(f32)
        W = rng.integers(-8, 9, size=W.shape).astype(f32)
        resid = rng.integers(-1000, 1001, size=resid.shape).astype(f32)
        vectors = rng.integers(-1000, 1001, size=vectors.shape).astype(f32)
    elif kind == "zero":
        for s, (o, T) in enumerate(zip(np.cumsum([0] + list(seq_lens))[:-1], seq_lens)):
            i = np.arange(T)
            z[:, o + i[i % 3 != 0]] = 0.0
    elif kind != "random":
        raise ValueError(kind)
    return Case(kind, d_head, n_heads, L, seq_lens, *(np.ascontiguousarray(a) for a in (resid, z, W, vectors)))


def zero_positions(T):
    """Positions of a ``zero`` case's sequence whose z row is 0."""
    return np.arange(T) % 3 != 0


# ------------------------------------------------------------------------------ kind 1
def _operands(case, site, mutate=None):
    T, o, dh = case.seq_lens[site.seq], case.off[site.seq], case.d_head
    h = (site.head + 1) % case.n_heads if mutate == "wrong_head" else site.head
    pos = np.arange(T)
    if mutate == "clamp":  # the last position of every tile of 16 (and of the sequence) reads its neighbour
        tn = np.minimum(16, T - 16 * (pos // 16))
        pos = 16 * (pos // 16) + np.minimum(pos % 16, np.maximum(tn - 2, 0))
    snap = case.resid[site.layer + 1, o:o + T]
    zz = case.z[site.layer, o + pos, h * dh:(h + 1) * dh]
    w = case.W[site.layer][:, h * dh:(h + 1) * dh]
    if mutate == "drop_k_chunk":  # the last four k of the second lane group's share
        zz = zz.copy()
        zz[:, dh // 2 - 4:dh // 2] = 0.0
    return snap, zz, w, case.vectors[site.vec]


def _dot_seq(zz, w):
    """fp32, sequential in k: [T][d]."""
    acc = np.zeros((zz.shape[0], w.shape[0]), dtype=np.float32)
    for k in range(zz.shape[1]):
        acc = acc + zz[:, k, None] * w[None, :, k]
    return acc


def _dot_pairwise_reversed(zz, w):
    """fp32, k reversed, summed as a binary tree: [T][d]."""
    p = (zz[:, None, ::-1] * w[None, :, ::-1]).astype(np.float32)
    while p.shape[-1] > 1:
        n = p.shape[-1]
        q = p[..., 0:n - n % 2:2] + p[..., 1:n:2]
        p = np.concatenate([q, p[..., n - 1:]], -1) if n % 2 else q
    return p[..., 0]


def replace_head_rows(case, site, form="ref", mutate=None):
    """[T][d]: fp64 (form "ref"), or one of the fp32 restatements "a" / "b"."""
    snap, zz, w, v = _operands(case, site, mutate)
    if form == "ref":
        dot = zz.astype(np.float64) @ w.astype(np.float64).T
        v64, s64 = v.astype(np.float64), snap.astype(np.float64)
        return s64 + v64 + dot if mutate == "v_plus_acc" else s64 + v64 - dot
    if form == "a":
        dot = _dot_seq(zz, w)
        return snap + (v[None, :] + dot) if mutate == "v_plus_acc" else snap + (v[None, :] - dot)
    dot = _dot_pairwise_reversed(zz, w)
    return (snap + v[None, :]) + dot if mutate == "v_plus_acc" else (snap + v[None, :]) - dot


def replace_head_dots(case, site):
    """The two restatements' dots alone (the exact kinds: both are exact)."""
    _, zz, w, _ = _operands(case, site)
    return _dot_seq(zz, w), _dot_pairwise_reversed(zz, w)


def replace_head_terms(case, site):
    """[T][d]: |snap| + |v| + sum_k |z w|, fp64."""
    snap, zz, w, v = _operands(case, site)
    return np.abs(snap.astype(np.float64)) + np.abs(v.astype(np.float64))[None, :] + \
        np.abs(zz.astype(np.float64)) @ np.abs(w.astype(np.float64)).T


def replace_head_exact(case, site):
    """[T][d] fp32, the one right answer of the exact kinds (and of the z = 0 rows of ``zero``)."""
    snap, zz, w, v = _operands(case, site)
    if case.kind == "select":
        k = np.argmax(zz, axis=1)
        assert (zz.sum(1) == 1.0).all()
        return snap + (v[None, :] - w[:, k].T)
    if case.kind == "integer":
        return (snap.astype(np.float64) + v.astype(np.float64) - zz.astype(np.float64) @ w.astype(np.float64).T).astype(np.float32)
    assert case.kind == "zero"
    return snap + v[None, :]


def bar(case, sites, refs=None):
    """(bar, worse restatement error, floor) over the REPLACE_HEAD sites of a case."""
    e, terms = 0.0, 0.0
    for i, s in enumerate(sites):
        ref = replace_head_rows(case, s) if refs is None else refs[i]
        e = max(e, max_err(replace_head_rows(case, s, "a"), ref), max_err(replace_head_rows(case, s, "b"), ref))
        terms = max(terms, float(replace_head_terms(case, s).max()))
    floor = FLOOR_ULPS * EPS24 * terms
    return max(BAR_MARGIN * e, floor), e, floor


# ------------------------------------------------------------------------------ every kind
def entry_layer(case, site, patches=()):
    if site.kind in (REPLACE_HEAD, ADD_LAST):
        return site.layer + 1
    if site.kind in (SET_POS, SET_VEC):
        return site.layer
    return min([p[0] for p in patches], default=case.L)  # NONE and the head sets ((layer, head, vec) triples)


def site_rows(case, site, patches=()):
    """(p0, rows [T - p0][d]) of the unshared site: fp64 for kind 1, else the exact fp32 rows."""
    T, o = case.seq_lens[site.seq], case.off[site.seq]
    e = entry_layer(case, site, patches)
    if site.kind == REPLACE_HEAD:
        return 0, replace_head_rows(case, site)
    if site.kind == ADD_LAST:
        return T - 1, case.resid[e, o + T - 1:o + T] + case.vectors[site.vec][None, :]
    if site.kind in (SET_POS, SET_VEC):
        rows = case.resid[e, o + site.pos:o + T].copy()
        rows[0] = case.vectors[site.vec] if site.kind == SET_VEC else case.resid[e, case.off[site.src_seq] + site.src_pos]
        return site.pos, rows
    if site.kind == SET_ALLPOS and patches:
        return 0, case.resid[e, o:o + T].copy()
    return T - 1, case.resid[e, o + T - 1:o + T].copy()


# ------------------------------------------------------------------------------ head sets
HS_FORMATS = ("f32", "x2f16", "x2f16i", "bf16")
HS_MUTATIONS = ("wide_zero",)


def headset_columns(fmt, K2, cols):
    """Byte offsets within an a2 row (K2 * 4 bytes) of the logical columns ``cols``, every plane."""
    cols = np.asarray(cols)
    if fmt == "f32":
        return (4 * cols[:, None] + np.arange(4)[None, :]).ravel()
    if fmt == "bf16":  # halves [K2] (the row's second half is unused)
        halves = cols
    elif fmt == "x2f16":  # halves [2][K2]
        halves = np.concatenate([cols, K2 + cols])
    else:  # halves [K2 / 32][2][32]: column c of plane p is half (c / 32) * 64 + p * 32 + c % 32
        halves = np.concatenate([(cols // 32) * 64 + p * 32 + cols % 32 for p in (0, 1)])
    return (2 * halves[:, None] + np.arange(2)[None, :]).ravel()


def headset_expect(fmt, d_head, K2, a2, resid, vectors, items, patches, mutate=None):
    """(a2, resid) after the launch.  a2 uint8 [rows][4 K2], resid / vectors fp32, items (row0, n_rows,
    first_patch, n_patches), patches (head, vec)."""
    a2, resid = a2.copy(), resid.copy()
    for row0, n_rows, first, n in items:
        s = np.zeros(resid.shape[1], dtype=np.float32)
        for head, vec in patches[first:first + n]:
            cols = np.arange(head * d_head, (head + 1) * d_head + (8 if mutate == "wide_zero" and fmt != "f32" else
                                                                  4 if mutate == "wide_zero" else 0))
            a2[row0:row0 + n_rows, headset_columns(fmt, K2, cols[cols < K2])] = 0
            s = s + vectors[vec]
        resid[row0:row0 + n_rows] = resid[row0:row0 + n_rows] + s[None, :]
    return a2, resid
