"""Per-source-token attribution launches with known answers, their fp64 reference
and the bar (shared by test_source_cases.py and test_gpu_source_attribution.py; a
plain module, not a conftest).  Host only.

The quantity, for one query row q per sequence, head h and key j <= q:

  src[s][h][j] = p[s][h][j] * (v[j][h] . g[s][h])         g[s] = (u[s] / sigma[s]) @ W_O
               = p[s][h][j] * ((v[j][h] @ W_O[h]) . u[s] / sigma[s])

with p the attention pattern of pattern_cases, W_O the columns [0, d) of a
tvr_layer_weights.w2 stand-in in (head, d_head) order, zero for j > q.

A launch is pattern_cases' launch (built on ``pattern_cases.make``: a sequence
queried at its last row, one queried mid-sequence, one of a single position;
every Q row but the queries' NaN, a NaN row after every sequence) with random V
rows, and NaN in the V of every row past each query: a kernel that reads a V it
has no business reading returns NaN.  The kernel's inputs are ``qkv`` and ``g``
(fp32 [n_seq][d]); ``g`` is the fp64 product (u / sigma) @ W_O of the case's
``u``, ``sigma`` and ``W`` rounded once to fp32.

``reference`` is the exact function of the kernel's inputs, in fp64: the pattern
of ``pattern_cases.reference`` times v . g.  Two fp32 restatements in different
summation orders stand for "a correct fp32 implementation":

  pattern  the plain fp32 pattern first, then V @ g as one BLAS product
  result   hook_result style: v_j projected through W_O[h] to d_model first, the
           dot with the UNscaled u in reversed column order, divided by sigma
           last; the pattern from the chunked online softmax

bar(case) = max(4 x their larger max |restatement - fp64|,
                4 x 2^-24 x the largest sum of |terms| of a key's value),
the project's convention (attribution_cases.bar); a key's terms are
p_j |v_je g_e| over the head's dims.  The bar never comes from the engine.

Kinds: ``random``, ``random_gain`` (4 x the query gain of pattern_cases and
columns of g of very different size); ``select``: a one-hot pattern and a g that
is one power of two per head, so src is V[hot][a] * 2^k at the hot key, bit for
bit, and zero elsewhere (of either sign: +0 times a negative dot is -0);
``unit``: V and g such that every v_j . g is exactly 1.0 in any summation order
(four products of 0.25, one in each chain of the kernel), so src is the pattern
bit for bit; ``zero``: g = 0.  The exact kinds use W_O = I, sigma = 2 and
u = 2 g, for which (u / sigma) @ W_O is g without rounding.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import attention_cases as A
import attribution_cases as C
import pattern_cases as P

ALL_T = (1, 15, 63, 64, 65, 129)  # the lane-count edges 63 / 64 / 65; a third pass over the keys
KINDS = ("random", "random_gain", "select", "unit", "zero")
MUTATIONS = ("head_g", "v_from_k", "unnormalised", "key_after_q")
BAR_MARGIN = C.BAR_MARGIN
FLOOR_ULPS = C.FLOOR_ULPS
EPS24 = C.EPS24
_PATTERN_KIND = {"random": "random", "random_gain": "random_gain", "select": "select", "unit": "random", "zero": "random"}


def unit_dims(d_head):
    """One dim in each of the kernel's four chains (dim e in chain e % 4), spread over the head."""
    dims = (0, d_head // 4 + 1, d_head // 2 + 2, d_head - 1)
    assert sorted(e % 4 for e in dims) == [0, 1, 2, 3]
    return dims


def _finish(case, W, u, sigma, dtype=np.float32):
    """W [d][>= d], u [n_seq][d], sigma [n_seq] kept in ``dtype``: g = fp32((u / sigma) @ W_O), from fp64."""
    d = case.d
    case.W, case.u, case.sigma = np.ascontiguousarray(W, dtype=dtype), np.asarray(u, dtype=dtype), np.asarray(sigma, dtype=dtype)
    g64 = (case.u.astype(np.float64) / case.sigma.astype(np.float64)[:, None]) @ case.W[:, :d].astype(np.float64)
    case.g = np.ascontiguousarray(g64.astype(np.float32))
    return case


def make(kind, d_head, n_heads, T, rot=0, W=None):
    """The pattern_cases launch for T with V rows, ``g`` [n_seq][d] and what the restatements need (``W``, ``u``,
    ``sigma``).  W: fp32 [d][>= d] for the random kinds (default attribution_cases.weights)."""
    case = P.make(_PATTERN_KIND[kind], d_head, n_heads, T, rot=rot)
    case.kind = kind
    H, DH, d, n_seq = n_heads, d_head, case.d, case.lay.n_seq
    rng = np.random.default_rng([T, DH, H, KINDS.index(kind)])
    eye = np.concatenate([np.eye(d, dtype=np.float32), np.zeros((d, C.D_MLP), dtype=np.float32)], 1)
    if kind in ("random", "random_gain"):
        W = C.weights(DH, H) if W is None else W
        u = rng.standard_normal((n_seq, d)).astype(np.float32)
        if kind == "random_gain":
            u *= np.exp2(rng.integers(-6, 6, size=(1, d))).astype(np.float32)
        _finish(case, W, u, (0.5 + rng.random(n_seq)).astype(np.float32))
    else:
        g = np.zeros((n_seq, H, DH), dtype=np.float32)
        if kind == "select":  # one power of two per (sequence, head), at a dim that moves with both
            a = (3 * np.arange(n_seq)[:, None] + 5 * np.arange(H)[None, :] + rot) % DH
            k = (np.arange(n_seq)[:, None] + np.arange(H)[None, :]) % 5 - 2
            np.put_along_axis(g, a[..., None], np.exp2(k).astype(np.float32)[..., None], -1)
            case.hot_dim = a
        elif kind == "unit":
            live = ~np.isnan(case.qkv[:, 2 * d])  # (the rows between the sequences stay NaN)
            for i, e in enumerate(unit_dims(DH)):
                for h in range(H):
                    k = (h + i) % 3
                    g[:, h, e] = np.float32(2.0 ** k)
                    case.qkv[live, 2 * d + h * DH + e] = np.float32(0.25 * 2.0 ** -k)
        else:
            assert kind == "zero", kind
        g = g.reshape(n_seq, d)
        _finish(case, eye, 2.0 * g, np.full(n_seq, 2.0, dtype=np.float32))
        assert np.array_equal(case.g, g)
    # V of every row past a query, as the rows between the sequences: never read
    for sd in case.seqs:
        case.qkv[sd.row0 + sd.q0 + 1:sd.row0 + sd.n, 2 * d:] = np.nan
    return case


def from_rows(q, k, v, lens, qpos, d_head, n_heads, W, u, sigma=None, dtype=np.float32, xL=None, eps=None):
    """A case from given Q / K / V rows ([tokens][d], sequences packed in order, before rotary), a layer's w2,
    the unscaled directions u [n_seq][d] and sigma [n_seq]: what judges an attribution computed from exactly
    these values (a trace's own hook_q / hook_k / hook_v).  ``g`` is not an input here: ``reference_from_model``.
    xL [n_seq][d] and eps instead of sigma: the final residual rows, whose LayerNormPre scale every form computes
    in its own precision (attribution_cases.centre_scale).  dtype = float64 keeps every array unrounded (the
    oracle's own rows)."""
    case = P.from_rows(np.asarray(q, dtype=np.float32), np.asarray(k, dtype=np.float32), lens, qpos, d_head, n_heads)
    d, off = case.d, 0
    case.qkv = case.qkv.astype(dtype)
    for sd in case.seqs:
        for i, a in enumerate((q, k, v)):
            case.qkv[sd.row0:sd.row0 + sd.n, i * d:(i + 1) * d] = np.asarray(a[off:off + sd.n], dtype=dtype)
        off += sd.n
    case.kind = "rows"
    if sigma is None:
        case.xL, case.eps = np.asarray(xL, dtype=dtype), eps
        sigma = C.centre_scale(case.xL, eps, np.float64)
    return _finish(case, W, u, sigma, dtype)


def _sigma(case, s, dtype):
    if hasattr(case, "xL"):
        return C.centre_scale(case.xL[s:s + 1], case.eps, dtype)[0]
    return case.sigma[s].astype(dtype)


# ------------------------------------------------------------------ the value side: v_j . g per key
def _keys(case, s, cols):
    sd = case.seqs[s]
    d = case.d
    return case.qkv[sd.row0:sd.row0 + sd.q0 + 1, cols * d:(cols + 1) * d].reshape(sd.q0 + 1, case.n_heads, case.d_head)


def dots_given(case, dtype, cols=2, roll=0):
    """[n_seq][H][maxT] of v_j[h] . g[s][h] from the given g, in ``dtype`` (fp32: one BLAS product per head);
    zero beyond each query.  cols = 1: "V" read from the K columns; roll: the neighbouring head's g."""
    H, DH = case.n_heads, case.d_head
    out = np.zeros((case.lay.n_seq, H, case.maxT), dtype=dtype)
    for s, sd in enumerate(case.seqs):
        v = _keys(case, s, cols).astype(dtype)
        g = np.roll(case.g[s].reshape(H, DH), roll, 0).astype(dtype)
        for h in range(H):
            out[s, h, :sd.q0 + 1] = v[:, h] @ g[h]
    return out


def dots_plain(case, dtype):
    """As dots_given, from u, sigma and W in ``dtype``: dirs = u / sigma, g = dirs @ W_O, then v . g."""
    H, DH, d = case.n_heads, case.d_head, case.d
    WO = case.W[:, :d].astype(dtype)
    out = np.zeros((case.lay.n_seq, H, case.maxT), dtype=dtype)
    for s, sd in enumerate(case.seqs):
        g = ((case.u[s].astype(dtype) / _sigma(case, s, dtype)).astype(dtype) @ WO).astype(dtype).reshape(H, DH)
        v = _keys(case, s, 2).astype(dtype)
        for h in range(H):
            out[s, h, :sd.q0 + 1] = v[:, h] @ g[h]
    return out


def dots_result(case, dtype):
    """hook_result style: r[j][h][c] = sum_k v[j][h][k] W_O[c][h dh + k] first, then the dot with the unscaled u in
    reversed column order, divided by sigma last."""
    H, DH, d = case.n_heads, case.d_head, case.d
    WO = case.W[:, :d].astype(dtype).reshape(d, H, DH)
    out = np.zeros((case.lay.n_seq, H, case.maxT), dtype=dtype)
    for s, sd in enumerate(case.seqs):
        r = np.einsum("jhk,chk->jhc", _keys(case, s, 2).astype(dtype), WO).astype(dtype)
        dot = (r[:, :, ::-1] * case.u[s].astype(dtype)[None, None, ::-1]).sum(-1, dtype=dtype)
        out[s, :, :sd.q0 + 1] = (dot / _sigma(case, s, dtype)).astype(dtype).T
    return out


def terms(case):
    """[n_seq][H][maxT]: p_j sum_e |v_je g_e| (the given g) in fp64, with the fp64 pattern of the plain tables: the
    magnitude the roundings of one output act on."""
    H, DH = case.n_heads, case.d_head
    out = np.zeros((case.lay.n_seq, H, case.maxT))
    for s, sd in enumerate(case.seqs):
        v = np.abs(_keys(case, s, 2).astype(np.float64))
        g = np.abs(case.g[s].reshape(H, DH).astype(np.float64))
        out[s, :, :sd.q0 + 1] = np.einsum("jhe,he->hj", v, g)
    return out


# ------------------------------------------------------------------ reference, restatements, bar
def _scores64(case, s, cos, sin):
    """fp64 scaled scores [H][T] of sequence s' query against all of its rows' keys (pattern_cases' arithmetic)."""
    H, DH, d = case.n_heads, case.d_head, case.d
    sd = case.seqs[s]
    cos, sin = torch.as_tensor(cos).double(), torch.as_tensor(sin).double()
    rows = torch.as_tensor(case.qkv[sd.row0:sd.row0 + sd.n]).double()
    q = A._rotary(rows[sd.q0:sd.q0 + 1, :d].reshape(1, H, DH), torch.tensor([sd.q0]), cos, sin, DH)
    k = A._rotary(rows[:, d:2 * d].reshape(sd.n, H, DH), torch.arange(sd.n), cos, sin, DH)
    return (torch.einsum("qhe,khe->hk", q, k) / math.sqrt(DH)).numpy()


def reference(case, cos, sin, mutate=None):
    """fp64 src [n_seq][H][maxT] from the kernel's inputs (qkv, g); zero beyond each query position.  mutate:
    one of MUTATIONS, a subtly wrong attribution."""
    p = P.reference(case, cos, sin)
    if mutate == "unnormalised":  # exp(score - max) without the division: the best key's weight is 1
        p = p / p.max(-1, keepdims=True)
    elif mutate == "key_after_q":  # the softmax runs over the keys <= q + 1 where the sequence has that row
        p = p.copy()
        for s, sd in enumerate(case.seqs):
            if sd.q0 + 1 < sd.n:
                sc = _scores64(case, s, cos, sin)[:, :sd.q0 + 2]
                e = np.exp(sc - sc.max(-1, keepdims=True))
                p[s, :, :sd.q0 + 1] = (e / e.sum(-1, keepdims=True))[:, :sd.q0 + 1]
    elif mutate not in (None, "head_g", "v_from_k"):
        raise ValueError(mutate)
    return p * dots_given(case, np.float64, cols=1 if mutate == "v_from_k" else 2, roll=1 if mutate == "head_g" else 0)


def reference_from_model(case, cos, sin):
    """fp64 src from u, sigma and W (g is not rounded to fp32 on the way): the trace path's reference."""
    return P.reference(case, cos, sin) * dots_plain(case, np.float64)


def restate_pattern(case, cos, sin, given=True):
    """fp32: the plain pattern first, then V @ g (given: the kernel's g; else g = (u / sigma) @ W_O in fp32)."""
    return (P.restate_plain(case, cos, sin) * (dots_given(case, np.float32) if given else dots_plain(case, np.float32))
            ).astype(np.float32)


def restate_result(case, cos, sin):
    """fp32: the chunked online-softmax pattern times the hook_result-style dot."""
    return (P.restate_chunked(case, cos, sin) * dots_result(case, np.float32)).astype(np.float32)


def max_err(got, ref):
    e = np.abs(np.asarray(got, dtype=np.float64)[..., :ref.shape[-1]] - ref)
    return float("inf") if np.isnan(e).any() else float(e.max()) if e.size else 0.0


def floor_of(case, cos, sin):
    return FLOOR_ULPS * EPS24 * float((P.reference(case, cos, sin) * terms(case)).max())


def bar(case, cos, sin, ref=None, given=True):
    """(bar, err of the pattern-first fp32 restatement, err of the hook_result-style one).  given: against
    ``reference`` (the kernel alone); else against ``reference_from_model`` (the trace path, which forms g itself)."""
    if ref is None:
        ref = reference(case, cos, sin) if given else reference_from_model(case, cos, sin)
    e1 = max_err(restate_pattern(case, cos, sin, given), ref)
    e2 = max_err(restate_result(case, cos, sin), ref)
    return max(BAR_MARGIN * max(e1, e2), floor_of(case, cos, sin)), e1, e2


# ------------------------------------------------------------------ the G pass: g = dirs @ W_O
def g_of(dirs, W, dtype=np.float64, reverse=False):
    """[n][d] = dirs @ W_O in ``dtype``; reverse: the weight rows summed in reversed order."""
    d = dirs.shape[1]
    a, WO = dirs.astype(dtype), np.ascontiguousarray(W[:, :d]).astype(dtype)
    return (a[:, ::-1] @ WO[::-1]).astype(dtype) if reverse else (a @ WO).astype(dtype)


def g_bar(dirs, W, ref=None):
    """(bar, err of the plain fp32 product, err of the reversed one): 4 x the larger, floored at 4 x 2^-24 x the
    largest sum of |dirs W| of an output."""
    ref = g_of(dirs, W) if ref is None else ref
    e1, e2 = max_err(g_of(dirs, W, np.float32), ref), max_err(g_of(dirs, W, np.float32, True), ref)
    t = np.abs(dirs.astype(np.float64)) @ np.abs(W[:, :dirs.shape[1]].astype(np.float64))
    return max(BAR_MARGIN * max(e1, e2), FLOOR_ULPS * EPS24 * float(t.max())), e1, e2


def select_exact(case, ld=None):
    """The exact src of a select case, fp32 [n_seq][H][ld]: V[hot][hot_dim] * g[hot_dim] at the hot key (one
    exact product: g is a power of two), zero elsewhere."""
    H, DH, d = case.n_heads, case.d_head, case.d
    out = np.zeros((case.lay.n_seq, H, ld or case.maxT), dtype=np.float32)
    for s, sd in enumerate(case.seqs):
        for h in range(H):
            j, a = int(case.hot[s, h]), int(case.hot_dim[s, h])
            out[s, h, j] = case.qkv[sd.row0 + j, 2 * d + h * DH + a] * case.g[s, h * DH + a]
    return out


def classes(case):
    """pattern_cases.classes: one class per row in [-1, N_CLASSES), with empty classes."""
    return P.classes(case)


def class_sums(src, case, cls, n_classes=P.N_CLASSES):
    """[n_seq][H][n_classes] of src summed in fp64 over the keys <= the query position by class."""
    return P.class_sums(src, case, cls, n_classes)
