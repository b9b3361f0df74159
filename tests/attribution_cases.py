"""Direct-logit-attribution cases with known answers, their fp64 reference and
the bar (shared by test_attribution_cases.py and test_gpu_attribution.py; a
plain module, not a conftest).  Host only, numpy.

The three quantities, from given arrays (``attribution``):

  dirs[s]         = (ut[s] - uc[s]) / sigma_s,  sigma_s = sqrt(mean((x_L - mean x_L)^2) + eps)
  resid[s][l]     = (x[l][s] - mean x[l][s]) . dirs[s]                       l in [0, L]
  heads[s][l][h]  = sum_k z[l][s][h dh + k] (sum_c dirs[s][c] W[l][c][h dh + k])

with W[l] the [d][>= d] matrix whose columns [0, d) are W_O in (head, d_head)
order (tvr_layer_weights.w2), ``ut`` / ``uc`` the unembedding rows of the target
and the contrast token.  ``heads_of`` is the last line alone for given
directions: the primitive tvr_head_attribution.

``reference`` evaluates them in fp64.  Two fp32 restatements in different
summation orders stand for "a correct fp32 implementation":

  plain   G = dirs @ W (a BLAS product), then the z dot over the head's columns;
          resid as one dot product with dirs
  result  hook_result first (r[s][h][c] = sum_k z W, TransformerLens'
          stack_head_results), then the dot with the UNscaled u in reversed
          column order, divided by sigma at the end; resid likewise

bar(case) = max(4 x the larger max |restatement - fp64|, floor), built exactly as
pattern_cases.bar is (the margin of 4 is attention_cases.BAR_MARGIN).  The
floor is 4 x 2^-24 x the largest sum of |terms| of any output of the case: four
roundings at the magnitude of the summands.  A smaller floor would hold an
implementation to an accident of the two restatements (on a 16-column head both
can be exact to the last bit, e.g. when all but a few products vanish); a larger
one would hide a lost term: every term that matters is far above 4 ulps of the
sum of their magnitudes.  Exact cases (``select``, ``zero``) are compared bit
for bit, not at the bar.
"""
from __future__ import annotations

import numpy as np

BAR_MARGIN = 4.0
FLOOR_ULPS = 4.0
EPS24 = 2.0 ** -24
KINDS = ("random", "gain", "cancel", "select", "zero")
ALL_N = (1, 15, 16, 17, 33)  # one row; a short chunk; a full one; one row into the second; a third chunk
D_MLP = 32


class Case:
    def __init__(self, kind, d_head, n_heads, W, z, dirs):
        self.kind, self.d_head, self.n_heads, self.d = kind, d_head, n_heads, d_head * n_heads
        self.W, self.z, self.dirs = W, z, dirs
        self.n = z.shape[0]
        self.exact = None  # select / zero: the exact fp32 answer [n][H]


def weights(d_head, n_heads, seed=5):
    """A stand-in for tvr_layer_weights.w2: fp32 [d][d + D_MLP]."""
    d = d_head * n_heads
    return np.random.default_rng(seed).standard_normal((d, d + D_MLP)).astype(np.float32) * np.float32(0.2)


def make(kind, d_head, n_heads, n, W=None, seed=0):
    """z, dirs fp32 [n][d] for W (fp32 [d][>= d]; default ``weights``)."""
    d = d_head * n_heads
    W = weights(d_head, n_heads) if W is None else np.ascontiguousarray(W, dtype=np.float32)
    assert W.shape[0] == d and W.shape[1] >= d
    rng = np.random.default_rng(1000 * seed + 17 * n + d_head + n_heads)
    z = rng.standard_normal((n, d)).astype(np.float32)
    dirs = rng.standard_normal((n, d)).astype(np.float32)
    exact = None
    if kind == "gain":  # rows and columns of very different size: every row has its own scale
        z *= np.exp2(rng.integers(-12, 12, size=(n, 1))).astype(np.float32)
        dirs *= np.exp2(rng.integers(-6, 6, size=(1, d))).astype(np.float32)
    elif kind == "cancel":
        # large head contributions that sum to nearly zero over the heads: scaled-up rows, and a direction
        # orthogonal (in fp64, before its rounding to fp32) to the sum over heads of the row's hook_result
        z *= np.float32(64.0)
        zw = np.einsum("nhk,chk->nhc", z.reshape(n, n_heads, d_head).astype(np.float64),
                       W[:, :d].reshape(d, n_heads, d_head).astype(np.float64))
        tot = zw.sum(1)
        v = rng.standard_normal((n, d))
        v -= (v * tot).sum(-1, keepdims=True) / np.maximum((tot * tot).sum(-1, keepdims=True), 1e-300) * tot
        dirs = (v * 8.0).astype(np.float32)
    elif kind == "select":
        # dirs a unit vector e_c, z a unit vector e_j: out[i][j // dh] = W[c][j], every other head +0.0
        c = (7 * np.arange(n) + 3) % d
        j = (11 * np.arange(n) + 5) % d
        z = np.zeros((n, d), dtype=np.float32)
        dirs = np.zeros((n, d), dtype=np.float32)
        z[np.arange(n), j] = 1.0
        dirs[np.arange(n), c] = 1.0
        exact = np.zeros((n, n_heads), dtype=np.float32)
        exact[np.arange(n), j // d_head] = W[c, j]
    elif kind == "zero":  # rows with z = 0 and rows with dirs = 0 among ordinary ones: exactly 0
        z[1::3] = 0.0
        dirs[2::3] = 0.0
    elif kind != "random":
        raise ValueError(kind)
    case = Case(kind, d_head, n_heads, W, np.ascontiguousarray(z), np.ascontiguousarray(dirs))
    case.exact = exact
    return case


def zero_rows(case):
    """Rows of a ``zero`` case whose answer is exactly 0."""
    r = np.arange(case.n)
    return r % 3 != 0


# ------------------------------------------------------------------------------ the three quantities
def heads_of(z, dirs, W, d_head, dtype=np.float64, form="plain", sigma=None):
    """[n][H].  form "plain": (dirs @ W_O) . z per head; "result": hook_result first, then the dot with dirs
    in reversed column order.  sigma [n] (result form of ``attribution``): dirs is the unscaled u, the
    quotient comes last."""
    n, d = z.shape
    H = d // d_head
    z, dirs, WO = z.astype(dtype), dirs.astype(dtype), np.ascontiguousarray(W[:, :d]).astype(dtype)
    if form == "plain":
        assert sigma is None
        g = dirs @ WO
        return (z * g).reshape(n, H, d_head).sum(-1, dtype=dtype)
    r = np.einsum("nhk,chk->nhc", z.reshape(n, H, d_head), WO.reshape(d, H, d_head)).astype(dtype)
    out = (r[:, :, ::-1] * dirs[:, None, ::-1]).sum(-1, dtype=dtype)
    return out if sigma is None else (out / sigma[:, None].astype(dtype)).astype(dtype)


def heads_terms(z, dirs, W, d_head):
    """[n][H]: the sum of |z W dirs| over the head's products, fp64."""
    n, d = z.shape
    g = np.abs(dirs.astype(np.float64)) @ np.abs(W[:, :d].astype(np.float64))
    return (np.abs(z.astype(np.float64)) * g).reshape(n, d // d_head, d_head).sum(-1)


def centre_scale(xL, eps, dtype):
    x = xL.astype(dtype)
    xc = x - x.mean(-1, keepdims=True, dtype=dtype)
    return np.sqrt((xc * xc).mean(-1, dtype=dtype) + dtype(eps)).astype(dtype)


def attribution(x, z, Ws, ut, uc, eps, d_head, dtype=np.float64, form="plain"):
    """(heads [n][L][H], resid [n][L + 1]) from x [L + 1][n][d] (the query rows of hook_resid_pre, x[L] the
    final residual), z [L][n][d], Ws [L] matrices, ut / uc [n][d] (uc may be None)."""
    L, n = len(Ws), x.shape[1]
    sigma = centre_scale(x[L], eps, dtype)
    u = ut.astype(dtype) - (0 if uc is None else uc.astype(dtype))
    xc = x.astype(dtype)
    xc = xc - xc.mean(-1, keepdims=True, dtype=dtype)
    if form == "plain":
        dirs = (u / sigma[:, None]).astype(dtype)
        heads = np.stack([heads_of(z[l], dirs, Ws[l], d_head, dtype) for l in range(L)], 1)
        resid = np.stack([(xc[l] * dirs).sum(-1, dtype=dtype) for l in range(L + 1)], 1)
    else:
        heads = np.stack([heads_of(z[l], u, Ws[l], d_head, dtype, "result", sigma) for l in range(L)], 1)
        resid = np.stack([((xc[l][:, ::-1] * u[:, ::-1]).sum(-1, dtype=dtype) / sigma).astype(dtype)
                          for l in range(L + 1)], 1)
    return heads, resid


def attribution_terms(x, z, Ws, ut, uc, eps, d_head):
    """Sums of |terms| of both outputs, fp64: (heads [n][L][H], resid [n][L + 1])."""
    L = len(Ws)
    sigma = centre_scale(x[L], eps, np.float64)
    dirs = (ut.astype(np.float64) - (0 if uc is None else uc.astype(np.float64))) / sigma[:, None]
    xc = x.astype(np.float64)
    xc = xc - xc.mean(-1, keepdims=True)
    heads = np.stack([heads_terms(z[l], dirs, Ws[l], d_head) for l in range(L)], 1)
    resid = np.stack([(np.abs(xc[l]) * np.abs(dirs)).sum(-1) for l in range(L + 1)], 1)
    return heads, resid


# ------------------------------------------------------------------------------ reference and bar
def reference(case):
    """fp64 out [n][H] of a primitive case."""
    return heads_of(case.z, case.dirs, case.W, case.d_head)


def restate_plain(case):
    return heads_of(case.z, case.dirs, case.W, case.d_head, np.float32, "plain")


def restate_result(case):
    return heads_of(case.z, case.dirs, case.W, case.d_head, np.float32, "result")


def max_err(got, ref):
    e = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return float("inf") if np.isnan(e).any() else float(e.max()) if e.size else 0.0


def floor_of(terms):
    return FLOOR_ULPS * EPS24 * float(np.max(terms)) if np.size(terms) else 0.0


def bar(case, ref=None):
    """(bar, err of the plain fp32 restatement, err of the result-first one)."""
    ref = reference(case) if ref is None else ref
    e1, e2 = max_err(restate_plain(case), ref), max_err(restate_result(case), ref)
    floor = floor_of(heads_terms(case.z, case.dirs, case.W, case.d_head))
    return max(BAR_MARGIN * max(e1, e2), floor), e1, e2


def attribution_bar(x, z, Ws, ut, uc, eps, d_head, ref=None):
    """(bar of heads, bar of resid) for the trace quantities, from the same two restatements."""
    ref = attribution(x, z, Ws, ut, uc, eps, d_head) if ref is None else ref
    a = attribution(x, z, Ws, ut, uc, eps, d_head, np.float32, "plain")
    b = attribution(x, z, Ws, ut, uc, eps, d_head, np.float32, "result")
    terms = attribution_terms(x, z, Ws, ut, uc, eps, d_head)
    return tuple(max(BAR_MARGIN * max(max_err(a[i], ref[i]), max_err(b[i], ref[i])), floor_of(terms[i]))
                 for i in range(2))


def select_is_exact(case):
    """Both fp32 restatements of a select case give W[c][j] in the head of column j and 0 elsewhere, bit for bit."""
    return all(np.array_equal(f(case), case.exact) for f in (restate_plain, restate_result))
