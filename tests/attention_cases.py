"""Attention launches with known answers, their fp64 reference and the bar
(shared by test_attention_cases.py and test_gpu_attention.py; a plain module,
not a conftest).

A launch is a batch of ragged sequences described as the kernels see them
(``Seq`` = csrc/sweep_desc.hpp SeqDesc = include/tvr.h tvr_attn_seq): computed
rows [row0, row0 + n) of ``qkv`` are the positions [p0, p0 + n), the K / V rows
of positions [0, p0) are rows ``cache_row ..`` of ``cache`` (prefix_live 0) or
of ``qkv`` itself (prefix_live 1), rows [q0, n) are queries.

``reference`` is the operation in fp64, written per sequence: gather, TL
rotate-half rotary on dims [0, d_head / 4) at absolute positions, scores
/ sqrt(d_head), keys <= query position, softmax, P V.  The bar of a case comes
from two fp32 restatements of the same function (``restate_plain``,
``restate_chunked``), never from the engine: bar = 4 x the larger of their
max |z - z64| over the launch, floored at 2^-22 max |V|.  The two fp32 orders
differ from each other by up to about 3 x, and the kernel is a third order
(permuted k, two MFMA chains, expf): hence the margin of 4.

Buffers.  Every sequence's rows are followed by one row that belongs to no
sequence, and so are the cache prefixes; those rows, the Q columns of the cache
and the Q columns of rows below q0 are NaN: a kernel that reads one row past a
sequence, or a Q it has no business reading, turns its output into NaN.
"""
from __future__ import annotations

import collections
import math
import types

import numpy as np
import torch

from oracle.hooked_pythia import HookedPythiaOracle

Seq = collections.namedtuple("Seq", "row0 n p0 cache_row q0 prefix_live")

# (d_head, n_heads): every head size; 6 and 3 heads: the single-query kernel is refused (n_heads % HG != 0)
MODELS = ((16, 4), (64, 4), (80, 4), (128, 2), (16, 6), (128, 3))
N_CTX = 320
D_MLP = 32
# longest T of a launch per kernel form (key tiles in registers; 0: chunked online softmax, 257: a third chunk)
MAXT = {1: (1, 15, 16), 2: (17, 32), 4: (33, 64), 8: (65, 128), 0: (129, 257, 300)}
ALL_T = tuple(t for ts in MAXT.values() for t in ts)
BAR_MARGIN = 4.0
BAR_FLOOR = 2.0 ** -22


def nkt_of(maxT):
    """launch_attention's key-tile form for a launch whose longest sequence is maxT."""
    kt = (maxT + 15) // 16
    return 1 if kt <= 1 else 2 if kt <= 2 else 4 if kt <= 4 else 8 if kt <= 8 else 0


def tables(d_head, n_ctx=N_CTX, base=10000.0, dtype=torch.float32):
    """TransformerLens' calculate_sin_cos_rotary as the oracle states it, computed in ``dtype``:
    (cos, sin) [n_ctx][d_head / 4]."""
    shim = types.SimpleNamespace(_table_dtype=dtype, dtype=dtype)
    sin, cos = HookedPythiaOracle._rotary_tables(shim, d_head // 4, n_ctx, base)
    return cos.numpy(), sin.numpy()


def tl_freq32(d_head, base=10000.0):
    """The fp32 frequencies of TL's tables, [d_head / 4] (the half repeated), as fp64 numbers."""
    half = d_head // 8
    f = torch.tensor(base, dtype=torch.float32) ** (torch.arange(half, dtype=torch.float32) / half)
    return torch.cat([f, f]).double().numpy()


def tables_from_freq(freq, n_ctx=N_CTX):
    """(cos, sin) [n_ctx][len(freq)] in fp64 of the angles pos / freq."""
    ang = np.arange(n_ctx, dtype=np.float64)[:, None] / np.asarray(freq, dtype=np.float64)[None, :]
    return np.cos(ang), np.sin(ang)


# ------------------------------------------------------------------ layouts
class Layout:
    """Sequences of one launch and where their rows sit (one free row before the first sequence and
    after every sequence, in ``qkv`` and in ``cache``)."""

    def __init__(self):
        self.seqs, self.rows, self.cache_rows, self.row_from = [], 1, 1, None

    def add(self, T, p0=0, q0=0, leader=None):
        """leader: index of an earlier sequence whose rows are the prefix (prefix_live 1); else the cache."""
        n = T - p0
        assert n >= 1 and 0 <= q0 < n
        cache_row, live = -1, 0
        if p0 and leader is not None:
            ld = self.seqs[leader]
            assert ld.p0 == 0 and ld.n >= p0
            cache_row, live = ld.row0, 1
        elif p0:
            cache_row = self.cache_rows
            self.cache_rows += p0 + 1
        self.seqs.append(Seq(self.rows, n, p0, cache_row, q0, live))
        self.rows += n + 1
        return self

    @property
    def maxT(self):
        return max(s.p0 + s.n for s in self.seqs)

    @property
    def n_seq(self):
        return len(self.seqs)


def batch(maxT, pad=None):
    """3-5 ragged sequences, the longest of maxT positions: a whole sequence, T = 1, a follower of the first
    (prefix_live 1), a cache prefix whose only query is the last row, a full-tile T behind a cache prefix
    with q0 = 3; p0 from {5, 16, 23} as far as they fit.  pad: one more sequence of that length at the END
    (the other sequences keep their rows and, generated per sequence, their values)."""
    lay = Layout().add(maxT).add(1)
    opts = [p for p in (5, 16, 23) if p < maxT]
    if opts:
        lay.add(maxT, p0=opts[-1], q0=min(3, maxT - opts[-1] - 1), leader=0)
        lay.add(max(maxT - 1, opts[0] + 1), p0=opts[0], q0=max(maxT - 1, opts[0] + 1) - opts[0] - 1)
        if maxT >= 16:
            full = 16 * (maxT // 16)
            p0 = 16 if full > 16 else 5
            lay.add(full, p0=p0, q0=min(3, full - p0 - 1))
    else:
        lay.add(maxT)
    lay.row_from = lay.n_seq
    if pad:
        lay.add(pad)
        lay.row_from = lay.n_seq
    assert lay.maxT == (pad or maxT)
    return lay


def batch_rows(maxT):
    """A launch with single-query sequences (row_from = 1): after one whole sequence, a sequence whose
    only query is its last row, one computed row behind a cache prefix (the patched last-position forwards),
    a follower of the first sequence, and T = 1."""
    lay = Layout().add(maxT)
    lay.add(maxT, q0=maxT - 1)
    if maxT > 1:
        lay.add(maxT, p0=maxT - 1)
        p0 = max(p for p in (1, 5, 16, 23) if p < maxT)
        lay.add(maxT, p0=p0, q0=maxT - p0 - 1, leader=0)
    lay.add(1)
    lay.row_from = 1
    return lay


# -------------------------------------------------------------------- cases
class Case:
    """qkv [rows][3 d] and cache [cache_rows][3 d] fp32 (numpy), the layout, and for ``select`` the exact
    expected z."""

    def __init__(self, kind, d_head, n_heads, lay, qkv, cache, expect=None):
        self.kind, self.d_head, self.n_heads, self.lay = kind, d_head, n_heads, lay
        self.qkv, self.cache, self.expect = qkv, cache, expect
        self.d = d_head * n_heads

    @property
    def seqs(self):
        return self.lay.seqs

    def own(self, s):
        sd = self.lay.seqs[s]
        return self.qkv[sd.row0:sd.row0 + sd.n]

    def prefix(self, s):
        sd = self.lay.seqs[s]
        src = self.qkv if sd.prefix_live else self.cache
        return src[sd.cache_row:sd.cache_row + sd.p0] if sd.p0 else self.qkv[:0]

    def max_v(self):
        m = 0.0
        for s in range(self.lay.n_seq):
            for a in (self.own(s), self.prefix(s)):
                if a.size:
                    m = max(m, float(np.abs(a[:, 2 * self.d:]).max()))
        return m


SELECT_FAMILIES = (
    ("diag", lambda i, p0: i),
    ("zero", lambda i, p0: 0 * i),
    ("prev", lambda i, p0: i - 1),
    ("future", lambda i, p0: i + 5),          # a future key is best: the causal mask must pick i
    ("cache_last", lambda i, p0: 0 * i + p0 - 1),
    ("own_first", lambda i, p0: 0 * i + p0),
    ("tile_m1", lambda i, p0: 16 * (i // 16) - 1),
    ("tile_p1", lambda i, p0: 16 * (i // 16) + 1),
    ("chunk_127", lambda i, p0: 0 * i + 127),
    ("chunk_128", lambda i, p0: 0 * i + 128),
    ("scatter", lambda i, p0: (i * 2654435761 + 12345) % 1000003 % (i + 1)),
)
SELECT_ROTS = (0, 1, 2)
SELECT_GAIN = 4096.0


def select_dims(d_head):
    """(a, a + 1) once in each non-rotary lane group's dims, including the last two."""
    return (d_head // 4, d_head // 2 + 1, d_head - 2)


def select_plan(d_head, n_heads, s, h, rot):
    """(family index, a) of head h of sequence s.  a depends on the head alone: a follower reads its
    leader's K rows."""
    return (s * n_heads + h + 4 * rot) % len(SELECT_FAMILIES), select_dims(d_head)[(h + rot) % 3]


ROW_T = (15, 33, 129, 300)  # single-query launches (batch_rows)


def select_launches():
    """(maxT, single-query launch, rotation) of every select launch test_gpu_attention.py runs per model."""
    return ([(t, False, r) for t in ALL_T for r in SELECT_ROTS] +
            [(t, True, r) for t in ROW_T for r in SELECT_ROTS])


def make(kind, d_head, n_heads, lay, seed=0, rot=0):
    """kind: random | random_gain | uniform | rotary_only | huge | range | range_below | select."""
    H, DH, d = n_heads, d_head, d_head * n_heads
    qkv = np.full((lay.rows, 3 * d), np.nan, dtype=np.float32)
    cache = np.full((lay.cache_rows, 3 * d), np.nan, dtype=np.float32)
    expect = {}
    for s, sd in enumerate(lay.seqs):
        T = sd.p0 + sd.n
        # values by absolute position; a follower's prefix is its leader's rows, a cache prefix its own
        rng = np.random.default_rng([seed, s, DH, H])
        x = rng.standard_normal((T, 3, H, DH)).astype(np.float32)
        pos = np.arange(T)
        if kind == "random_gain":
            x[:, 0] *= 4.0
        elif kind == "uniform":
            x[:, 0] = 0.0
        elif kind == "rotary_only":
            x[:, :2, :, DH // 4:] = 0.0
        elif kind == "huge":
            # one dim: q = 200, k = +-(150 + chunk) in alternating blocks of 8 keys, the first block negative:
            # scores of -+3e4 before scaling, exact in fp32, the keys of a block exactly tied; the best block
            # of a later chunk of 128 beats every earlier one, so the online softmax rescales
            x[:, :2] = 0.0
            x[:, 0, :, DH - 1] = 200.0
            x[:, 1, :, DH - 1] = (np.where((pos // 8) % 2 == 0, -1.0, 1.0) * (150.0 + pos // 128))[:, None]
        elif kind in ("range", "range_below"):
            if s == 0:
                x[0, 2] = 5000.0 if kind == "range" else 4000.0
        elif kind == "select":
            x[:, :2] = 0.0
            x[:, 2] += 3.0
            for h in range(H):
                fam, a = select_plan(DH, H, s, h, rot)
                pi = np.maximum(SELECT_FAMILIES[fam][1](pos, sd.p0), 0)
                x[:, 1, h, a] = pos
                x[:, 1, h, a + 1] = -0.5 * pos.astype(np.float64) ** 2
                x[:, 0, h, a] = SELECT_GAIN * pi
                x[:, 0, h, a + 1] = SELECT_GAIN
                expect[(s, h)] = np.minimum(pi, pos)
        else:
            assert kind == "random", kind
        x = x.reshape(T, 3 * d)
        if sd.p0 and not sd.prefix_live:
            cache[sd.cache_row:sd.cache_row + sd.p0] = x[:sd.p0]
            cache[sd.cache_row:sd.cache_row + sd.p0, :d] = np.nan  # the cache's Q columns are never read
        qkv[sd.row0:sd.row0 + sd.n] = x[sd.p0:]
    # the queries' Q only: below q0 the engine may not have computed it
    for sd in lay.seqs:
        qkv[sd.row0:sd.row0 + sd.q0, :d] = np.nan
    case = Case(kind, DH, H, lay, qkv, cache)
    if kind == "select":
        # z of query position i, head h = V of position min(pi, i), bit for bit
        z = np.full((lay.rows, d), np.nan, dtype=np.float32)
        for s, sd in enumerate(lay.seqs):
            v = np.concatenate([case.prefix(s), case.own(s)])[:, 2 * d:]
            for h in range(H):
                sel = expect[(s, h)][sd.p0 + sd.q0:]
                z[sd.row0 + sd.q0:sd.row0 + sd.n, h * DH:(h + 1) * DH] = v[sel, h * DH:(h + 1) * DH]
        case.expect = z
    return case


# ------------------------------------------------- the reference and its restatements
def _rotary(x, pos, cos, sin, DH, sign=1.0):
    """TL rotate-half on dims [0, DH / 4) of x [L][H][DH] at positions pos [L]."""
    rd, half = DH // 4, DH // 8
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    x0, x1 = x[..., :half], x[..., half:rd]
    out = x.clone()
    out[..., :half] = x0 * c[..., :half] - x1 * s[..., :half]
    out[..., half:rd] = x1 * c[..., half:] + sign * x0 * s[..., half:]
    return out


def _attend(case, cos, sin, dtype, form, mutate=None):
    """z [rows][d] (NaN outside the query rows) in ``dtype``.  form "plain": scores, mask, softmax, P V;
    "chunked": head dims reversed in the dot products, keys in chunks of 128, online softmax.
    mutate (fp64 reference only): one of MUTATIONS, a subtly wrong attention."""
    H, DH, d = case.n_heads, case.d_head, case.d
    cos, sin = torch.as_tensor(cos).to(dtype), torch.as_tensor(sin).to(dtype)
    out = torch.full((case.lay.rows, d), float("nan"), dtype=dtype)
    inv = torch.tensor(1.0 / math.sqrt(DH), dtype=dtype)
    for s, sd in enumerate(case.seqs):
        T = sd.p0 + sd.n
        kv = torch.as_tensor(np.concatenate([case.prefix(s), case.own(s)])).to(dtype)
        qpos = torch.arange(sd.p0 + sd.q0, T)
        kpos = torch.arange(T)
        q = torch.as_tensor(case.own(s)[sd.q0:, :d]).to(dtype).reshape(-1, H, DH)
        k, v = kv[:, d:2 * d].reshape(T, H, DH), kv[:, 2 * d:].reshape(T, H, DH)
        if mutate == "value_row" and T > 1:  # the last key's V row replaced by the one before it
            v = v.clone()
            v[T - 1] = v[T - 2]
        q = _rotary(q, qpos, cos, sin, DH)
        k = _rotary(k, torch.clamp(kpos + 1, max=N_CTX - 1) if mutate == "key_position" else kpos, cos, sin, DH,
                    sign=-1.0 if mutate == "rotary_sign" else 1.0)
        seen = kpos[None, :] <= qpos[:, None]
        if mutate == "mask":  # key < query position (position 0 still sees itself)
            seen = (kpos[None, :] < qpos[:, None]) | (kpos[None, :] == 0)
        if form == "plain":
            sc = torch.einsum("qhe,khe->hqk", q, k) * inv
            sc = sc.masked_fill(~seen[None], float("-inf"))
            z = torch.einsum("hqk,khe->qhe", torch.softmax(sc, dim=-1), v)
        else:
            perm = torch.arange(DH - 1, -1, -1)
            qp, kp = q[..., perm].contiguous(), k[..., perm].contiguous()
            m = torch.full((H, len(qpos)), float("-inf"), dtype=dtype)
            l = torch.zeros((H, len(qpos)), dtype=dtype)
            acc = torch.zeros((H, len(qpos), DH), dtype=dtype)
            for k0 in range(0, T, 128):
                sc = torch.einsum("qhe,khe->hqk", qp, kp[k0:k0 + 128]) * inv
                sc = sc.masked_fill(~seen[None, :, k0:k0 + 128], float("-inf"))
                m_new = torch.maximum(m, sc.max(-1).values)
                scale = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - m_new))
                p = torch.exp(sc - m_new[..., None])
                l = l * scale + p.sum(-1)
                acc = acc * scale[..., None] + torch.einsum("hqk,khe->hqe", p, v[k0:k0 + 128])
                m = m_new
            z = (acc / l[..., None]).permute(1, 0, 2)
        out[sd.row0 + sd.q0:sd.row0 + sd.n] = z.reshape(-1, d)
    return out.numpy()


MUTATIONS = ("mask", "rotary_sign", "key_position", "value_row")


def reference(case, cos, sin, mutate=None):
    """fp64 z [rows][d]; NaN in the rows that are no query."""
    return _attend(case, cos, sin, torch.float64, "plain", mutate)


def restate_plain(case, cos, sin):
    return _attend(case, cos, sin, torch.float32, "plain")


def restate_chunked(case, cos, sin):
    return _attend(case, cos, sin, torch.float32, "chunked")


def query_rows(lay, lo=0, hi=None):
    """The query rows of sequences [lo, hi)."""
    m = np.zeros(lay.rows, dtype=bool)
    for sd in lay.seqs[lo:hi]:
        m[sd.row0 + sd.q0:sd.row0 + sd.n] = True
    return m


def max_err(z, z64, lay, lo=0, hi=None):
    """max |z - z64| over the query rows of sequences [lo, hi) (NaN counts as infinite)."""
    q = query_rows(lay, lo, hi)
    if not q.any():
        return 0.0
    e = np.abs(z[q].astype(np.float64) - z64[q])
    return float("inf") if np.isnan(e).any() else float(e.max())


def bar(case, cos, sin, z64=None):
    """(bar, err of the plain fp32 restatement, err of the chunked one)."""
    z64 = reference(case, cos, sin) if z64 is None else z64
    e1 = max_err(restate_plain(case, cos, sin), z64, case.lay)
    e2 = max_err(restate_chunked(case, cos, sin), z64, case.lay)
    return max(BAR_MARGIN * max(e1, e2), BAR_FLOOR * case.max_v()), e1, e2


def select_is_exact(case, cos, sin):
    """The fp32 softmax of a select case is exactly one-hot and P V is V[pi] bit for bit (plain order and
    chunked online softmax)."""
    q = query_rows(case.lay)
    return all(np.array_equal(f(case, cos, sin)[q], case.expect[q]) for f in (restate_plain, restate_chunked))
