"""Attention-pattern launches with known answers, their fp64 reference and the
bar (shared by test_pattern_cases.py and test_gpu_attention_pattern.py; a plain
module, not a conftest).

A launch is three whole sequences (p0 = 0) of attention_cases' layout, each
with ONE query row, ``q0``: a sequence of T positions queried at its last row,
one of T positions queried mid-sequence (q = T // 2: the later K rows exist and
must be ignored, their pattern columns zero-filled), and one of a single
position.  Values come from ``attention_cases.make``; on top of its NaN rows
(the row after every sequence, the Q of rows below q0) the Q columns of EVERY
row that is not its sequence's query are NaN here: a kernel that reads a Q or a
row it has no business reading returns NaN.

``reference`` is the pattern in fp64: TL rotate-half rotary on dims
[0, d_head / 4) at absolute positions, scores / sqrt(d_head), keys <= the query
position, softmax; zero beyond the query.  The bar of a case comes from two
fp32 restatements of the same function (plain; head dims reversed in the dot
products with keys in chunks of 128 and an online max / sum), never from the
engine: bar = 4 x the larger of their max |p - p64|, floored at 2^-22 — the
method and the margin attention_cases.bar argues for; a probability is at most
1, hence the floor.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import attention_cases as A

ALL_T = (1, 15, 16, 17, 63, 64, 65, 129, 300)  # lane-count edges 63 / 64 / 65; a second, third and fifth pass
KINDS = ("random", "random_gain", "uniform", "rotary_only", "huge")
BAR_MARGIN = A.BAR_MARGIN
BAR_FLOOR = 2.0 ** -22
N_CLASSES = 3
MUTATIONS = ("mask", "rotary_sign", "key_position")


def layout(T):
    return A.Layout().add(T, q0=T - 1).add(T, q0=T // 2).add(1)


def make(kind, d_head, n_heads, T, rot=0):
    """The attention_cases.Case of the launch for T, with ``qpos`` [n_seq], ``row0`` [n_seq] and, for
    ``select``, ``hot`` [n_seq][H]: the key that holds all of the pattern."""
    lay = layout(T)
    case = A.make(kind, d_head, n_heads, lay, seed=T, rot=rot)
    d = case.d
    keep = np.zeros(lay.rows, dtype=bool)
    for sd in lay.seqs:
        keep[sd.row0 + sd.q0] = True
    case.qkv[~keep, :d] = np.nan
    case.qpos = np.asarray([sd.q0 for sd in lay.seqs], dtype=np.int32)
    case.row0 = np.asarray([sd.row0 for sd in lay.seqs], dtype=np.int32)
    case.maxT = lay.maxT
    if kind == "select":
        hot = np.zeros((lay.n_seq, n_heads), dtype=np.int64)
        for s, sd in enumerate(lay.seqs):
            for h in range(n_heads):
                fam, _ = A.select_plan(d_head, n_heads, s, h, rot)
                pi = max(int(A.SELECT_FAMILIES[fam][1](np.asarray([sd.q0]), 0)[0]), 0)
                hot[s, h] = min(pi, sd.q0)
        case.hot = hot
    return case


def from_rows(q, k, lens, qpos, d_head, n_heads):
    """A case from given Q / K rows (fp32 [tokens][d], sequences packed in order, before rotary): what
    ``reference`` and ``bar`` need to judge a pattern computed from exactly these values (a trace's own
    hook_q / hook_k).  V is zero."""
    lay = A.Layout()
    for T, qp in zip(lens, qpos):
        lay.add(int(T), q0=int(qp))
    d = d_head * n_heads
    qkv = np.full((lay.rows, 3 * d), np.nan, dtype=np.float32)
    off = 0
    for sd in lay.seqs:
        qkv[sd.row0:sd.row0 + sd.n, :d] = q[off:off + sd.n]
        qkv[sd.row0:sd.row0 + sd.n, d:2 * d] = k[off:off + sd.n]
        qkv[sd.row0:sd.row0 + sd.n, 2 * d:] = 0.0
        off += sd.n
    case = A.Case("rows", d_head, n_heads, lay, qkv, None)
    case.qpos = np.asarray(qpos, dtype=np.int32)
    case.row0 = np.asarray([sd.row0 for sd in lay.seqs], dtype=np.int32)
    case.maxT = lay.maxT
    return case


def one_hot(case, ld=None):
    """The exact pattern of a select case, fp32 [n_seq][H][ld]."""
    p = np.zeros((case.lay.n_seq, case.n_heads, ld or case.maxT), dtype=np.float32)
    for s in range(case.lay.n_seq):
        p[s, np.arange(case.n_heads), case.hot[s]] = 1.0
    return p


def _pattern(case, cos, sin, dtype, form, mutate=None):
    """[n_seq][H][maxT] in ``dtype``.  form "plain": scores, mask, softmax; "chunked": head dims reversed in
    the dot products, keys in chunks of 128, online max / sum.  mutate (fp64 reference only): a subtly wrong
    pattern."""
    H, DH, d = case.n_heads, case.d_head, case.d
    cos, sin = torch.as_tensor(cos).to(dtype), torch.as_tensor(sin).to(dtype)
    out = torch.zeros((case.lay.n_seq, H, case.maxT), dtype=dtype)
    inv = torch.tensor(1.0 / math.sqrt(DH), dtype=dtype)
    for s, sd in enumerate(case.seqs):
        T, qp = sd.n, sd.q0
        rows = torch.as_tensor(case.qkv[sd.row0:sd.row0 + T]).to(dtype)
        q = rows[qp:qp + 1, :d].reshape(1, H, DH)
        k = rows[:, d:2 * d].reshape(T, H, DH)
        kpos = torch.arange(T)
        q = A._rotary(q, torch.tensor([qp]), cos, sin, DH)
        k = A._rotary(k, torch.clamp(kpos + 1, max=A.N_CTX - 1) if mutate == "key_position" else kpos, cos, sin, DH,
                      sign=-1.0 if mutate == "rotary_sign" else 1.0)
        seen = kpos <= qp
        if mutate == "mask":  # key < query position (position 0 still sees itself)
            seen = (kpos < qp) | (kpos == 0)
        if form == "plain":
            sc = torch.einsum("qhe,khe->hk", q, k) * inv
            p = torch.softmax(sc.masked_fill(~seen[None], float("-inf")), dim=-1)
        else:
            perm = torch.arange(DH - 1, -1, -1)
            qr, kr = q[..., perm].contiguous(), k[..., perm].contiguous()
            m = torch.full((H,), float("-inf"), dtype=dtype)
            l = torch.zeros((H,), dtype=dtype)
            parts = []  # (exp(sc - the running max when the chunk was met), that max)
            for k0 in range(0, T, 128):
                sc = torch.einsum("qhe,khe->hk", qr, kr[k0:k0 + 128]) * inv
                sc = sc.masked_fill(~seen[None, k0:k0 + 128], float("-inf"))
                m_new = torch.maximum(m, sc.max(-1).values)
                scale = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - m_new))
                e = torch.exp(sc - m_new[:, None])
                l = l * scale + e.sum(-1)
                parts.append((e, m_new))
                m = m_new
            p = torch.cat([e * torch.exp(mc - m)[:, None] for e, mc in parts], dim=-1) / l[:, None]
        out[s, :, :T] = p
    return out.numpy()


def reference(case, cos, sin, mutate=None):
    """fp64 pattern [n_seq][H][maxT]; zero beyond each query position."""
    return _pattern(case, cos, sin, torch.float64, "plain", mutate)


def restate_plain(case, cos, sin):
    return _pattern(case, cos, sin, torch.float32, "plain")


def restate_chunked(case, cos, sin):
    return _pattern(case, cos, sin, torch.float32, "chunked")


def max_err(p, p64):
    e = np.abs(np.asarray(p, dtype=np.float64)[..., :p64.shape[-1]] - p64)
    return float("inf") if np.isnan(e).any() else float(e.max())


def bar(case, cos, sin, p64=None):
    """(bar, err of the plain fp32 restatement, err of the chunked one)."""
    p64 = reference(case, cos, sin) if p64 is None else p64
    e1 = max_err(restate_plain(case, cos, sin), p64)
    e2 = max_err(restate_chunked(case, cos, sin), p64)
    return max(BAR_MARGIN * max(e1, e2), BAR_FLOOR), e1, e2


def select_is_exact(case, cos, sin):
    """Both fp32 restatements of a select case are exactly one-hot: 1.0 at min(pi, qpos), 0.0 elsewhere."""
    hot = one_hot(case)
    return all(np.array_equal(f(case, cos, sin), hot) for f in (restate_plain, restate_chunked))


def classes(case):
    """One class per row of the launch's buffer in [-1, N_CLASSES): every sequence mixes the classes and -1;
    class 2 is empty in the mid-queried sequence, classes 0 and 2 in the one-position sequence."""
    cls = np.full(case.lay.rows, -1, dtype=np.int32)
    for s, sd in enumerate(case.seqs):
        c = (np.arange(sd.n) * 7 + s) % 4 - 1
        if s == 1:
            c[c == 2] = 0
        cls[sd.row0:sd.row0 + sd.n] = c
    return cls


def class_sums(p, case, cls, n_classes=N_CLASSES):
    """mass [n_seq][H][n_classes] of a pattern p [n_seq][H][>= maxT], summed in fp64 over the keys <= the query
    position by the class of their row; class -1 is counted nowhere."""
    p = np.asarray(p, dtype=np.float64)
    out = np.zeros((case.lay.n_seq, case.n_heads, n_classes), dtype=np.float64)
    for s, sd in enumerate(case.seqs):
        c = cls[sd.row0:sd.row0 + sd.q0 + 1]
        for k in range(n_classes):
            out[s, :, k] = p[s, :, :sd.q0 + 1][:, c == k].sum(-1)
    return out
