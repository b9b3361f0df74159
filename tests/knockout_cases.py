"""Attention-knockout launches with known answers, their fp64 reference and the
bar (shared by test_knockout_cases.py and test_gpu_knockout.py; a plain module,
not a conftest).

The primitive (tvr_attention_knockout, csrc/attention_knockout.hpp): for an item
(sequence, head, blocked keys B) the z slice of the sequence's LAST row is the
attention of that query over the keys j <= q, j not in B.  ``reference`` states
it in fp64 as a softmax over the gathered unblocked keys; the bar of a launch
comes from two fp32 restatements of the same function — ``restate_plain``
(scores masked_fill'ed with -inf, softmax, P V) and ``restate_online`` (keys one
by one, a running max / sum / accumulator, a blocked key skipped) — never from
the engine: bar = BAR_MARGIN x the larger of their max |z - z64|, floored at
BAR_FLOOR max |V| (attention_cases.bar's rule and constants).

The layouts and values are attention_cases': rows that belong to no sequence and
every Q the kernel has no business reading are NaN.

The oracle-side knockout needs no change under oracle/: one run_with_hooks call
in which a ``hook_resid_pre`` hook records the layer's residual and a ``hook_z``
hook replaces z[0, -1, h] of the members by the masked recomputation from
``oracle.w``, ``_ln_pre`` and ``_rotate``.
"""
from __future__ import annotations

import collections
import math

import numpy as np
import torch

import attention_cases as A

MODELS = A.MODELS
ALL_T = (2, 15, 16, 17, 33, 64, 65, 129, 300)
FAMILIES = ("first", "last", "argmax", "every_other", "all_but_one", "word_boundary", "empty")
BAR_MARGIN, BAR_FLOOR = A.BAR_MARGIN, A.BAR_FLOOR

# one item: the last row of sequence `seq`, one head, the blocked key positions (sorted)
Item = collections.namedtuple("Item", "seq head keys")


def layout(T):
    """A whole sequence (p0 = 0, only its last row a query), one computed row behind a cache prefix
    (n = 1, p0 = T - 1: the patched last-position forwards) and a follower of the first sequence."""
    lay = A.Layout().add(T, q0=T - 1)
    lay.add(T, p0=T - 1)
    p0 = max(p for p in (1, 5, 16, 23) if p < T)
    lay.add(T, p0=p0, q0=T - p0 - 1, leader=0)
    lay.row_from = 0
    return lay


def make(model, T, kind="random"):
    return A.make(kind, model[0], model[1], layout(T), seed=1000 + T)


def _qkv_last(case, s, cos, sin, dtype):
    """(q [H][DH] rotated, k [T][H][DH] rotated, v [T][H][DH]) of sequence s' last query in ``dtype``."""
    H, DH, d = case.n_heads, case.d_head, case.d
    sd = case.seqs[s]
    T = sd.p0 + sd.n
    cos, sin = torch.as_tensor(cos).to(dtype), torch.as_tensor(sin).to(dtype)
    kv = torch.as_tensor(np.concatenate([case.prefix(s), case.own(s)])).to(dtype)
    q = torch.as_tensor(case.own(s)[-1:, :d]).to(dtype).reshape(1, H, DH)
    k, v = kv[:, d:2 * d].reshape(T, H, DH), kv[:, 2 * d:].reshape(T, H, DH)
    q = A._rotary(q, torch.tensor([T - 1]), cos, sin, DH)[0]
    k = A._rotary(k, torch.arange(T), cos, sin, DH)
    return q, k, v


def scores64(case, s, cos, sin):
    """fp64 scaled scores [H][T] of sequence s' last query."""
    q, k, _ = _qkv_last(case, s, cos, sin, torch.float64)
    return torch.einsum("he,khe->hk", q, k) / math.sqrt(case.d_head)


def blocked_set(family, T, best):
    """The blocked keys of one family for a query over T keys whose best key is ``best``; None where the
    family does not exist at this T (it would block every key, or nothing but what "empty" blocks)."""
    if family == "first":
        ks = [0]
    elif family == "last":
        ks = [T - 1]
    elif family == "argmax":
        ks = [int(best)]
    elif family == "every_other":
        ks = list(range(0, T, 2))
    elif family == "all_but_one":
        ks = [j for j in range(T) if j != T // 2]
    elif family == "word_boundary":
        ks = list(range(28, min(36, T)))
    else:
        assert family == "empty", family
        return []
    return ks if 0 < len(ks) < T else None


def items_of(case, family, cos, sin):
    """One item per (sequence, head) of the launch (argmax: the head's own best key)."""
    out = []
    for s, sd in enumerate(case.seqs):
        T = sd.p0 + sd.n
        best = scores64(case, s, cos, sin).argmax(-1) if family == "argmax" else [0] * case.n_heads
        for h in range(case.n_heads):
            ks = blocked_set(family, T, best[h])
            if ks is not None:
                out.append(Item(s, h, tuple(ks)))
    return out


def _knocked(case, items, cos, sin, dtype, form):
    """z slices [n_items][DH] in ``dtype``.  form: "gather" (softmax over the unblocked keys alone),
    "plain" (-inf scores, softmax over all, P V), "online" (one key at a time, blocked keys skipped)."""
    DH = case.d_head
    out = torch.zeros((len(items), DH), dtype=dtype)
    pattern = []
    inv = torch.tensor(1.0 / math.sqrt(DH), dtype=dtype)
    cache = {}
    for x, it in enumerate(items):
        if it.seq not in cache:
            cache[it.seq] = _qkv_last(case, it.seq, cos, sin, dtype)
        q, k, v = cache[it.seq]
        T = k.shape[0]
        q, k, v = q[it.head], k[:, it.head], v[:, it.head]
        keep = torch.ones(T, dtype=torch.bool)
        if it.keys:
            keep[list(it.keys)] = False
        if form == "gather":
            p = torch.zeros(T, dtype=dtype)
            p[keep] = torch.softmax((k[keep] @ q) * inv, 0)
            out[x] = p[keep] @ v[keep]
            pattern.append(p)
        elif form == "plain":
            sc = ((k @ q) * inv).masked_fill(~keep, float("-inf"))
            out[x] = torch.softmax(sc, 0) @ v
        else:
            assert form == "online", form
            qp, kp = q.flip(0), k.flip(1)  # another order of the dot product
            m, l, acc = None, torch.zeros((), dtype=dtype), torch.zeros(DH, dtype=dtype)
            for j in range(T):
                if not keep[j]:
                    continue
                sc = (kp[j] @ qp) * inv
                m_new = sc if m is None else torch.maximum(m, sc)
                scale = torch.zeros((), dtype=dtype) if m is None else torch.exp(m - m_new)
                p = torch.exp(sc - m_new)
                l = l * scale + p
                acc = acc * scale + p * v[j]
                m = m_new
            out[x] = acc / l
    return out.numpy(), pattern


def reference(case, items, cos, sin):
    """fp64 z slices [n_items][DH]."""
    return _knocked(case, items, cos, sin, torch.float64, "gather")[0]


def pattern64(case, items, cos, sin):
    """The knocked fp64 patterns, one [T] per item."""
    return _knocked(case, items, cos, sin, torch.float64, "gather")[1]


def restate_plain(case, items, cos, sin):
    return _knocked(case, items, cos, sin, torch.float32, "plain")[0]


def restate_online(case, items, cos, sin):
    return _knocked(case, items, cos, sin, torch.float32, "online")[0]


def bar(case, items, cos, sin, z64=None):
    """(bar, err of the plain fp32 restatement, err of the online one)."""
    z64 = reference(case, items, cos, sin) if z64 is None else z64
    e1 = float(np.abs(restate_plain(case, items, cos, sin).astype(np.float64) - z64).max())
    e2 = float(np.abs(restate_online(case, items, cos, sin).astype(np.float64) - z64).max())
    return max(BAR_MARGIN * max(e1, e2), BAR_FLOOR * case.max_v()), e1, e2


def tables_of(items):
    """(items [n][4] int64 rows (seq, head mask, first_key, n_keys), keys int32) as the op takes them."""
    rows, keys = [], []
    for it in items:
        rows.append((it.seq, 1 << it.head, len(keys), len(it.keys)))
        keys += list(it.keys)
    return np.asarray(rows, dtype=np.int64).reshape(-1, 4), np.asarray(keys, dtype=np.int32)


# ----------------------------------------------------------------- select (bitwise)
def make_select(model, T):
    """One-hot scores (attention_cases' "select" construction on the last query): head h's best key is
    b = (3 h + 1) % T, its runner-up r = (b + 1 + h) % T (r != b for T >= H + 2), every other key far
    below.  With b blocked the slice is V[r] bit for bit.  Returns (case, items, expect [n_items][DH])."""
    DH, H = model
    d = DH * H
    case = A.make("random", DH, H, layout(T), seed=77 + T)
    items, expect = [], []
    for s, sd in enumerate(case.seqs):
        rows = np.concatenate([case.prefix(s), case.own(s)])  # views' copies: write back below
        pos = np.arange(T, dtype=np.float64)
        for h in range(H):
            a = A.select_dims(DH)[h % 3]
            b = (3 * h + 1) % T
            r = (b + 1 + h % (T - 1)) % T
            assert r != b
            # key score(j) = GAIN * (w_j): w = 2 at b, 1 at r, -|j| - 2 elsewhere, through two non-rotary dims
            w = -(pos + 2.0)
            w[b], w[r] = 2.0, 1.0
            k = rows[:, d + h * DH:d + (h + 1) * DH]
            k[:] = 0.0
            k[:, a] = w
            q = rows[-1, h * DH:(h + 1) * DH]
            q[:] = 0.0
            q[a] = A.SELECT_GAIN
            items.append(Item(s, h, (b,)))
            expect.append(rows[r, 2 * d + h * DH:2 * d + (h + 1) * DH].copy())
        # the Q of rows that are no query stays NaN: only K and the last Q were written
        if sd.p0 and not sd.prefix_live:
            case.cache[sd.cache_row:sd.cache_row + sd.p0, d:] = rows[:sd.p0, d:]
        case.qkv[sd.row0:sd.row0 + sd.n, d:] = rows[sd.p0:, d:]  # (a follower's prefix: its leader's rows, same pattern)
        case.qkv[sd.row0 + sd.n - 1, :d] = rows[-1, :d]
    return case, items, np.stack(expect)


# ------------------------------------------------------------- the oracle-side knockout
def knocked_z(oracle, l, resid, heads, keys):
    """hook_z[0, -1, h] for h in ``heads`` of layer l with the last query's scores to ``keys`` at -inf,
    recomputed from the layer's hook_resid_pre [1, T, d]: {h: [d_head]}."""
    b = oracle.w["blocks"][l]
    x = oracle._ln_pre(resid)
    q = torch.einsum("bpd,hde->bphe", x, b["W_Q"]) + b["b_Q"]
    k = torch.einsum("bpd,hde->bphe", x, b["W_K"]) + b["b_K"]
    v = torch.einsum("bpd,hde->bphe", x, b["W_V"]) + b["b_V"]
    q, k = oracle._rotate(q), oracle._rotate(k)
    T = x.shape[1]
    keep = torch.ones(T, dtype=torch.bool)
    if len(keys):
        keep[list(keys)] = False
    out, pat = {}, {}
    for h in heads:
        sc = (k[0, keep, h] @ q[0, -1, h]) / math.sqrt(oracle.cfg.d_head)
        p = torch.zeros(T, dtype=x.dtype)
        p[keep] = torch.softmax(sc, 0)
        out[h], pat[h] = p[keep] @ v[0, keep, h], p
    return out, pat


def knockout_hooks(oracle, members, keys):
    """run_with_hooks hooks of one knockout: members [(layer, head)], keys the blocked positions."""
    by_layer = collections.defaultdict(list)
    for l, h in members:
        by_layer[l].append(h)
    hooks, resid = [], {}
    if not keys:
        return hooks
    for l, heads in by_layer.items():
        def rec(x, hook, l=l):
            resid[l] = x.clone()

        def put(z, hook, l=l, heads=heads):
            new, _ = knocked_z(oracle, l, resid[l], heads, keys)
            for h in heads:
                z[0, -1, h] = new[h]
            return z
        hooks += [(f"blocks.{l}.hook_resid_pre", rec), (f"blocks.{l}.attn.hook_z", put)]
    return hooks


def knocked_logits(oracle, prompt, members, keys):
    """Last-position logits of ``prompt`` under the knockout (members, keys)."""
    return oracle.run_with_hooks(torch.tensor([list(prompt)]), fwd_hooks=knockout_hooks(oracle, members, keys))[0, -1]


def masked_forward_logits(oracle, prompt, members, keys):
    """The same, written independently: a full forward whose attention scores are masked_fill'ed."""
    w, cfg = oracle.w, oracle.cfg
    mem = set(members)
    resid = w["W_E"][torch.tensor([list(prompt)])]
    T = resid.shape[1]
    causal = torch.triu(torch.ones(T, T, dtype=torch.bool), diagonal=1)
    for l in range(cfg.n_layers):
        b = w["blocks"][l]
        x = oracle._ln_pre(resid)
        q = oracle._rotate(torch.einsum("bpd,hde->bphe", x, b["W_Q"]) + b["b_Q"])
        k = oracle._rotate(torch.einsum("bpd,hde->bphe", x, b["W_K"]) + b["b_K"])
        v = torch.einsum("bpd,hde->bphe", x, b["W_V"]) + b["b_V"]
        sc = torch.einsum("bqhe,bkhe->bhqk", q, k) / math.sqrt(cfg.d_head)
        sc = sc.masked_fill(causal, float("-inf"))
        for h in range(cfg.n_heads):
            if (l, h) in mem and keys:
                sc[0, h, -1, list(keys)] = float("-inf")
        z = torch.einsum("bkhe,bhqk->bqhe", v, torch.softmax(sc, -1))
        attn = z.reshape(1, T, -1) @ b["W_O"].reshape(-1, cfg.d_model) + b["b_O"]
        mlp = torch.nn.functional.gelu(x @ b["W_in"] + b["b_in"]) @ b["W_out"] + b["b_out"]
        resid = resid + attn + mlp
    return (oracle._ln_pre(resid) @ w["W_U"] + w["b_U"])[0, -1]


# ------------------------------------------------------------- the end-to-end cases
E2E_LENS = (3, 7, 12, 30)
LOGIT_TOL, PROB_TOL, BF16_TOL = 1e-4, 1e-5, 2e-2  # tests/test_gpu_engine.py's bars


def e2e_prompts(cfg):
    g = torch.Generator().manual_seed(21)
    return [[0] + torch.randint(1, cfg.d_vocab, (n - 1,), generator=g).tolist() for n in E2E_LENS]


def e2e_cases(cfg, T):
    """(members, blocked keys) of one prompt of T tokens: members in one layer, in several layers
    including the last, all heads of a window; the BOS key, self, all but one key.  Every case has to move
    the fp64 logits by more than 100 x LOGIT_TOL (test_knockout_cases.py's negative control).  The d_head 80
    config's last token puts too little attention on BOS or on itself alone for that (1e-5 .. 3e-3 of
    max |logit|, fp64), so there the BOS block takes the first half of the prompt with it and the self block
    the second half; tiny4 blocks the single keys."""
    L, H = cfg.n_layers, cfg.n_heads
    wide = cfg.d_head == 80
    bos = list(range(0, max(1, T // 2))) if wide else [0]
    own = list(range(T // 2 + 1 if T > 3 else T - 1, T)) if wide else [T - 1]
    layer1 = [(1, h) for h in range(H)] if wide else [(1, 2), (1, 0)]
    several = [(0, h) for h in range(H)] + [(1, 3), (L - 1, 0)] if wide else [(0, 1), (1, 3), (L - 1, 0)]
    window = [(l, h) for l in range(min(1, L - 1), L) for h in range(H)]
    return [(layer1, bos),
            (several, own),
            (window, bos),
            (window, [j for j in range(T) if j != T // 2]),
            ([(0, h) for h in range(H)] + [(L - 1, 2)], list(range(0, T - 1))),
            ([(L - 1, h) for h in range(H)], list(range(0, T, 2)))]


# ------------------------------------------------------------- the façade's inputs and reference
FACADE_MARGIN = 4e-4  # accuracy is compared on prompts whose fp64 top-1 margin exceeds this x max |logit|
FACADE_LENS = (5, 9, 14, 6, 11, 20, 8, 16)
FACADE_WINDOWS = ((0, 1), (1, 3), (2, 2))
ROLE_SEED, ROLE_PROMPTS, ROLE_NAMES = 3, 8, ("bos", "demo_label", "separator")


def facade_inputs(cfg, o64):
    """(prompts, answers, blocked, windows) of the attention_knockout_effect test: 8 random prompts; the
    answer of every other prompt is the fp64 clean top-1 (so accuracies are not all zero), else token 1 of
    the prompt; blocked alternates between {BOS, the middle key} and every odd key before the last."""
    g = torch.Generator().manual_seed(33)
    prompts = [[0] + torch.randint(1, cfg.d_vocab, (n - 1,), generator=g).tolist() for n in FACADE_LENS]
    answers = [int(o64(torch.tensor([p]))[0, -1].argmax()) if i % 2 == 0 else p[1] for i, p in enumerate(prompts)]
    blocked = [[0, len(p) // 2] if i % 2 else list(range(1, len(p) - 1, 2)) for i, p in enumerate(prompts)]
    return prompts, answers, blocked, list(FACADE_WINDOWS)


def oracle_effect(o64, prompts, answers, blocked, windows, heads):
    """The loop attention_knockout_effect replaces: per prompt and window one hooked forward (fp64)."""
    H = o64.cfg.n_heads
    hs = list(range(H)) if heads is None else list(heads)
    n, W = len(prompts), len(windows)
    p_clean, p_ko = np.zeros(n), np.zeros((n, W))
    margin_ok, top_ko = np.zeros((n, W), bool), np.zeros((n, W), bool)

    def margin(lg):
        t = torch.topk(lg, 2).values
        return ((t[0] - t[1]) > FACADE_MARGIN * lg.abs().max()).item()

    for i, p in enumerate(prompts):
        lg = o64(torch.tensor([list(p)]))[0, -1]
        p_clean[i] = torch.softmax(lg, 0)[answers[i]].item()
        for w, (a, b) in enumerate(windows):
            members = [(l, h) for l in range(a, b + 1) for h in hs]
            lg = knocked_logits(o64, p, members, sorted(set(blocked[i])))
            p_ko[i, w] = torch.softmax(lg, 0)[answers[i]].item()
            margin_ok[i, w], top_ko[i, w] = margin(lg), lg.argmax().item() == answers[i]
    return dict(p_clean=p_clean, p_ko=p_ko, margin_ok=margin_ok, top_ko=top_ko)
