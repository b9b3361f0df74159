"""CPU: the per-source-token attribution cases of tests/source_cases.py — the fp64
reference is tied to the fp64 tiny oracle (its per-key terms sum to the oracle's
own hook_result . u / sigma), the exact kinds are exact in both fp32
restatements, the bar separates the reference from every mutation of it, and the
NaN rows are where the module says they are."""
import math

import numpy as np
import pytest
import torch

import attention_cases as A
import pattern_cases as P
import source_cases as S
from conftest import make_oracle

MODEL_IDS = [f"dh{dh}h{h}" for dh, h in A.MODELS]
LENS = (1, 5, 17)
MID = (0, 2, 8)
TARGETS = (5, 77, 300)
CONTRAST = (9, 3, 411)


def tables(d_head):
    return A.tables(d_head)


def oracle_qkv(oracle, cache, l):
    """(q, k, v) [T, d] before rotary, recomputed from the oracle's cached hook_resid_pre with its own _ln_pre,
    W_Q / W_K / W_V and biases (as test_gpu_attention_pattern.oracle_qkv_pattern does)."""
    b = oracle.w["blocks"][l]
    x = oracle._ln_pre(cache[f"blocks.{l}.hook_resid_pre"])
    q = torch.einsum("bpd,hde->bphe", x, b["W_Q"]) + b["b_Q"]
    k = torch.einsum("bpd,hde->bphe", x, b["W_K"]) + b["b_K"]
    v = torch.einsum("bpd,hde->bphe", x, b["W_V"]) + b["b_V"]
    T = x.shape[1]
    return tuple(t[0].reshape(T, -1).numpy() for t in (q, k, v))


@pytest.mark.parametrize("contrast", (None, CONTRAST), ids=("target", "contrast"))
@pytest.mark.parametrize("pos", (None, MID), ids=("last", "mid"))
def test_reference_sums_to_the_oracles_head_attribution(tiny_cfg, tiny_sd, tokenizer, pos, contrast):
    """In fp64, from the oracle's own rows: sum_j src[j] = hook_result[q, h] . u / sigma to 1e-12, and the pattern
    inside the reference is the one the oracle's own _rotate gives."""
    o = make_oracle(tiny_cfg, tiny_sd, tokenizer, torch.float64)
    o.cfg.use_attn_result = True  # (this test's own oracle: hook_result is cached)
    cfg = tiny_cfg
    H, DH, d, nl = cfg.n_heads, cfg.d_head, cfg.d_model, cfg.n_layers
    cos, sin = A.tables(DH, n_ctx=cfg.n_ctx, base=cfg.rotary_base, dtype=torch.float64)
    g = torch.Generator().manual_seed(7)
    for s, T in enumerate(LENS):
        ids = [0] + torch.randint(1, cfg.d_vocab, (T - 1,), generator=g).tolist()
        q = T - 1 if pos is None else pos[s]
        _, cache = o.run_with_cache(torch.tensor([ids]))
        xL = cache[f"blocks.{nl - 1}.hook_resid_post"][0, q]
        xc = xL - xL.mean()
        sigma = (xc.pow(2).mean() + o.cfg.eps).sqrt()
        u = o.w["W_U"][:, TARGETS[s]] - (o.w["W_U"][:, contrast[s]] if contrast is not None else 0)
        for l in range(nl):
            b = o.w["blocks"][l]
            assert not b["b_V"].any(), "the processed model has b_V = 0: z is a pattern-weighted sum of V rows"
            W = b["W_O"].reshape(d, d).T.numpy()  # [c][h dh + k]
            qq, kk, vv = oracle_qkv(o, cache, l)
            case = S.from_rows(qq, kk, vv, [T], [q], DH, H, W, u.numpy()[None], sigma.numpy()[None], dtype=np.float64)
            src = S.reference_from_model(case, cos, sin)[0]
            want = (cache[f"blocks.{l}.attn.hook_result"][0, q] @ (u / sigma)).numpy()
            scale = max(1.0, np.abs(src).sum(-1).max())
            assert np.abs(src.sum(-1) - want).max() <= 1e-12 * scale, (s, l)
            assert (src[:, q + 1:] == 0).all()
            rq, rk = (o._rotate(torch.from_numpy(a).reshape(1, T, H, DH)) for a in (qq, kk))
            p = torch.softmax(torch.einsum("bqhe,bkhe->bhqk", rq, rk)[0, :, q, :q + 1] / math.sqrt(DH), -1).numpy()
            assert np.abs(P.reference(case, cos, sin)[0][:, :q + 1] - p).max() <= 1e-12
            # the reference from the given (fp32-rounded) g: within half an ulp of g per term
            t = (P.reference(case, cos, sin) * S.terms(case))[0]
            assert (np.abs(S.reference(case, cos, sin)[0] - src) <= S.EPS24 * t * 1.001 + 1e-300).all()


@pytest.mark.parametrize("model", A.MODELS, ids=MODEL_IDS)
def test_every_mutation_moves_the_reference_beyond_the_bar(model):
    cos, sin = tables(model[0])
    case = S.make("random", model[0], model[1], 17)
    ref = S.reference(case, cos, sin)
    bar, e1, e2 = S.bar(case, cos, sin, ref)
    assert 0 < max(e1, e2) <= bar < 1e-4 * np.abs(ref).max()
    for mutate in S.MUTATIONS:
        moved = S.max_err(S.reference(case, cos, sin, mutate), ref)
        assert moved > 100 * bar, (model, mutate, moved, bar)
    with pytest.raises(ValueError):
        S.reference(case, cos, sin, "no_such_mutation")


@pytest.mark.parametrize("model", A.MODELS, ids=MODEL_IDS)
def test_exact_kinds_are_exact_in_both_restatements(model):
    DH, H = model
    cos, sin = tables(DH)
    for T in (1, 17, 65):
        for rot in A.SELECT_ROTS:
            case = S.make("select", DH, H, T, rot=rot)
            want = S.select_exact(case)
            assert P.select_is_exact(case, cos, sin)
            for f in (S.restate_pattern, S.restate_result):
                got = f(case, cos, sin)
                assert np.array_equal(got, want), (T, rot, f.__name__)  # (-0.0 == +0.0)
            hot = want != 0
            assert hot.sum() == case.lay.n_seq * H  # one key per (sequence, head); V = N(3, 1) is not 0 here
            assert np.array_equal(S.reference(case, cos, sin).astype(np.float32), want)
        case = S.make("unit", DH, H, T)
        for f, pat in ((S.restate_pattern, P.restate_plain), (S.restate_result, P.restate_chunked)):
            assert np.array_equal(f(case, cos, sin).view(np.int32), pat(case, cos, sin).view(np.int32))
        assert np.array_equal(S.reference(case, cos, sin), P.reference(case, cos, sin))
        case = S.make("zero", DH, H, T)
        assert not S.reference(case, cos, sin).any() and not S.restate_pattern(case, cos, sin).any()
        assert not S.restate_result(case, cos, sin).any()
        assert S.bar(case, cos, sin)[0] == 0.0  # (compared exactly, not at the bar)


@pytest.mark.parametrize("model", A.MODELS, ids=MODEL_IDS)
def test_layout_and_nan_rows(model):
    DH, H = model
    d = DH * H
    for kind in S.KINDS:
        case = S.make(kind, DH, H, 17)
        assert case.qkv.dtype == np.float32 and case.g.dtype == np.float32 and case.g.shape == (3, d)
        assert list(case.qpos) == [16, 8, 0] and case.maxT == 17
        used = np.zeros(case.lay.rows, dtype=bool)
        for sd in case.seqs:
            keys = slice(sd.row0, sd.row0 + sd.q0 + 1)
            used[sd.row0:sd.row0 + sd.n] = True
            assert not np.isnan(case.qkv[keys, d:]).any()                       # K and V of the keys <= q
            assert not np.isnan(case.qkv[sd.row0 + sd.q0, :d]).any()             # the query's Q
            assert np.isnan(case.qkv[sd.row0 + sd.q0 + 1:sd.row0 + sd.n, 2 * d:]).all()  # V past the query
            assert not np.isnan(case.qkv[sd.row0:sd.row0 + sd.n, d:2 * d]).any()  # (their K exists)
            q_rows = np.ones(sd.n, dtype=bool)
            q_rows[sd.q0] = False
            assert np.isnan(case.qkv[sd.row0:sd.row0 + sd.n, :d][q_rows]).all()  # every other Q
        assert np.isnan(case.qkv[~used]).all()  # the rows between the sequences
        # g is what (u / sigma) @ W_O rounds to
        g64 = (case.u.astype(np.float64) / case.sigma.astype(np.float64)[:, None]) @ case.W[:, :d].astype(np.float64)
        assert np.array_equal(case.g, g64.astype(np.float32))
    cos, sin = tables(DH)
    case = S.make("random_gain", DH, H, 17)
    ref = S.reference(case, cos, sin)
    for s, q in enumerate(case.qpos):
        assert not ref[s, :, q + 1:].any() and ref[s, :, :q + 1].all()
    cls = S.classes(case)
    sums = S.class_sums(ref, case, cls)
    counted = np.stack([ref[s, :, :q + 1][:, cls[r:r + q + 1] >= 0].sum(-1) for s, (q, r) in enumerate(zip(case.qpos, case.row0))])
    assert np.abs(sums.sum(-1) - counted).max() <= 1e-12 * np.abs(ref).sum(-1).max()


def test_unit_dims_hit_every_chain():
    for DH, _ in A.MODELS:
        dims = S.unit_dims(DH)
        assert len(set(dims)) == 4 and max(dims) == DH - 1 and math.prod(e % 4 + 1 for e in dims) == 24
