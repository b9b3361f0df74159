"""CPU: the attribution cases, their fp64 reference and the bar stand on their
own — the reference reproduces TransformerLens' decomposition on the fp64 tiny
oracle (heads from hook_result, the rest of a layer from hook_attn_out and
hook_mlp_out, and the parts add up to the logit difference), the bars are finite
and positive, the exact cases are exact in both fp32 restatements."""
import numpy as np
import pytest
import torch

import attention_cases as A
import attribution_cases as C
from conftest import make_oracle

LENS = (6, 9, 4)
EPS = 1e-5


def ragged_prompts(cfg, lens, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [[0] + torch.randint(1, cfg.d_vocab, (n - 1,), generator=g).tolist() for n in lens]


@pytest.fixture(scope="module")
def oracle64(tiny_cfg, tiny_sd, tokenizer):
    o = make_oracle(tiny_cfg, tiny_sd, tokenizer, torch.float64)
    o.cfg.use_attn_result = True  # (this module's own oracle: hook_result is cached)
    return o


def oracle_arrays(o, seqs, qpos):
    """What ``attribution`` takes, from the oracle's cache: x [L + 1][n][d], z [L][n][d], plus the oracle's own
    hook_result / hook_attn_out / hook_mlp_out rows and the last-position logits."""
    L = o.cfg.n_layers
    x, z, res, attn, mlp, logits = [], [], [], [], [], []
    for ids, q in zip(seqs, qpos):
        lg, cache = o.run_with_cache(torch.tensor([ids]))
        x.append([cache[f"blocks.{l}.hook_resid_pre"][0, q] for l in range(L)] + [cache[f"blocks.{L - 1}.hook_resid_post"][0, q]])
        z.append([cache[f"blocks.{l}.attn.hook_z"][0, q].reshape(-1) for l in range(L)])
        res.append([cache[f"blocks.{l}.attn.hook_result"][0, q] for l in range(L)])
        attn.append([cache[f"blocks.{l}.hook_attn_out"][0, q] for l in range(L)])
        mlp.append([cache[f"blocks.{l}.hook_mlp_out"][0, q] for l in range(L)])
        logits.append(lg[0, q])
    st = lambda rows: np.stack([np.stack([t.numpy() for t in r]) for r in rows]).swapaxes(0, 1)  # noqa: E731
    return st(x), st(z), st(res), st(attn), st(mlp), np.stack([t.numpy() for t in logits])


@pytest.mark.parametrize("contrast", (False, True))
def test_reference_is_transformer_lens_decomposition(oracle64, tiny_cfg, contrast):
    o, cfg = oracle64, tiny_cfg
    L, H, dh, d = cfg.n_layers, cfg.n_heads, cfg.d_model // cfg.n_heads, cfg.d_model
    seqs = ragged_prompts(cfg, LENS)
    qpos = [len(s) - 1 for s in seqs[:-1]] + [1]
    tg = np.asarray([5, 77, 300])
    ct = np.asarray([9, 3, 411]) if contrast else None
    x, z, res, attn, mlp, logits = oracle_arrays(o, seqs, qpos)
    WU = o.w["W_U"].numpy()  # [d][V]
    ut, uc = WU[:, tg].T, (WU[:, ct].T if contrast else None)
    # the engine's layout of W_O: w2[c][h dh + k] = W_O[h][k][c]
    Ws = [o.w["blocks"][l]["W_O"].reshape(d, d).T.numpy() for l in range(L)]
    heads, resid = C.attribution(x, z, Ws, ut, uc, cfg.ln_eps, dh)
    u = ut - (0 if uc is None else uc)
    sigma = C.centre_scale(x[L], cfg.ln_eps, np.float64)
    dirs = u / sigma[:, None]
    scale = np.abs(resid).max()
    # heads from hook_result
    want = np.einsum("lnhc,nc->nlh", res, dirs)
    assert np.abs(heads - want).max() <= 1e-12 * scale
    # the rest of a layer: (hook_attn_out - sum of hook_result) + hook_mlp_out = b_O + MLP
    rest_want = np.einsum("lnc,nc->nl", (attn - res.sum(2)) + mlp, dirs)
    rest = resid[:, 1:] - resid[:, :-1] - heads.sum(-1)
    assert np.abs(rest - rest_want).max() <= 1e-12 * scale
    # conservation: embed + sum over layers of (heads + rest) = the logit difference minus b_U's
    bU = o.w["b_U"].numpy()
    diff = logits[np.arange(3), tg] - bU[tg]
    if contrast:
        diff = diff - (logits[np.arange(3), ct] - bU[ct])
    total = resid[:, 0] + (heads.sum(-1) + rest).sum(-1)
    assert np.abs(total - diff).max() <= 1e-12 * np.abs(diff).max()
    assert np.abs(resid[:, L] - diff).max() <= 1e-12 * np.abs(diff).max()
    # the trace bars of these arrays (as fp32 inputs) are finite and positive
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    bars = C.attribution_bar(f32(x), f32(z), [f32(w) for w in Ws], f32(ut), f32(uc), cfg.ln_eps, dh)
    assert all(np.isfinite(b) and 0 < b < 1e-3 * scale for b in bars), bars


@pytest.mark.parametrize("model", A.MODELS, ids=[f"dh{dh}h{h}" for dh, h in A.MODELS])
def test_bars_are_finite_and_positive_and_exact_cases_exact(model):
    dh, H = model
    for n in C.ALL_N:
        for kind in C.KINDS:
            case = C.make(kind, dh, H, n)
            ref = C.reference(case)
            b, e1, e2 = C.bar(case, ref)
            assert np.isfinite(b) and b > 0 and np.isfinite(ref).all(), (kind, n, b)
            assert b <= 1e-4 * max(np.abs(C.heads_terms(case.z, case.dirs, case.W, dh)).max(), 1e-30), (kind, n, b)
            if kind == "select":
                assert C.select_is_exact(case)
                assert np.array_equal(ref.astype(np.float32), case.exact) and np.count_nonzero(case.exact) <= n
            if kind == "zero":
                zr = C.zero_rows(case)
                assert (n < 2 or zr.any()) and (ref[zr] == 0).all() and (C.restate_plain(case)[zr] == 0).all() \
                    and (C.restate_result(case)[zr] == 0).all()
                assert (ref[~zr] != 0).all()
            if kind == "cancel":  # the heads' shares are large against their sum
                assert np.abs(ref.sum(-1)).max() <= 1e-4 * np.abs(ref).sum(-1).min()


def test_a_lost_term_or_a_wrong_head_misses_the_bar():
    """The bar separates: dropping one weight row of 1,024 products, or reading the next head's z, is far outside."""
    dh, H = 64, 4
    case = C.make("random", dh, H, 17)
    ref = C.reference(case)
    b = C.bar(case, ref)[0]
    W = case.W.copy()
    W[3] = 0.0
    assert C.max_err(C.heads_of(case.z, case.dirs, W, dh), ref) > 100 * b
    z = np.roll(case.z, dh, axis=1)
    assert C.max_err(C.heads_of(z, case.dirs, case.W, dh), ref) > 100 * b
