"""The attention reference, cases and bar of attention_cases.py, on the CPU.

* the fp64 reference restates the project's oracle: on a whole sequence it
  equals ``oracle/hooked_pythia.py`` ``_attn``'s ``hook_z`` of the tiny model;
* the layouts hold what test_gpu_attention.py relies on (every kernel form's
  longest T, p0 off and on a tile edge, followers, q0 > 0, single rows);
* every ``select`` case the GPU test runs is exact in fp32: the softmax is
  one-hot and P V equals the selected V row bit for bit, in the plain order and
  in the chunked online-softmax order;
* a subtly wrong attention (a mask off by one, a rotary sign, a key rotated at
  the next position, one clamped V row) misses the bar of the ``random`` cases
  by more than 100 x: the bar separates right from wrong.
"""
import numpy as np
import pytest
import torch

import attention_cases as A


def test_reference_restates_the_oracle(tiny_cfg, tiny_oracle64):
    o, cfg = tiny_oracle64, tiny_cfg
    T, d, H, DH = 23, cfg.d_model, cfg.n_heads, cfg.d_head
    torch.manual_seed(5)
    x = o._ln_pre(torch.randn(1, T, d, dtype=torch.float64))
    b = o.w["blocks"][0]
    q, k, v = (torch.einsum("bpd,hde->bphe", x, b["W_" + n]) + b["b_" + n] for n in "QKV")
    cache = {}
    o._hooks = {"blocks.0.attn.hook_z": [lambda t, hook: cache.setdefault("z", t.clone())]}
    try:
        o._attn(0, x)
    finally:
        o._hooks = {}
    lay = A.Layout().add(T)
    lay.row_from = 1
    qkv = np.full((lay.rows, 3 * d), np.nan)
    qkv[1:1 + T] = torch.cat([t.reshape(T, d) for t in (q, k, v)], dim=1).numpy()
    case = A.Case("oracle", DH, H, lay, qkv, np.zeros((1, 3 * d)))
    z = A.reference(case, o._cos[:, :DH // 4].numpy(), o._sin[:, :DH // 4].numpy())
    want = cache["z"].reshape(T, d).numpy()
    assert np.abs(z[1:1 + T] - want).max() <= 1e-14 * np.abs(want).max()
    assert np.isnan(z[0]).all() and np.isnan(z[1 + T]).all()


def test_tables_are_the_fp32_tables_of_the_oracle(tiny_cfg, tiny_oracle):
    cos, sin = A.tables(tiny_cfg.d_head, tiny_cfg.n_ctx, tiny_cfg.rotary_base)
    assert cos.dtype == np.float32 and cos.shape == (tiny_cfg.n_ctx, tiny_cfg.d_head // 4)
    assert np.array_equal(cos, tiny_oracle._cos.numpy()) and np.array_equal(sin, tiny_oracle._sin.numpy())


def test_layouts_reach_the_edges():
    for nkt, ts in A.MAXT.items():
        for maxT in ts:
            assert A.nkt_of(maxT) == nkt
            for lay in (A.batch(maxT), A.batch_rows(maxT)):
                assert 3 <= lay.n_seq <= 5 and lay.maxT == maxT
                assert any(s.p0 + s.n == 1 for s in lay.seqs)
                rows = [r for s in lay.seqs for r in range(s.row0, s.row0 + s.n)]
                assert len(set(rows)) == len(rows) and 0 not in rows and max(rows) == lay.rows - 2
                for s in lay.seqs[lay.row_from:]:
                    assert s.q0 == s.n - 1
            lay = A.batch(maxT)
            if maxT >= 15:
                assert {s.prefix_live for s in lay.seqs if s.p0} == {0, 1}
                assert any(s.p0 % 16 for s in lay.seqs) and any(0 < s.q0 < s.n - 1 for s in lay.seqs)
                assert any(s.p0 and s.q0 == s.n - 1 for s in lay.seqs)
            if maxT >= 32:
                assert {0, 5, 16, 23} == {s.p0 for s in lay.seqs}
                assert any((s.p0 + s.n) % 16 == 0 for s in lay.seqs)
    # padding appends: the other sequences keep their rows and values
    a, b = A.batch(15), A.batch(15, pad=100)
    assert b.seqs[:-1] == a.seqs and A.nkt_of(b.maxT) == 8
    ca, cb = A.make("random", 16, 4, a, seed=3), A.make("random", 16, 4, b, seed=3)
    assert np.array_equal(ca.qkv[:a.rows - 1], cb.qkv[:a.rows - 1], equal_nan=True)
    assert np.array_equal(ca.cache, cb.cache, equal_nan=True)


def test_select_dims_sit_in_every_lane_group():
    for DH, _ in A.MODELS:
        a = A.select_dims(DH)
        for g, x in enumerate(a, start=1):
            assert g * DH // 4 <= x and x + 1 < (g + 1) * DH // 4
        assert a[-1] + 1 == DH - 1
    # over the rotations every head meets every dim pair, and a launch of 5 x 4 heads holds every family
    for H in (2, 3, 4, 6):
        for h in range(H):
            assert {A.select_plan(16, H, 0, h, r)[1] for r in A.SELECT_ROTS} == set(A.select_dims(16))
    fams = {A.select_plan(64, 4, s, h, r)[0] for s in range(5) for h in range(4) for r in A.SELECT_ROTS}
    assert fams == set(range(len(A.SELECT_FAMILIES)))


@pytest.mark.parametrize("model", A.MODELS, ids=lambda m: f"dh{m[0]}h{m[1]}")
def test_select_cases_are_exact_in_fp32(model):
    """Every select case of test_gpu_attention.py (its SELECT_LAUNCHES)."""
    DH, H = model
    cos, sin = A.tables(DH)
    for maxT, rows, rot in A.select_launches():
        lay = A.batch_rows(maxT) if rows else A.batch(maxT)
        case = A.make("select", DH, H, lay, seed=maxT, rot=rot)
        q = A.query_rows(lay)
        assert not np.isnan(case.expect[q]).any() and (case.expect[q] != 0).all()
        assert A.select_is_exact(case, cos, sin), (model, maxT, rows, rot)


def test_select_future_key_is_masked():
    lay = A.Layout().add(40)
    lay.row_from = 1
    for rot in A.SELECT_ROTS:
        case = A.make("select", 16, 4, lay, rot=rot)
        for h in range(4):
            fam, _ = A.select_plan(16, 4, 0, h, rot)
            if A.SELECT_FAMILIES[fam][0] == "future":  # pi = i + 5 > i: the answer is V of the query's own row
                assert np.array_equal(case.expect[1:41, 16 * h:16 * h + 16], case.qkv[1:41, 128 + 16 * h:144 + 16 * h])
                return
    raise AssertionError("no head took the future family")


@pytest.mark.parametrize("model", A.MODELS, ids=lambda m: f"dh{m[0]}h{m[1]}")
def test_wrong_attention_misses_the_bar(model):
    DH, H = model
    cos, sin = A.tables(DH)
    for maxT in (15, 33, 129):
        case = A.make("random", DH, H, A.batch(maxT), seed=maxT)
        z64 = A.reference(case, cos, sin)
        bar, e1, e2 = A.bar(case, cos, sin, z64)
        # fp32 attention on unit-normal inputs: 5e-8 .. 2e-6 of max |V|, the two orders within about 3 x
        assert 2e-8 < max(e1, e2) / case.max_v() < 3e-6 and max(e1, e2) <= 4 * min(e1, e2)
        for mut in A.MUTATIONS:
            err = A.max_err(A.reference(case, cos, sin, mutate=mut), z64, case.lay)
            assert err > 100 * bar, (mut, maxT, err, bar)


def test_forced_inputs_are_what_they_claim():
    DH, H = 16, 4
    cos, sin = A.tables(DH)
    lay = A.batch(300)
    # uniform: z[i] = mean of V[0 .. i]
    case = A.make("uniform", DH, H, lay)
    z = A.reference(case, cos, sin)
    sd = lay.seqs[0]
    v = case.own(0)[:, 2 * case.d:].astype(np.float64)
    want = np.cumsum(v, axis=0) / np.arange(1, sd.n + 1)[:, None]
    assert np.abs(z[sd.row0:sd.row0 + sd.n] - want).max() < 1e-13
    # huge: scores of -+3e4 before scaling, finite z, inside the bar's reach in fp32
    case = A.make("huge", DH, H, lay)
    q, k = case.own(0)[:, :case.d], case.own(0)[:, case.d:2 * case.d]
    sc = q[:, :DH].astype(np.float64) @ k[:, :DH].astype(np.float64).T
    assert set(np.unique(np.abs(sc))) == {3e4, 3.02e4, 3.04e4} and sc[0, 0] < 0 < sc[0, 8]
    z64 = A.reference(case, cos, sin)
    bar, e1, e2 = A.bar(case, cos, sin, z64)
    assert np.isfinite(z64[A.query_rows(lay)]).all() and np.isfinite(bar) and bar < 1e-5
    # rotary_only: nothing outside the rotary dims of Q and K
    case = A.make("rotary_only", DH, H, lay)
    x = case.own(0).reshape(-1, 3, H, DH)
    assert (x[:, :2, :, DH // 4:] == 0).all() and (x[:, :2, :, :DH // 4] != 0).all()
    # range: one V row at 5000 reaches a z row unmixed (T = 1 sees only it); 4000 stays below 4095
    for kind, top in (("range", 5000.0), ("range_below", 4000.0)):
        case = A.make(kind, DH, H, lay)
        z = A.reference(case, cos, sin)
        assert np.nanmax(np.abs(z)) == top
