"""CPU: the site-entry and head-set cases of tests/entry_cases.py judge themselves: both fp32 restatements of
the head replacement pass their own bar with room to spare, the exact kinds are exact, the floor sets the bar
in a bounded share of the graded cases, and every mutation of the reference misses the bar or the exact
comparison."""
import numpy as np
import pytest

import attention_cases as A
import entry_cases as E

LENS = (1, 15, 16, 17, 33)


def sites_of(case):
    """One REPLACE_HEAD site per sequence: heads first / middle / last in turn, layers in turn."""
    H = case.n_heads
    heads = (0, H // 2, H - 1)
    return [E.Site(s, E.REPLACE_HEAD, layer=s % case.L, head=heads[s % 3], vec=heads[s % 3] if case.kind == "cancel" else s % 3)
            for s in range(len(case.seq_lens))]


def make(kind, model, seed=0):
    return E.make(kind, *model, LENS, nv=model[1] if kind == "cancel" else 3, seed=seed)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_constants_are_the_projects():
    import attribution_cases as C
    assert E.BAR_MARGIN is A.BAR_MARGIN and E.FLOOR_ULPS is C.FLOOR_ULPS and E.EPS24 is C.EPS24


def test_restatements_pass_their_own_bar_and_the_floor_share():
    graded = floored = 0
    for model in A.MODELS:
        for kind in E.GRADED:
            for seed in (0, 1, 2):
                case = make(kind, model, seed)
                sites = sites_of(case)
                bar, e, floor = E.bar(case, sites)
                assert 0 < bar and e <= bar / E.BAR_MARGIN + 1e-300, (model, kind, e, bar)
                graded += 1
                floored += bar == floor
                if kind == "cancel":  # the regime: at position 0, v - dot is a few ulps of a value 2^6 and more times larger
                    s = next(x for x in sites if x.layer == 0)
                    snap, zz, w, v = E._operands(case, s)
                    dot = zz[0].astype(np.float64) @ w.astype(np.float64).T
                    assert np.abs(v - dot).max() <= 8 * 2.0 ** -24 * np.abs(dot).max() and np.abs(dot).max() > 16
    print(f"the floor sets the bar in {floored} of {graded} graded cases")
    assert (floored, graded) == (11, 72) and floored <= graded // 4  # (the share the module's docstring records)


def test_exact_kinds_are_exact_in_both_restatements():
    for model in A.MODELS:
        for kind in ("select", "integer", "zero"):
            case = make(kind, model)
            for s in sites_of(case):
                want = E.replace_head_exact(case, s)
                a, b = E.replace_head_rows(case, s, "a"), E.replace_head_rows(case, s, "b")
                rows = E.zero_positions(case.seq_lens[s.seq]) if kind == "zero" else slice(None)
                assert (bits(a[rows]) == bits(want[rows])).all(), (model, kind)
                if kind == "select":  # b's dot is the selected column too; its two last roundings associate otherwise
                    da, db = E.replace_head_dots(case, s)
                    assert (bits(da) == bits(db)).all()
                    assert (bits(s_v_w(case, s, da)) == bits(want)).all()
                else:
                    assert (bits(b[rows]) == bits(want[rows])).all(), (model, kind)
                # and the fp64 reference rounds to the same rows where one rounding suffices
                if kind == "integer":
                    assert (E.replace_head_rows(case, s) == want).all()


def s_v_w(case, site, dot):
    snap, _, _, v = E._operands(case, site)
    return snap + (v[None, :] - dot)


@pytest.mark.parametrize("mutate", E.MUTATIONS)
def test_every_mutation_of_the_head_replacement_is_caught(mutate):
    for model in A.MODELS:
        for kind in E.KINDS:
            case = make(kind, model)
            sites = sites_of(case)
            bar = E.bar(case, sites)[0]
            caught = False
            for s in sites:
                T = case.seq_lens[s.seq]
                if mutate == "clamp" and T == 1:
                    continue  # (one position: nothing to clamp to)
                bad = E.replace_head_rows(case, s, mutate=mutate)
                if kind in ("select", "integer"):
                    hit = (bad.astype(np.float32) != E.replace_head_exact(case, s)).any()
                else:
                    hit = E.max_err(bad, E.replace_head_rows(case, s)) > bar
                if kind == "zero" and mutate in ("wrong_head", "drop_k_chunk", "v_plus_acc") and T <= 1:
                    continue
                caught = caught or hit
                if kind in ("random", "gain") and T > 1:
                    assert hit, (mutate, model, kind, T)  # every site of the ordinary kinds sees it
            if not (kind == "cancel" and mutate == "clamp"):  # (cancel's z rows are the same to 2^-17: a neighbour's row passes)
                assert caught, (mutate, model, kind)


def test_copy_kinds_and_entry_layers():
    case = make("random", (16, 4))
    L = case.L
    T2 = case.seq_lens[2]
    p0, rows = E.site_rows(case, E.Site(2, E.SET_POS, layer=1, pos=3, src_seq=4, src_pos=20))
    assert p0 == 3 and rows.shape == (T2 - 3, case.d)
    assert (rows[0] == case.resid[1, case.off[4] + 20]).all() and (rows[1:] == case.resid[1, case.off[2] + 4:case.off[2] + T2]).all()
    p0, rows = E.site_rows(case, E.Site(2, E.SET_VEC, layer=0, pos=T2 - 1, vec=1))
    assert p0 == T2 - 1 and (rows == case.vectors[1][None]).all()
    p0, rows = E.site_rows(case, E.Site(1, E.ADD_LAST, layer=L - 1, vec=2))
    assert p0 == 14 and (bits(rows[0]) == bits(case.resid[L, case.off[1] + 14] + case.vectors[2])).all()
    p0, rows = E.site_rows(case, E.Site(3, E.NONE))
    assert p0 == 16 and (rows[0] == case.resid[L, case.off[3] + 16]).all()
    assert E.site_rows(case, E.Site(3, E.SET_ALLPOS), ((1, 0, 0), (0, 2, 1)))[1].shape == (17, case.d)
    assert E.entry_layer(case, E.Site(3, E.SET_LASTPOS), ((1, 0, 0),)) == 1
    assert E.site_rows(case, E.Site(3, E.SET_ALLPOS))[0] == 16  # an empty set is NONE


def hs_inputs(fmt, model, rows=11, seed=0):
    DH, H = model
    d, K2 = DH * H, DH * H + E.D_MLP
    rng = np.random.default_rng([seed, DH, H])
    a2 = rng.integers(1, 256, size=(rows, 4 * K2), dtype=np.uint8)  # no zero byte: a zeroed one shows
    resid = rng.standard_normal((rows, d)).astype(np.float32)
    vectors = rng.standard_normal((4, d)).astype(np.float32)
    return a2, resid, vectors, d, K2


@pytest.mark.parametrize("fmt", E.HS_FORMATS)
def test_headset_expectation(fmt):
    for model in A.MODELS:
        DH, H = model
        a2, resid, vectors, d, K2 = hs_inputs(fmt, model)
        items = [(1, 3, 0, 2), (6, 4, 2, 1), (4, 1, 3, 0)]
        patches = [(H - 1, 2), (0, 1), (H // 2, 1)]
        got_a2, got_r = E.headset_expect(fmt, DH, K2, a2, resid, vectors, items, patches)
        planes = 2 if fmt.startswith("x2") else 1
        width = 4 if fmt == "f32" else 2
        zeroed = (got_a2 == 0)
        assert zeroed[1:4].sum() == 3 * 2 * planes * width * DH and zeroed[6:10].sum() == 4 * planes * width * DH
        assert (got_a2[[0, 4, 5, 10]] == a2[[0, 4, 5, 10]]).all() and (got_a2[~zeroed] == a2[~zeroed]).all()
        assert (bits(got_r[1:4]) == bits(resid[1:4] + ((0 + vectors[2]) + vectors[1]))).all()
        assert (bits(got_r[[0, 4, 5, 10]]) == bits(resid[[0, 4, 5, 10]])).all()  # (an empty range: x + 0)
        if fmt == "x2f16i":  # the interleaved rows are the planar rows permuted (tests/test_gpu_act_layout.py)
            pl = a2.view(np.uint16).reshape(-1, K2 // 32, 2, 32).transpose(0, 2, 1, 3).reshape(-1, 2 * K2)
            want, _ = E.headset_expect("x2f16", DH, K2, np.ascontiguousarray(pl).view(np.uint8), resid, vectors, items, patches)
            assert (got_a2.view(np.uint16).reshape(-1, K2 // 32, 2, 32).transpose(0, 2, 1, 3).reshape(-1, 2 * K2) ==
                    want.view(np.uint16)).all()
        for mutate in E.HS_MUTATIONS:  # one 16-byte word too long: a neighbour's or the MLP columns' bytes
            bad, _ = E.headset_expect(fmt, DH, K2, a2, resid, vectors, items, patches, mutate=mutate)
            # (head 0's extra word lies in head 1, which item 0 patches itself when there are two heads)
            assert (bad != got_a2).sum() == 16 * planes * (3 * (2 if H > 2 else 1) + 4), (fmt, model)
