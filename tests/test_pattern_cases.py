"""CPU: the attention-pattern cases of tests/pattern_cases.py are what they claim
to be — the select cases exactly one-hot in both fp32 restatements, the bar
tight enough that a wrong mask, rotary sign or key position exceeds it, the
inputs poisoned where no read is due, the class helper an fp64 sum."""
import numpy as np
import pytest

import attention_cases as A
import pattern_cases as P

MODEL_IDS = [f"dh{dh}h{h}" for dh, h in A.MODELS]


@pytest.fixture(scope="module", params=A.MODELS, ids=MODEL_IDS)
def model(request):
    return request.param


def test_layout_and_poison(model):
    for T in P.ALL_T:
        case = P.make("random", *model, T)
        d = case.d
        assert case.qpos.tolist() == [T - 1, T // 2, 0] and case.maxT == T
        owned = np.zeros(case.lay.rows, dtype=bool)
        for s, sd in enumerate(case.seqs):
            assert sd.p0 == 0 and case.row0[s] == sd.row0
            owned[sd.row0:sd.row0 + sd.n] = True
            q_nan = np.isnan(case.qkv[sd.row0:sd.row0 + sd.n, :d]).all(axis=1)
            assert q_nan.sum() == sd.n - 1 and not q_nan[sd.q0], "only the query row keeps its Q"
            assert not np.isnan(case.qkv[sd.row0:sd.row0 + sd.n, d:]).any(), "later K rows exist"
        assert np.isnan(case.qkv[~owned]).all(), "the rows between the sequences are NaN"


def test_select_restatements_are_exactly_one_hot(model):
    cos, sin = A.tables(model[0])
    for T in P.ALL_T:
        for rot in A.SELECT_ROTS:
            case = P.make("select", *model, T, rot=rot)
            assert (case.hot <= case.qpos[:, None]).all() and (case.hot >= 0).all()
            assert P.select_is_exact(case, cos, sin), (model, T, rot)
            p64 = P.reference(case, cos, sin)
            # (in fp64 the next-best key keeps exp(-2048 / sqrt(d_head)) > 0: below any fp32 number)
            assert np.abs(p64 - P.one_hot(case)).max() < 1e-70
    # the hot key is not always the query or key 0: the cases would pass a kernel that ignores the scores
    hots = {int(h) for T in P.ALL_T for h in P.make("select", *model, T).hot[0]}
    assert len(hots) > 3


def test_reference_rows_sum_to_one_and_are_zero_beyond_the_query(model):
    cos, sin = A.tables(model[0])
    for kind in P.KINDS:
        case = P.make(kind, *model, 65)
        p64 = P.reference(case, cos, sin)
        assert p64.dtype == np.float64 and p64.shape == (3, model[1], 65)
        np.testing.assert_allclose(p64.sum(-1), 1.0, rtol=0, atol=1e-13)
        for s, q in enumerate(case.qpos):
            assert (p64[s, :, q + 1:] == 0).all() and (p64[s, :, :q + 1] >= 0).all()
        b, e1, e2 = P.bar(case, cos, sin, p64)
        assert b == max(4 * max(e1, e2), 2.0 ** -22) and b < 1e-5
        if kind == "uniform":
            for s, q in enumerate(case.qpos):
                assert np.array_equal(p64[s, :, :q + 1], np.full((model[1], q + 1), 1.0 / (q + 1)))
        if kind == "huge":  # the keys of a block of 8 are exactly tied
            assert np.array_equal(p64[0, :, 56], p64[0, :, 63])


@pytest.mark.parametrize("mutation", P.MUTATIONS)
def test_mutations_exceed_the_bar(model, mutation):
    cos, sin = A.tables(model[0])
    caught = 0
    for kind in ("random", "rotary_only"):
        for T in (17, 65, 300):
            case = P.make(kind, *model, T)
            p64 = P.reference(case, cos, sin)
            err = P.max_err(P.reference(case, cos, sin, mutate=mutation), p64)
            caught += err > P.bar(case, cos, sin, p64)[0]
    assert caught >= 1, (model, mutation)


def test_class_helper_sums_in_fp64(model):
    cos, sin = A.tables(model[0])
    case = P.make("random", *model, 129)
    cls = P.classes(case)
    assert cls.min() == -1 and cls.max() == P.N_CLASSES - 1 and cls.shape == (case.lay.rows,)
    p32 = P.restate_plain(case, cos, sin)
    mass = P.class_sums(p32, case, cls)
    assert mass.dtype == np.float64 and mass.shape == (3, model[1], P.N_CLASSES)
    s1 = case.seqs[1]
    assert (cls[s1.row0:s1.row0 + s1.n] != 2).all() and (mass[1, :, 2] == 0).all(), "class 2 is empty in sequence 1"
    assert (mass[2, :, 0] == 0).all() and (mass[2, :, 2] == 0).all() and (mass[2, :, 1] == p32[2, :, 0]).all()
    # with the keys of class -1 the classes partition the seen keys: an exact fp64 identity up to its rounding
    for s, sd in enumerate(case.seqs):
        c = cls[sd.row0:sd.row0 + sd.q0 + 1]
        rest = p32[s, :, :sd.q0 + 1].astype(np.float64)[:, c == -1].sum(-1)
        np.testing.assert_allclose(mass[s].sum(-1) + rest, p32[s].astype(np.float64).sum(-1), rtol=0, atol=1e-15)
    # a key beyond the query position is never counted, whatever its class
    far = cls.copy()
    far[s1.row0 + s1.q0 + 1:s1.row0 + s1.n] = 2
    assert np.array_equal(P.class_sums(p32, case, far), mass)
