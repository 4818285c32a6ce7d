"""
tests/argmax_reference.py pinned without a GPU: the rule against numpy.argmax and against brute force on arrays with planted ties,
NaNs and exclusion balls; and the plateau construction of tests/test_gpu_argmax_contract.py -- for every model and acquisition that
file uses, through the oracle's posterior and EI / PI / UCB, a far row has the closed-form plateau value and every unit-cube row
stays below 0.9 of it.  The margin is a condition on the inputs: a model that misses it gets another seed, not another factor.
"""
import numpy as np
import pytest

import argmax_reference as ar


def brute(values, cand, exclude, radius, index_base):
    """the contract, one row at a time, nothing vectorised"""
    best = None
    for i, v in enumerate(values):
        if v != v:
            continue
        inside = False
        for e in ([] if exclude is None else exclude):
            d = float(np.sqrt(sum((float(c) - float(x)) ** 2 for c, x in zip(cand[i], e))))
            if not d > radius:
                inside = True
        if inside:
            continue
        if best is None or v > best[0]:
            best = (float(v), i)
    return (-np.inf, -1) if best is None else (best[0], index_base + best[1])


def test_rule_is_numpy_argmax_on_clean_arrays():
    rs = np.random.RandomState(0)
    for M in (1, 2, 63, 64, 65, 1000):
        v = rs.randint(0, 5, size=M).astype(float)               # many ties
        for base in (0, 1000, (1 << 33) + 5):
            assert ar.argmax_rule(v, index_base=base) == (v.max(), base + int(np.argmax(v)))
    assert ar.argmax_rule(np.array([-np.inf, -np.inf])) == (-np.inf, 0)        # -inf is a value: the first one wins


def test_rule_against_brute_force_with_ties_nans_and_balls():
    rs = np.random.RandomState(1)
    for trial in range(200):
        M, D = int(rs.randint(1, 80)), int(rs.randint(1, 5))
        cand = rs.randint(0, 8, size=(M, D)) * 0.25
        v = rs.randint(0, 4, size=M).astype(float)
        v[rs.rand(M) < .2] = np.nan
        if trial % 5 == 0:
            cand[rs.randint(M)] = np.nan                         # a NaN coordinate: its distance is NaN, the row excluded
        n = int(rs.randint(0, 3))
        excl = rs.randint(0, 8, size=(n, D)) * 0.25 if n else None
        radius = float(rs.choice([0.0, 0.25, 0.5, np.nextafter(0.25, 0)]))
        base = int(rs.choice([0, 1000, (1 << 33) + 5]))
        assert ar.argmax_rule(v, cand, excl, radius, base) == brute(v, cand, excl, radius, base), trial


def test_rule_edges():
    assert ar.argmax_rule(np.full(7, np.nan), index_base=1000) == (-np.inf, -1)            # -1 is not shifted
    c = np.array([[0.25, 0.], [5., 5.]])
    assert ar.argmax_rule([2., 1.], c, [[0., 0.]], 0.25, 10) == (1., 11)                   # the boundary is closed
    assert ar.argmax_rule([2., 1.], c, [[0., 0.]], np.nextafter(0.25, 0), 10) == (2., 10)
    assert ar.argmax_rule([2., 1.], c, [[0., 0.]], 100., 10) == (-np.inf, -1)
    assert ar.argmax_rule([1., 3., 3., np.nan, 3.]) == (3., 1)


def test_planted_inputs():
    for D in (3, 4):
        f = ar.far_rows(40, D)
        assert len(np.unique(f, axis=0)) == 40 and np.all(f >= 1000) and np.all(f <= 2000) and np.all(f * 4 == np.round(f * 4))
        d = np.abs(f[:, None, 0] - f[None, :, 0]) + np.eye(40)
        assert d.min() >= 1.0
    c = ar.plant(70000, 3, [5, 0, 69999])
    assert np.array_equal(c[[5, 0, 69999]], ar.far_rows(3, 3)) and np.all(np.delete(c, [0, 5, 69999], axis=0) < 1.0)
    assert np.array_equal(c[1], c[1 + ar.LOSER_BASE])


@pytest.mark.parametrize("name", sorted(ar.MODELS))
def test_plateau_margin(oracle, name):
    """every loser of every GPU test below MARGIN x plateau, and the plateau is what the oracle gives a far row"""
    seed, N, D, kind, hyper = ar.MODELS[name]
    X, Y = ar.model_data(name)
    assert -3.5 < Y.max() < -2.9
    ogp = oracle.GP(oracle.Kern(kind, hyper), X, Y, noise=ar.NOISE)
    invR = ogp.inv_factor()
    lose = ar.losers(ar.LOSER_BASE, D)
    far = ar.far_rows(8, D)
    code = {"ei": oracle.ACQ_EI, "pi": oracle.ACQ_PI, "ucb": oracle.ACQ_UCB}
    for acq, parm in ar.ACQS.values():
        plateau = ar.plateau_value(acq, parm, Y.max())
        o = oracle.sweep_native(ogp, far, code[acq], parm, invR=invR)
        assert np.all(o["mu"] == 0.0) and np.all(o["s2"] == 1.0 + ar.NOISE)
        np.testing.assert_allclose(o["acq"], plateau, rtol=1e-12, atol=0)
        worst = oracle.sweep_native(ogp, lose, code[acq], parm, invR=invR)["acq"].max()
        print("%s %s: plateau %.4f, best loser %.4f (ratio %.3f)" % (name, acq, plateau, worst, worst / plateau))
        assert plateau > 0 and worst < ar.MARGIN * plateau, (name, acq, worst, plateau)


def test_knowledge_gradient_inputs():
    A, strong, weak, best, rest = ar.kg_inputs()
    print("KG: strong row %.4g, best weak row %.4g of %d" % (best, rest, len(weak)))
    assert len(A) == ar.KG_NREF and len(weak) > 1000 and best > 1e-3 and rest < 0.5 * best < ar.MARGIN * best
    assert not np.any(np.all(weak == strong, axis=1))
    c = ar.plant_kg(3000, [2999, 0], strong, weak)
    assert np.array_equal(c[0], strong) and np.array_equal(c[2999], strong) and np.array_equal(c[1], weak[1])
