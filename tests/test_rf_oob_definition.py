"""CPU-only: tests/_rfoobdef.py (the NumPy second author of train_forest's out-of-bag outputs) against cases worked out by
hand and against the properties the definition promises.  The device trainer is held to _rfoobdef in tests/test_gpu_forest_oob.py."""
import math

import numpy as np
import pytest

import _rfdef
import _rfoobdef as R

SEED = _rfdef.DEFAULT_SEED


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_six_rows_one_column_three_trees_by_hand():
    """Rows x = 0..5 of classes 0 0 1 0 1 1 (labels -1 -1 1 -1 1 1), sample_ratio 0 (six draws), weights 1 and 1.

    tree 0: bag 0 x1, 3 x2, 5 x3 (classes 0 0 1): one cut between 3 and 5 at 4.0, left class 0, right class 1.
            out of bag 1, 2, 4 -> all go left: classes 0 0 0.  Their own classes are 0 1 1: n = (1, 2), r = (1, 0).
            pi = (2, 1, 0): rank 0 gets x = 4, rank 2 gets x = 1, all still go left: d = (0, 0).
            votes so far: rows 1, 2, 4 one vote for class 0.  seen 3 (1 of class 0, 2 of class 1), wrong: rows 2 and 4.
    tree 1: bag 0 x2, 1 x3, 5 x1: one cut between 1 and 5 at 3.0.  out of bag 2, 3, 4 -> classes 0 0 1; own 1 0 1: n = (1, 2), r = (1, 1).
            pi = (0, 2, 1): row 3 gets x = 4 and turns to class 1 (d_0 = 1), row 4 gets x = 3 and turns to class 0 (d_1 = 1).
            votes: row 1 (1, 0), row 2 (2, 0), row 3 (1, 0), row 4 (1, 1) -- a tie, so class 0.  seen 4, wrong: rows 2 and 4.
    tree 2: bag 0, 2, 3 x2, 4, 5: cuts at 3.5, then 2.5, then 1.0; out of bag only row 1 -> left, left, left: class 0.  m = 1, pi = (0): d = 0.
    Gini: tree 0 root (3, 3) -> (3, 0) + (0, 3): 3 + 3 - 3 = 3.  tree 1 root (5, 1) -> 5 + 1 - 26/6.  tree 2: root (3, 3) -> (3, 1) + (0, 2):
          2.5 + 2 - 3; node 1 (3, 1) -> (1, 1) + (2, 0): 1 + 2 - 2.5; node 3 (1, 1) -> 1 + 1 - 1."""
    X = np.arange(6.0).reshape(6, 1)
    y = np.array([-1, -1, 1, -1, 1, 1], np.int32)
    opts = dict(ntree=3, sample_ratio=0.0)
    assert [_rfdef.bootstrap(SEED, t, 6, 6).tolist() for t in range(3)] == [[1, 0, 0, 2, 0, 3], [2, 3, 0, 0, 0, 1], [1, 0, 1, 2, 1, 1]]
    model = _rfdef.train(X, y, **opts)
    assert model["ndbigtree"].tolist() == [3, 3, 7]
    assert model["xbestsplit"][:, 0].tolist() == [4.0, 3.0, 3.5] and model["xbestsplit"][2, :4].tolist() == [3.5, 2.5, 0.0, 1.0]
    assert model["nodeclass"][2].tolist() == [0, 0, 2, 0, 1, 1, 2]
    assert [R.perm_all(SEED, t, 0, m).tolist() for t, m in ((0, 3), (1, 3), (2, 1))] == [[2, 1, 0], [0, 2, 1], [0]]
    details = {}
    got = R.oob(X, y, model, details=details, **opts)
    trees = details["trees"]
    assert [t["oob"].tolist() for t in trees] == [[1, 2, 4], [2, 3, 4], [1]]
    assert [t["p"].tolist() for t in trees] == [[0, 0, 0], [0, 0, 1], [0]]
    assert [t["n_k"] for t in trees] == [[1, 2], [1, 2], [1, 0]] and [t["r_k"] for t in trees] == [[1, 0], [1, 1], [1, 0]]
    assert [t["d"].tolist() for t in trees] == [[[0, 0]], [[1, 1]], [[0, 0]]]
    assert got["counttr"].tolist() == [[0, 2, 2, 1, 1, 0], [0, 0, 0, 0, 1, 0]]
    assert got["votes"].tolist() == [[0, 0], [2, 0], [2, 0], [1, 0], [1, 1], [0, 0]]
    assert got["oob_times"].tolist() == [0, 2, 2, 1, 2, 0] and got["outcl"].tolist() == [0, 1, 1, 1, 1, 0]
    assert got["err_wrong"].tolist() == [[2, 0, 2]] * 3 and got["err_seen"].tolist() == [[3, 1, 2], [4, 2, 2], [4, 2, 2]]
    assert got["errtr"].tolist() == [[2.0 / 3.0, 0.0, 1.0], [0.5, 0.0, 1.0], [0.5, 0.0, 1.0]]
    g = ((3.0 + (6.0 - 26.0 / 6.0)) + 1.5 + 0.5 + 1.0) / 3.0
    assert got["importance"].tolist() == [[1.0 / 3.0, 0.5 / 3.0, (2.0 / 3.0) / 3.0, g]]
    sd = [math.sqrt((s2 / 3.0 - (s / 3.0) * (s / 3.0)) / 3.0) for s, s2 in ((1.0, 1.0), (0.5, 0.25), (2.0 / 3.0, (2.0 / 3.0) * (2.0 / 3.0)))]
    assert got["importanceSD"].tolist() == [sd]


def test_feistel_rounds_by_hand():
    """m = 3: b = 2, one bit per half.  One pass from x = (L, R) is four times (L, R) <- (R, L ^ (mix(K_r ^ R) & 1))."""
    assert [R.perm_bits(m) for m in (1, 2, 4, 5, 16, 17, 64, 65, 256, 257)] == [2, 2, 2, 4, 4, 6, 6, 8, 8, 10]
    K = [_rfdef.h(SEED, 5, R.A_PERM + 2, r) for r in range(4)]
    for j in range(3):
        x, passes = j, 0
        while True:
            L, Rr = x >> 1, x & 1
            for r in range(4):
                L, Rr = Rr, L ^ (_rfdef.mix(K[r] ^ Rr) & 1)
            x = (L << 1) | Rr
            passes += 1
            if x < 3:
                break
        seen = []
        assert R.perm(SEED, 5, 2, j, 3, seen) == x and seen == [passes]
    # the argument 2^32 + v collides with neither the bootstrap (0) nor the tried variables (1 + node < 2^29)
    assert R.A_PERM > (1 << 29)


@pytest.mark.parametrize("m", list(range(1, 301)) + [4 ** k + d for k in range(1, 8) for d in (-1, 0, 1)])
def test_the_permutation_is_a_bijection(m):
    for t, v in ((0, 0), (3, 7), (254, 103)):
        pi = R.perm_all(SEED, t, v, m)
        assert np.array_equal(np.sort(pi), np.arange(m))
        if m <= 64:                                                         # the scalar and the vectorised form are one function
            assert [R.perm(SEED, t, v, j, m) for j in range(m)] == pi.tolist()


@pytest.fixture(scope="module")
def forty():
    """40 rows x 3 columns, 5 trees; column 1 is constant, so no node can test it"""
    rng = np.random.default_rng(20261021)
    X = rng.normal(size=(40, 3))
    X[:, 1] = 2.5
    y = np.where(X[:, 0] + 0.4 * rng.normal(size=40) > 0, 1, -1).astype(np.int32)
    opts = dict(ntree=5, mtry=2)
    details = {}
    return X, y, opts, R.oob(X, y, details=details, **opts), details


def test_tallies_hang_together(forty):
    X, y, opts, got, details = forty
    assert (got["votes"] == got["counttr"].T).all() and (got["oob_times"] == got["counttr"].sum(axis=0)).all()
    assert (np.diff(got["err_seen"], axis=0) >= 0).all()                      # a row once seen stays seen
    assert (got["err_seen"][:, 0] == got["err_seen"][:, 1:].sum(axis=1)).all() and (got["err_wrong"][:, 0] == got["err_wrong"][:, 1:].sum(axis=1)).all()
    assert got["err_seen"][-1, 0] == (got["oob_times"] > 0).sum()
    cls = _rfdef.derive(y, 3)["cls"]
    seen = got["oob_times"] > 0
    assert got["err_wrong"][-1, 0] == (seen & (got["outcl"] - 1 != cls)).sum() and (got["outcl"][~seen] == 0).all()
    assert got["oob_times"].sum() == sum(t["m"] for t in details["trees"])
    assert got["importance"].shape == (3, 4) and got["importanceSD"].shape == (3, 3) and got["errtr"].shape == (5, 3)


def test_a_column_no_tree_tests_has_importance_zero(forty):
    X, y, opts, got, details = forty
    assert not (details["model"]["bestvar"] == 2).any() and (details["model"]["bestvar"] == 1).any()
    assert (_bits(got["importance"][1]) == 0).all() and (_bits(got["importanceSD"][1]) == 0).all()        # +0.0 exactly
    assert got["importance"][0, 2] > 0 and got["importance"][0, 3] > 0


def test_walking_every_column_equals_skipping_untested_ones(forty):
    """the definition's shortcut (a column no node of the tree tests: d = 0) against the walks it leaves out"""
    X, y, opts, got, details = forty
    model, cls = details["model"], _rfdef.derive(y, 3)["cls"]
    for t, tree in enumerate(details["trees"]):
        O = tree["oob"]
        for v in range(3):
            rows = X[O].copy()
            rows[:, v] = X[O[R.perm_all(SEED, t, v, len(O))], v]
            p2, _ = R.classes(model, t, rows)
            assert [tree["r_k"][k] - int(((cls[O] == k) & (p2 == k)).sum()) for k in range(2)] == tree["d"][v].tolist()


def test_without_importance_only_the_tallies(forty):
    X, y, opts, got, _ = forty
    only = R.oob(X, y, importance=False, **opts)
    assert sorted(only) == sorted(R.INT_KEYS + ("errtr",)) and R.differences(only, {k: got[k] for k in only}) == []
