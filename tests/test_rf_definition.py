"""CPU-only: tests/_rfdef.py -- the NumPy restatement of the forest growing rule that the device trainer is held to --
against trees worked out by hand, written here as literals, and the derived quantities against the arithmetic of
ml/rf/main_train_rf.cxx:40-61 and ml/rf/ml_rf_train.cxx:362,376."""
import numpy as np

import _rfdef

ONES = [1.0, 1.0]


def _tree(X, y, mult=None, mtry=None, w=ONES, **kw):
    X = np.asarray(X, np.float64)
    d = _rfdef.derive(y, X.shape[1])
    return _rfdef.grow_tree(X, d["cls"], w, 0, mtry=X.shape[1] if mtry is None else mtry, mult=np.ones(len(X), np.int64) if mult is None else mult, **kw)


def test_four_rows_one_column():
    # cut between 0 and 1: nL = (2, 0), nR = (0, 2): crit = 4 / 2 + 4 / 2; the daughters are pure
    left, var, split, ncl = _tree([[0.0], [0.0], [1.0], [1.0]], [-1, -1, 1, 1])
    assert (left, var, split, ncl) == ([2, 0, 0], [1, 0, 0], [0.5, 0.0, 0.0], [0, 1, 2])


def test_equal_crit_in_two_variables_goes_to_the_lower_one():
    # both columns separate the classes perfectly (crit 4 each): variable 0 at 0.5, not variable 1 at 7
    X = [[0.0, 5.0], [0.0, 5.0], [1.0, 9.0], [1.0, 9.0]]
    assert _tree(X, [-1, -1, 1, 1]) == ([2, 0, 0], [1, 0, 0], [0.5, 0.0, 0.0], [0, 1, 2])
    Xr = [[r[1], r[0]] for r in X]
    assert _tree(Xr, [-1, -1, 1, 1]) == ([2, 0, 0], [1, 0, 0], [7.0, 0.0, 0.0], [0, 1, 2])


def test_equal_crit_at_two_cuts_goes_to_the_lower_value():
    # cut after 0: 1 / 1 + (1 + 1) / 2 = 2; cut after 1: (1 + 1) / 2 + 1 / 1 = 2 -> split 0.5; then {1, 2} splits at 1.5.  Level order:
    # node 0 root, 1 = leaf (-1), 2 = {1, 2} -> nodes 3 (class +1) and 4 (class -1)
    left, var, split, ncl = _tree([[0.0], [1.0], [2.0]], [-1, 1, -1])
    assert (left, var, split, ncl) == ([2, 0, 4, 0, 0], [1, 0, 1, 0, 0], [0.5, 0.0, 1.5, 0.0, 0.0], [0, 1, 0, 2, 1])


def test_adjacent_doubles_fall_back_to_the_lower_value():
    a = float(np.nextafter(1.0, 2.0))
    b = float(np.nextafter(a, 2.0))
    assert 0.5 * a + 0.5 * b == b                              # the midpoint rounds up (a's last bit is set) ...
    left, var, split, ncl = _tree([[a], [b], [a], [b]], [-1, 1, -1, 1])
    assert (left, var, ncl) == ([2, 0, 0], [1, 0, 0], [0, 1, 2]) and split == [a, 0.0, 0.0]      # ... so the split is x_a itself
    c = float(np.nextafter(b, 2.0))
    assert 0.5 * b + 0.5 * c == b                              # here it rounds down to x_a: no fallback needed, same answer
    assert _tree([[b], [c]], [-1, 1])[2] == [b, 0.0, 0.0]


def test_signed_zeros_are_one_value():
    # -0.0 and +0.0 hold both classes and cannot be separated: the only cut is between 0 and 1
    left, var, split, ncl = _tree([[-0.0], [0.0], [0.0], [-0.0], [1.0]], [-1, 1, -1, -1, 1])
    assert (left, var, split) == ([2, 0, 0], [1, 0, 0], [0.5, 0.0, 0.0])
    assert ncl == [0, 1, 2]                                    # left leaf: 3 x class -1 against 1 x class +1


def test_weights_multiplicities_and_terminal_rules():
    # crit from integer counts and weights: nL = (3, 0) with w = (1, 3) and nR = (0, 1): 9 / 3 + 9 / 3
    assert _rfdef.crit_of([1.0, 3.0], [3, 0], [0, 1]) == 6.0
    # a leaf's class is the largest w_k n_k, ties to the lowest class: 3 x (-1) against 1 x (+1) in one value
    X, y = [[2.0], [2.0], [2.0], [2.0]], [-1, -1, -1, 1]
    assert _tree(X, y, w=[1.0, 1.0])[3] == [1] and _tree(X, y, w=[1.0, 3.0])[3] == [1] and _tree(X, y, w=[1.0, 3.5])[3] == [2]
    assert _tree(X, y, mult=[1, 1, 0, 2])[3] == [1]             # 2 against 2: the tie goes to the lower class
    # nodesize counts distinct in-bag rows; max_depth stops at that depth
    X, y = [[0.0], [1.0], [2.0], [3.0]], [-1, 1, -1, 1]
    assert _tree(X, y, nodesize=4)[0] == [0] and _tree(X, y, nodesize=3)[0][0] == 2
    assert _tree(X, y, max_depth=1)[0] == [2, 0, 0] and len(_tree(X, y)[0]) == 7
    # rows out of the bag play no part: without row 1 the classes part between 2 and 3 (with it, the root cuts at 0.5: 1 + 5 / 3 there
    # and at 2.5, 2 at 1.5)
    assert _tree(X, y, mult=[1, 0, 1, 1])[:3] == ([2, 0, 0], [1, 0, 0], [2.5, 0.0, 0.0]) and _tree(X, y)[2][0] == 0.5


def test_derived_quantities():
    # (int)((float)N * 0.7 + 0.5): 2.6, 7.5, 701.2
    assert [_rfdef.sampsize_of(n, 0.7) for n in (3, 10, 1001)] == [2, 7, 701]
    assert _rfdef.sampsize_of(10, 0.0) == 10 and _rfdef.sampsize_of(10, 1e-7) == 10 and _rfdef.sampsize_of(10, 1.0) == 10
    # (double)maxcnt / (double)cnt
    assert _rfdef.class_weights([30, 10], 1) == [1.0, 3.0] and _rfdef.class_weights([10, 30], 1) == [3.0, 1.0]
    assert _rfdef.class_weights([30, 10], 0) == [1.0, 1.0]
    assert _rfdef.class_weights([7, 3], 1) == [1.0, 7.0 / 3.0]
    # floor(sqrt(D)), clamped to [1, D]
    assert [_rfdef.mtry_of(0, d) for d in (1, 104)] == [1, 10] and _rfdef.mtry_of(5, 1) == 1 and _rfdef.mtry_of(200, 104) == 10
    assert _rfdef.mtry_of(104, 104) == 104 and _rfdef.mtry_of(-3, 9) == 3
    d = _rfdef.derive([5, -1, 5, 5, 2, -1], 9)
    assert d["orig_labels"] == [-1, 2, 5] and list(d["cls"]) == [2, 0, 2, 2, 1, 0] and d["classwt"] == [1.5, 3.0, 1.0]
    assert d["cutoff"] == [1.0 / 3] * 3 and d["mtry"] == 3 and d["sampsize"] == 4


def test_random_numbers():
    # mix(0) is the first output of splitmix64 seeded with 0 (Steele, Lea & Flood 2014; the published test vector)
    assert _rfdef.mix(0) == 0xE220A8397B1DCDAF
    s = _rfdef.DEFAULT_SEED
    assert _rfdef.h(s, 2, 1, 5) == _rfdef.mix(_rfdef.mix(_rfdef.mix(_rfdef.mix(s) ^ 2) ^ 1) ^ 5)
    assert [int(v) for v in _rfdef.h_many(s, 2, 1, 7)] == [_rfdef.h(s, 2, 1, b) for b in range(7)]
    m = _rfdef.bootstrap(s, 3, 10, 7)
    assert m.sum() == 7 and list(m) == list(np.bincount([_rfdef.h(s, 3, 0, j) % 10 for j in range(7)], minlength=10))
    v = _rfdef.tried_variables(s, 0, 4, 104, 10)
    assert len(set(v)) == 10 and v == sorted(v) and v == _rfdef.tried_variables(s, 0, 4, 104, 10) != _rfdef.tried_variables(s, 0, 5, 104, 10)
    hs = sorted((_rfdef.h(s, 0, 5, b), b) for b in range(104))
    assert v == sorted(b for _, b in hs[:10])
    assert _rfdef.tried_variables(s, 1, 0, 3, 3) == [0, 1, 2]


def test_train_assembles_the_model_arrays():
    X = np.array([[0.0], [0.0], [1.0], [1.0]] * 8)
    y = np.array([-1, -1, 1, 1] * 8)
    m = _rfdef.train(X, y, ntree=3, sample_ratio=0)
    assert m["xbestsplit"].shape == (3, 3) and (m["ndbigtree"] == 3).all() and m["mtry"] == 1
    assert (m["treemap"] == [[2, 3], [0, 0], [0, 0]]).all() and (m["nodestatus"] == [1, -1, -1]).all() and (m["bestvar"] == [1, 0, 0]).all()
    assert (m["nodeclass"] == [0, 1, 2]).all() and (m["xbestsplit"] == [0.5, 0, 0]).all()
    assert list(m["orig_labels"]) == [-1, 1] and list(m["new_labels"]) == [1, 2] and list(m["cutoff"]) == [0.5, 0.5]
    assert (_rfdef.predict(m, X, -1) == (y == -1)).all() and _rfdef.walk(m, 0, [0.5]) == 1 and _rfdef.walk(m, 0, [0.5000001]) == 2
