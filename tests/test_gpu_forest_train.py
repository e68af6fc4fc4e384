"""-m gpu: train_forest (glia_hmt_forest_train, glia_amd/csrc/forest_train.hip) against the growing rule's second author, tests/_rfdef.py:
every model array equal -- integers ==, xbestsplit / classwt / cutoff bit for bit -- on the smallest shapes at which each mechanism of
the trainer can break, plus determinism, a known answer through the device predictor, and structural properties at a size the Python
definition is too slow for.

The table of cases names `N = 1` and `N = 2 of one class` as root-terminal cases; the definition refuses fewer than two distinct labels,
so those two inputs are checked to BE refused, and the root-terminal paths they stand for (one in-bag row; one in-bag class) are reached
with two-class inputs whose bootstrap holds a single row or a single class."""
import numpy as np
import pytest

import _rfdef

pytestmark = pytest.mark.gpu
TREE_KEYS = ("treemap", "nodestatus", "nodeclass", "bestvar", "ndbigtree", "orig_labels", "new_labels")
BIT_KEYS = ("xbestsplit", "classwt", "cutoff")


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    c.close()


def _differences(got, want):
    bad = [k for k in TREE_KEYS if got[k].shape != want[k].shape or not (got[k] == want[k]).all()]
    bad += [k for k in BIT_KEYS if got[k].shape != want[k].shape or
            not (np.ascontiguousarray(got[k], np.float64).view(np.uint64) == np.ascontiguousarray(want[k], np.float64).view(np.uint64)).all()]
    if got["mtry"] != want["mtry"]:
        bad.append("mtry")
    return bad


def _noisy(rng, n, d, nclass=2, flip=0.15):
    X = rng.normal(size=(n, d))
    score = X[:, 0] + 0.5 * X[:, d - 1]
    y = np.digitize(score, np.quantile(score, np.linspace(0, 1, nclass + 1)[1:-1]))
    noise = rng.random(n) < flip
    y[noise] = rng.integers(0, nclass, noise.sum())
    labels = np.array([-1, 1] if nclass == 2 else [-1, 1, 4, 7, 9][:nclass])
    return X, labels[y].astype(np.int32)


def _cases():
    rng = np.random.default_rng(20261020)
    c = {}
    c["constant_columns"] = (np.full((10, 3), 2.5), np.array([-1, 1] * 5, np.int32), dict(ntree=3))
    c["one_in_bag_row"] = (np.array([[0.0], [1.0]]), np.array([-1, 1], np.int32), dict(ntree=4, sample_ratio=0.5))        # sampsize 1
    c["two_rows_one_cut"] = (np.array([[0.0], [1.0]]), np.array([-1, 1], np.int32), dict(ntree=7, sample_ratio=0))        # some bags hold one class
    X = rng.integers(0, 4, (200, 6)).astype(np.float64)
    c["heavy_repeats"] = (X, np.where(X[:, 0] + X[:, 1] + rng.integers(0, 3, 200) > 4, 1, -1).astype(np.int32), dict(ntree=3, mtry=6))
    c["signed_zeros"] = (np.array([[-0.0], [0.0], [-0.0], [0.0], [1.0], [-0.0], [0.0], [-1.0]]), np.array([-1, 1, 1, -1, 1, -1, -1, 1], np.int32),
                         dict(ntree=5, sample_ratio=0))
    a = np.nextafter(1.0, 2.0)
    b = np.nextafter(a, 2.0)                 # 0.5 a + 0.5 b rounds to b (a's last bit is set): the split falls back to a
    c["adjacent_doubles"] = (np.array([[a], [a], [a], [b], [b], [b]]), np.array([-1, -1, -1, 1, 1, 1], np.int32), dict(ntree=4, sample_ratio=0))
    for n in (63, 64, 65, 257, 1000):
        c["rows_%d" % n] = _noisy(rng, n, 8) + (dict(ntree=2),)
    c["row_width_104"] = _noisy(rng, 600, 104) + (dict(ntree=2, mtry=0),)
    c["mtry_clamp"] = _noisy(rng, 80, 1) + (dict(ntree=2, mtry=5),)
    c["three_classes"] = _noisy(rng, 300, 5, nclass=3) + (dict(ntree=2),)
    X = rng.normal(size=(300, 4))
    y = np.where(rng.random(300) < 0.1, 1, -1).astype(np.int32)       # about 9 : 1, not separable: the weights decide the leaves
    y[:3] = 1
    c["balance_0"] = (X, y, dict(ntree=2, balance=0, nodesize=5))
    c["balance_1"] = (X, y, dict(ntree=2, balance=1, nodesize=5))
    X, y = _noisy(rng, 200, 6)
    c["nodesize_1"] = (X, y, dict(ntree=2, nodesize=1))
    c["nodesize_5"] = (X, y, dict(ntree=2, nodesize=5))
    for sr in (0.7, 1.0, 0.0):
        c["sample_ratio_%g" % sr] = (X, y, dict(ntree=2, sample_ratio=sr))
    c["max_depth_2"] = (X, y, dict(ntree=3, max_depth=2))
    X = np.stack([np.arange(300, dtype=np.float64), np.full(300, 7.0)], axis=1)
    c["staircase"] = (X, _staircase_labels(300, STAIRCASE_SEED), dict(ntree=1, mtry=2, sample_ratio=0, seed=STAIRCASE_SEED))
    return c


STAIRCASE_SEED = 1


def _staircase_labels(n, seed):
    """Labels over rows sorted by their one informative column that alternate in short runs, the runs cut so that the class balance
    WEIGHTED BY THE TREE'S OWN BOOTSTRAP stays inside a band one unit wide at every prefix.  No cut in the middle of a node then gains
    anything to speak of, and the best cut peels the run at an end: one pure leaf and one more level per split.  (Plain alternation does
    not do this: the multiplicities unbalance the halves and the best cuts fall in the middle -- 21 levels at 300 rows.)"""
    mult = _rfdef.bootstrap(seed, 0, n, n)
    cls = np.zeros(n, np.int64)
    balance, c = 0, 0
    for i in range(n):
        cls[i] = c
        balance += mult[i] if c == 0 else -mult[i]
        if (c == 0 and balance >= 1) or (c == 1 and balance <= 0):
            c ^= 1
    return np.where(cls == 0, -1, 1).astype(np.int32)


def _levels(treemap, n):
    """nodes on every level of a tree (root = level 0)"""
    depth = np.zeros(n, np.int64)
    for k in range(n):
        if treemap[k, 0]:
            depth[treemap[k] - 1] = depth[k] + 1
    return np.bincount(depth)


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_equals_the_definition(ctx, name):
    from glia_amd import hmt
    X, y, opts = CASES[name]
    want = _rfdef.train(X, y, **opts)
    got = hmt.train_forest(ctx, X, y, **opts).arrays()
    assert _differences(got, want) == []
    if name == "staircase":       # the case is what its name says: more than a hundred levels of a few nodes each, one launch round per level
        per_level = _levels(want["treemap"][0], want["ndbigtree"][0])
        assert len(per_level) >= 100 and per_level.max() <= 8
        assert (_levels(got["treemap"][0], got["ndbigtree"][0]) == per_level).all()
        assert hmt.last_forest_train_timing(ctx)["levels"] == len(per_level)
    if name in ("constant_columns", "one_in_bag_row"):
        assert (got["ndbigtree"] == 1).all()
    if name == "adjacent_doubles":
        a = np.nextafter(1.0, 2.0)
        assert ((got["xbestsplit"][got["nodestatus"] == 1]) == a).all() and (got["nodestatus"] == 1).any()


@pytest.mark.parametrize("rows,labels", [(np.zeros((1, 2)), [1]), (np.array([[0.0], [1.0]]), [1, 1])])
def test_fewer_than_two_classes_are_refused(ctx, rows, labels):
    from glia_amd import hmt
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_forest(ctx, rows, np.array(labels, np.int32))
    assert e.value.code == hmt.ERR_ARG and "two classes" in str(e.value)


def test_invalid_inputs_are_refused_with_a_message(ctx):
    from glia_amd import hmt
    X, y = np.array([[0.0, 1.0], [1.0, np.nan]]), np.array([-1, 1], np.int32)
    for rows, labels, opts, word in ((X, y, {}, "non-finite"), (np.array([[0.0, np.inf], [1.0, 0.0]]), y, {}, "non-finite"),
                                     (np.zeros((0, 2)), y[:0], {}, "0 rows"), (np.zeros((2, 0)), y, {}, "0 columns"),
                                     (np.arange(9.0).reshape(9, 1), np.arange(9, dtype=np.int32), {}, "more than 8 classes"),
                                     (np.array([[0.0], [1.0]]), y, dict(sample_ratio=0.1), "sample size"),
                                     (np.array([[0.0], [1.0]]), y, dict(sample_ratio=2.0), "sample size")):
        with pytest.raises(hmt.HmtError) as e:
            hmt.train_forest(ctx, rows, labels, **opts)
        assert e.value.code == hmt.ERR_ARG and word in str(e.value), (word, str(e.value))


def test_trees_do_not_depend_on_how_many_are_grown_together(ctx):
    """tree t of a 7-tree forest = tree t of its own seed, whether 7, 2 or 1 trees are in flight; another seed gives other trees"""
    from glia_amd import hmt
    X, y, _ = CASES["rows_257"]
    seven = hmt.train_forest(ctx, X, y, ntree=7).arrays()
    one = hmt.train_forest(ctx, X, y, ntree=1).arrays()
    n = one["ndbigtree"][0]
    assert n == seven["ndbigtree"][0]
    for k in ("xbestsplit", "treemap", "nodestatus", "nodeclass", "bestvar"):
        assert (one[k][0, :n] == seven[k][0, :n]).all()
    for in_flight in ("1", "2"):
        hmt.set_option("GLIA_HMT_TRAIN_TREES", in_flight)
        try:
            again = hmt.train_forest(ctx, X, y, ntree=7).arrays()
            assert hmt.last_forest_train_timing(ctx)["trees_in_flight"] == int(in_flight)
        finally:
            hmt.set_option("GLIA_HMT_TRAIN_TREES", None)
        assert _differences(again, seven) == []
    for t in (3, 6):
        want = _rfdef.train(X, y, ntree=1, first_tree=t)
        n = want["ndbigtree"][0]
        assert n == seven["ndbigtree"][t]
        for k in ("treemap", "nodestatus", "nodeclass", "bestvar"):
            assert (want[k][0, :n] == seven[k][t, :n]).all()
        assert (want["xbestsplit"][0, :n].view(np.uint64) == seven["xbestsplit"][t, :n].view(np.uint64)).all()
    other = hmt.train_forest(ctx, X, y, ntree=7, seed=12345).arrays()
    assert _differences(other, seven) != []


def test_two_calls_write_identical_files(ctx, tmp_path):
    from glia_amd import hmt
    X, y, opts = CASES["rows_1000"]
    files = []
    for i in range(2):
        files.append(str(tmp_path / ("m%d.bin" % i)))
        hmt.train_forest(ctx, X, y, ntree=5).write(files[-1])
    assert open(files[0], "rb").read() == open(files[1], "rb").read()
    loaded = hmt.RandomForest(ctx, files[0], predict_label=-1)      # load_forest_file reads the writer's output
    model = hmt.train_forest(ctx, X, y, ntree=5)
    assert (loaded.predict(X) == model.forest(-1).predict(X)).all()


def test_known_answer_through_the_predictor(ctx):
    from glia_amd import hmt
    rng = np.random.default_rng(5)
    X = rng.normal(size=(512, 5))
    X[:, 3] = rng.integers(0, 2, 512)
    y = np.where(X[:, 3] == 0, -1, 1).astype(np.int32)
    model = hmt.train_forest(ctx, X, y, mtry=5, ntree=15)
    a = model.arrays()
    assert (a["ndbigtree"] == 3).all() and a["xbestsplit"].shape == (15, 3)
    assert (a["bestvar"][:, 0] == 4).all() and (a["xbestsplit"][:, 0] == 0.5).all()
    assert (a["nodestatus"] == [1, -1, -1]).all() and (a["nodeclass"] == [0, 1, 2]).all() and (a["treemap"][:, 0] == [2, 3]).all()
    p = model.forest(-1).predict(X)
    assert (p[y == -1] == 1.0).all() and (p[y == 1] == 0.0).all()


def test_device_predictor_agrees_with_the_plain_walk(ctx):
    from glia_amd import hmt
    X, y, _ = CASES["rows_257"]
    model = hmt.train_forest(ctx, X, y, ntree=7)
    rows = np.concatenate([X, np.random.default_rng(9).normal(size=(100, X.shape[1]))])
    for label in (-1, 1):
        want = _rfdef.predict(model.arrays(), rows, label)
        assert (model.forest(label).predict(rows) == want).all()          # exact k / ntree


def test_properties_of_a_large_forest(ctx):
    from glia_amd import hmt
    rng = np.random.default_rng(77)
    N, D, ntree = 20000, 104, 3
    X = rng.normal(size=(N, D))                                          # (no two rows alike: every leaf can be pure)
    y = np.where(X[:, 5] + 0.3 * rng.normal(size=N) > 0, 1, -1).astype(np.int32)
    a = hmt.train_forest(ctx, X, y, ntree=ntree, nodesize=1).arrays()
    d = _rfdef.derive(y, D)
    assert a["mtry"] == d["mtry"] == 10 and a["xbestsplit"].shape[1] == a["ndbigtree"].max()
    for t in range(ntree):
        n = int(a["ndbigtree"][t])
        st, tm, bv, nc = a["nodestatus"][t], a["treemap"][t], a["bestvar"][t], a["nodeclass"][t]
        inner = np.nonzero(st[:n] == 1)[0]
        leaf = np.nonzero(st[:n] == -1)[0]
        assert len(inner) + len(leaf) == n and n == 2 * len(inner) + 1
        assert (st[n:] == 0).all() and (tm[n:] == 0).all() and (bv[n:] == 0).all() and (nc[n:] == 0).all()
        # level order: the i-th splitting node (ascending) owns nodes 2 i + 1 and 2 i + 2
        assert (tm[inner, 0] == 2 * np.arange(len(inner)) + 2).all() and (tm[inner, 1] == tm[inner, 0] + 1).all()
        assert (bv[inner] >= 1).all() and (bv[inner] <= D).all() and (nc[inner] == 0).all()
        assert (tm[leaf] == 0).all() and (bv[leaf] == 0).all() and ((nc[leaf] == 1) | (nc[leaf] == 2)).all()
        # every in-bag row ends in a leaf of its own class
        mult = _rfdef.bootstrap(_rfdef.DEFAULT_SEED, t, N, d["sampsize"])
        rows = np.nonzero(mult)[0]
        at = np.zeros(len(rows), np.int64)
        for _ in range(n):
            go = st[at] == 1
            if not go.any():
                break
            k = at[go]
            right = X[rows[go], bv[k] - 1] > a["xbestsplit"][t][k]
            at[go] = tm[k, 0] - 1 + right
        assert (st[at] == -1).all() and (nc[at] - 1 == d["cls"][rows]).all()
        # the root against the definition
        crit, var, split, left, right = _rfdef.grow_tree(X, d["cls"], d["classwt"], t, sampsize=d["sampsize"], mtry=d["mtry"], root_only=True)
        assert bv[0] == var + 1 and np.float64(a["xbestsplit"][t][0]).view(np.uint64) == np.float64(split).view(np.uint64)
        goes_left = X[rows, var] <= a["xbestsplit"][t][0]
        assert goes_left.sum() == len(left) and (~goes_left).sum() == len(right)
