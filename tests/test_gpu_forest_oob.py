"""-m gpu: train_forest(oob=True, importance=True) (glia_hmt_forest_train_oob, glia_amd/csrc/forest_oob.hip) against the definition's
second author, tests/_rfoobdef.py: every integer array ==, every double bit for bit, and the model arrays those of a plain train_forest
call -- on the smallest shapes at which each mechanism of the passes can break.  Each case is named for what it breaks."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _rfdef
import _rfoobdef as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cli")
SEED = _rfdef.DEFAULT_SEED
TILE = 256                       # out-of-bag ranks per workgroup of the importance pass
TILE_EDGES_N, TILE_EDGES_TREES = 517, 8


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    assert hmt.Context.internal_errors() == 0
    c.close()


def _noisy(rng, n, d, nclass=2, flip=0.15):
    X = rng.normal(size=(n, d))
    score = X[:, 0] + 0.5 * X[:, d - 1]
    y = np.digitize(score, np.quantile(score, np.linspace(0, 1, nclass + 1)[1:-1]))
    noise = rng.random(n) < flip
    y[noise] = rng.integers(0, nclass, noise.sum())
    labels = np.array([-1, 1] if nclass == 2 else [-7, -1, 1, 4, 7, 9, 12, 30][:nclass])
    return X, labels[y].astype(np.int32)


def _cases():
    rng = np.random.default_rng(20261021)
    c = {}
    c["basic"] = _noisy(rng, 40, 3) + (dict(ntree=5),)
    c["never_oob"] = _noisy(rng, 30, 2) + (dict(ntree=2),)
    c["empty_and_single_oob"] = (np.array([[0.0], [1.0], [2.0]]), np.array([-1, 1, 1], np.int32), dict(ntree=40, sample_ratio=0))
    c["vote_ties"] = _noisy(rng, 60, 3, flip=0.4) + (dict(ntree=6),)
    c["eight_classes"] = _noisy(rng, 160, 4, nclass=8, flip=0.1) + (dict(ntree=4),)
    X = rng.normal(size=(12, 2))
    y = np.full(12, -1, np.int32)
    y[5] = 1
    c["single_leaf_trees"] = (X, y, dict(ntree=12))
    c["one_column"] = _noisy(rng, 80, 1) + (dict(ntree=4),)
    c["tile_edges"] = _noisy(rng, TILE_EDGES_N, 3) + (dict(ntree=TILE_EDGES_TREES, nodesize=5),)
    c["row_width_104"] = _noisy(rng, 600, 104) + (dict(ntree=3),)
    c["unstaged_rows"] = _noisy(rng, 120, 800) + (dict(ntree=2),)
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _want(name):
    """(model arrays, out-of-bag arrays, per-tree details) of the definition, computed once per case"""
    X, y, opts = CASES[name]
    model = _rfdef.train(X, y, **opts)
    details = {}
    return model, R.oob(X, y, model, details=details, **opts), details


def _model_differences(got, want):
    bad = [k for k in ("treemap", "nodestatus", "nodeclass", "bestvar", "ndbigtree", "orig_labels", "new_labels") if got[k].shape != want[k].shape or
           not (got[k] == want[k]).all()]
    bad += [k for k in ("xbestsplit", "classwt", "cutoff") if got[k].shape != want[k].shape or
            not (np.ascontiguousarray(got[k]).view(np.uint64) == np.ascontiguousarray(want[k], np.float64).view(np.uint64)).all()]
    return bad


def _m_of(name):
    X, y, opts = CASES[name]
    s = _rfdef.sampsize_of(len(y), opts.get("sample_ratio", 0.7))
    return [int((_rfdef.bootstrap(SEED, t, len(y), s) == 0).sum()) for t in range(opts["ntree"])]


@pytest.mark.parametrize("name", sorted(CASES))
def test_oob_outputs_equal_the_definition(ctx, name):
    from glia_amd import hmt
    X, y, opts = CASES[name]
    model, want, details = _want(name)
    trained = hmt.train_forest(ctx, X, y, oob=True, importance=True, **opts)
    got = trained.oob()
    assert R.differences(got, want) == []
    arrays = trained.arrays()
    assert _model_differences(arrays, model) == []
    tm = hmt.last_forest_oob_timing(ctx)
    assert _model_differences(hmt.train_forest(ctx, X, y, **opts).arrays(), arrays) == []
    m = _m_of(name)
    assert tm["oob_rows"] == sum(m) and tm["walks_nominal"] == sum(m) * X.shape[1] and 0 <= tm["walks_done"] <= tm["walks_nominal"]
    nclass = len(set(y.tolist()))
    D = X.shape[1]
    assert got["importance"].shape == (D, nclass + 2) and got["importanceSD"].shape == (D, nclass + 1) and got["errtr"].shape == (opts["ntree"], nclass + 1)
    assert got["counttr"].shape == (nclass, len(y)) and got["votes"].shape == (len(y), nclass)
    # the case is what its name says
    if name == "never_oob":
        never = got["oob_times"] == 0
        assert never.any() and (~never).any() and (got["outcl"][never] == 0).all() and (got["outcl"][~never] > 0).all()
    if name == "empty_and_single_oob":
        assert {0, 1} <= set(m)
    if name == "vote_ties":
        tie = (got["counttr"][0] == got["counttr"][1]) & (got["counttr"][0] > 0)
        assert tie.any() and (got["outcl"][tie] == 1).all()
    if name == "eight_classes":
        assert nclass == 8 and (got["counttr"].sum(axis=1) > 0).all()
    if name == "single_leaf_trees":
        leaf_only = arrays["ndbigtree"] == 1
        assert leaf_only.any() and (~leaf_only).any()
    if name == "one_column":
        assert (arrays["bestvar"][arrays["nodestatus"] == 1] == 1).all() and tm["walks_done"] >= sum(mt for mt, n in zip(m, arrays["ndbigtree"]) if n > 1)
    if name == "tile_edges":
        assert min(m) < TILE - 1 and TILE in m and max(m) > TILE + 1
    if name == "row_width_104":
        assert tm["walks_done"] < tm["walks_nominal"] // 4                     # a path tests a few of the 104 columns
    if name == "unstaged_rows":
        assert D * nclass > 1024 and D > 128                                   # the counters of a tree do not fit a workgroup's table


@pytest.mark.parametrize("flags", [(True, False), (False, True)])
def test_each_option_alone(ctx, flags):
    from glia_amd import hmt
    X, y, opts = CASES["basic"]
    _, want, _ = _want("basic")
    got = hmt.train_forest(ctx, X, y, oob=flags[0], importance=flags[1], **opts).oob()
    keys = (R.INT_KEYS + ("errtr",)) if flags[0] else ("importance", "importanceSD")
    assert sorted(got) == sorted(keys) and R.differences(got, {k: want[k] for k in keys}) == []
    with pytest.raises(hmt.HmtError):
        hmt.train_forest(ctx, X, y, **opts).oob()
    assert hmt.last_forest_oob_timing(ctx) == dict(ms_walk=0.0, ms_tally=0.0, ms_importance=0.0, oob_rows=0, walks_nominal=0, walks_done=0, device_bytes=0)


def test_batches(ctx):
    """GLIA_HMT_TRAIN_TREES = 2 with 5 trees: three batches, the counts carried from one to the next"""
    from glia_amd import hmt
    X, y, opts = CASES["basic"]
    _, want, _ = _want("basic")
    hmt.set_option("GLIA_HMT_TRAIN_TREES", "2")
    try:
        got = hmt.train_forest(ctx, X, y, oob=True, importance=True, **opts).oob()
        assert hmt.last_forest_train_timing(ctx)["batches"] == 3
    finally:
        hmt.set_option("GLIA_HMT_TRAIN_TREES", None)
    assert R.differences(got, want) == []


def test_determinism(ctx, tmp_path):
    from glia_amd import hmt
    X, y, opts = CASES["row_width_104"]
    files = []
    for i in range(2):
        files.append(str(tmp_path / ("m%d.bin" % i)))
        hmt.train_forest(ctx, X, y, oob=True, importance=True, **opts).write(files[-1])
    assert open(files[0], "rb").read() == open(files[1], "rb").read()
    plain = str(tmp_path / "plain.bin")
    hmt.train_forest(ctx, X, y, **opts).write(plain)
    data, head = open(files[0], "rb").read(), open(plain, "rb").read()
    assert len(data) > len(head) and data[520:len(head)] == head[520:]          # the arrays follow what the file always held


def test_cli(ctx, tmp_path):
    """train_rf --oob 1 --imp 1 --impf at 200 x 8: the numbers on stderr, the table, the model file's slots; pred_rf is unchanged"""
    from glia_amd import hmt
    from test_rf_oob_model_file import read_model_file
    subprocess.check_call(["make", "-C", CLI, "train_rf", "pred_rf"], stdout=subprocess.DEVNULL)
    X, y = _noisy(np.random.default_rng(8), 200, 8)
    p = lambda n: str(tmp_path / n)
    open(p("feats.txt"), "w").write("".join(" ".join("%.17g" % v for v in row) + "\n" for row in X))
    open(p("labels.txt"), "w").write("".join("%d\n" % v for v in y))
    run = lambda *argv: subprocess.run([os.path.join(CLI, argv[0])] + list(argv[1:]), capture_output=True, text=True, timeout=120)
    base = ("train_rf", "--f", p("feats.txt"), "--l", p("labels.txt"), "--nt", "7")
    r = run(*base, "--m", p("plain.bin"))
    assert r.returncode == 0 and "OOB" not in r.stderr, r.stderr
    r = run(*base, "--oob", "1", "--imp", "1", "--impf", p("imp.txt"), "--m", p("oob.bin"))
    assert r.returncode == 0, r.stderr
    trained = hmt.train_forest(ctx, X, y, ntree=7, oob=True, importance=True)
    got = trained.oob()
    last = got["errtr"][-1]
    lines = [ln for ln in r.stderr.split("\n") if ln.startswith("OOB")]
    assert lines == ["OOB error: %.6g" % last[0], "OOB error of class -1: %.6g" % last[1], "OOB error of class 1: %.6g" % last[2]]
    assert 0.0 < last[0] < 0.5
    table = "".join(" ".join("%.17g" % v for v in list(got["importance"][v]) + list(got["importanceSD"][v])) + "\n" for v in range(8))
    assert open(p("imp.txt")).read() == table
    trained.write(p("py.bin"))
    assert open(p("py.bin"), "rb").read() == open(p("oob.bin"), "rb").read()
    f = read_model_file(p("oob.bin"))
    assert f["counttr"][:2] == (2, 200) and (f["counttr"][2].reshape(2, 200) == got["counttr"]).all() and (f["errtr"][2].reshape(7, 3) == got["errtr"]).all()
    assert f["importance"][:2] == (8, 4) and (f["importance"][2].reshape(8, 4) == got["importance"]).all() and (f["oob_times"][2] == got["oob_times"]).all()
    preds = []
    for model in ("plain.bin", "oob.bin"):
        r = run("pred_rf", "--m", p(model), "--f", p("feats.txt"), "--l", "-1", "--p", p(model + ".pred"))
        assert r.returncode == 0, r.stderr
        preds.append(open(p(model + ".pred")).read())
    assert preds[0] == preds[1] and len(set(preds[0].split())) > 2
    assert (hmt.RandomForest(ctx, p("oob.bin"), predict_label=-1).predict(X) == trained.forest(-1).predict(X)).all()
    # --impf alone asks for the importances; the file then holds them and no out-of-bag group
    r = run(*base, "--impf", p("imp2.txt"), "--m", p("imp.bin"))
    assert r.returncode == 0 and "OOB" not in r.stderr and open(p("imp2.txt")).read() == table
    assert read_model_file(p("imp.bin"))["counttr"][:2] == (0, 0) and read_model_file(p("imp.bin"))["importance"][:2] == (8, 4)
