"""-m gpu: batch forest prediction (glia_hmt_forest_predict / _device, glia_amd/csrc/forest_predict.hip; RandomForest.predict; cli/pred_rf)
against the oracle's walk of the same forest, row by row (O.forest_predict).  Votes are integers: every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cli")
N_ROWS = 1000
# tiles hold 64, 32, 16 or 8 rows (the largest that fits the LDS budget for the row length; 16 at most for an input this small):
# 1, the sizes around every tile height, and many tiles with a partial last one
N_CASES = (1, 8, 9, 16, 17, 33, 63, 64, 65, N_ROWS)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    c.close()


def _load(ctx, tmp, forests, **kw):
    """hmt.RandomForest of one forest dict or a list of three"""
    import _rf
    from glia_amd import hmt
    single = isinstance(forests, dict)
    paths = []
    for i, f in enumerate([forests] if single else forests):
        paths.append(os.path.join(str(tmp), "model%d_%d.bin" % (i, len(os.listdir(str(tmp))))))
        _rf.write_model(paths[-1], f)
    return hmt.RandomForest(ctx, paths[0] if single else paths, predict_label=-1, **kw)


def _oracle(forest, rows):
    from oracle import pyoracle as O
    f = O.make_forest(forest, -1)
    return np.array([O.forest_predict(f, r) for r in rows], np.float64)


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    # bit for bit (so -0.0 is not 0.0); a NaN equals a NaN whatever its sign and payload, which no arithmetic rule fixes
    return a.shape == b.shape and ((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all()


def _max_var(forest):
    return int((forest["bestvar"][forest["nodestatus"] == 1] - 1).max())


@pytest.fixture(scope="module")
def cases():
    """(rows [N_ROWS, dim], forest, oracle predictions) per (dim kind, ntree), computed once and never written to"""
    import _rf
    from glia_amd import hmt
    out = {}
    for kind, dim in (("maxvar+1", 40), ("104", 104), ("384", 384), ("above-staging", hmt.PREDICT_STAGE_MAX_DIM + 3)):
        rng = np.random.default_rng(dim)
        rows = rng.standard_normal((N_ROWS, dim))
        for ntree in (1, 15, 255):
            forest = _rf.random_forest(rng, ntree, 10 if ntree < 255 else 8, rows)
            r = rows
            if kind == "maxvar+1":
                r = np.ascontiguousarray(rows[:, :_max_var(forest) + 1])
            ref = _oracle(forest, r)
            assert 0.0 <= ref.min() and ref.max() <= 1.0 and (ntree == 1 or len(np.unique(ref)) > 2)
            for a in (r, ref):
                a.setflags(write=False)
            out[(kind, ntree)] = (r, forest, ref)
    return out


@pytest.mark.parametrize("ntree", [1, 15, 255])
@pytest.mark.parametrize("kind", ["maxvar+1", "104", "384", "above-staging"])
def test_shapes(ctx, cases, tmp_path, kind, ntree):
    import torch
    rows, forest, ref = cases[(kind, ntree)]
    if kind == "maxvar+1":
        assert rows.shape[1] == _max_var(forest) + 1
    clf = _load(ctx, tmp_path, forest)
    for n in N_CASES:
        assert _same(clf.predict(rows[:n]), ref[:n]), n
    d = torch.from_numpy(np.array(rows)).cuda()
    for n in (1, 65, N_ROWS):
        got = clf.predict(d[:n])
        assert got.is_cuda and _same(got.cpu().numpy(), ref[:n]), n


def test_small_inputs_take_small_tiles(cases):
    """what test_shapes runs: 16-row tiles (8 at 384 columns), none above the staging limit -- the taller tiles are test_tall_tiles'"""
    from glia_amd import hmt
    for n in N_CASES:
        assert hmt.predict_tile_rows(n, 104) == 16 and hmt.predict_tile_rows(n, 384) == 8 and hmt.predict_tile_rows(n, hmt.PREDICT_STAGE_MAX_DIM + 3) == 0


# (rows, columns, tile height): inputs of at least 512 tiles keep the tallest tile that fits the LDS budget -- 32 rows at 104 columns (the
# initial-edge case of the benchmark), 64 rows up to 95 columns; the last tile is partial (23, 45 and 1 rows), 8 and 4 slots share the trees
TALL = [(16407, 104, 32), (32813, 95, 64), (32769, 40, 64)]


@pytest.fixture(scope="module")
def tall_cases():
    import _rf
    out = {}
    for n, dim, _ in TALL:
        rng = np.random.default_rng(n)
        rows = rng.standard_normal((n, dim))
        rows[rng.integers(0, n, 50), rng.integers(0, dim, 50)] = np.nan
        forest = _rf.random_forest(rng, 9, 8, rows[:400])
        ref = _oracle(forest, rows)
        assert len(np.unique(ref)) > 4
        out[(n, dim)] = (rows, forest, ref)
    return out


@pytest.mark.parametrize("n,dim,tile", TALL)
def test_tall_tiles(ctx, tall_cases, tmp_path, n, dim, tile):
    """the staged kernel at its 32- and 64-row tiles: host entry, device entry, device entry with a row stride and poisoned padding"""
    import torch
    from glia_amd import hmt
    rows, forest, ref = tall_cases[(n, dim)]
    assert hmt.predict_tile_rows(n, dim) == tile and n % tile != 0
    clf = _load(ctx, tmp_path, forest)
    assert _same(clf.predict(rows), ref)
    d = torch.from_numpy(rows).cuda()
    assert _same(clf.predict(d).cpu().numpy(), ref)
    buf = torch.full((n, dim + 3), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :dim] = d
    assert buf[:, :dim].stride(0) == dim + 3 and _same(clf.predict(buf[:, :dim]).cpu().numpy(), ref)
    # one row fewer than 512 tiles' worth: the next smaller tile, the same answers
    m = 511 * tile
    assert hmt.predict_tile_rows(m, dim) == tile // 2 and _same(clf.predict(d[:m]).cpu().numpy(), ref[:m])


def test_tall_tiles_ensemble(ctx, tmp_path):
    """three forests of different sizes under 64-row tiles: the lanes of a slot walk different models"""
    import _rf
    import torch
    from glia_amd import hmt
    from oracle import pyoracle as O
    rng = np.random.default_rng(77)
    n, dim, dim0, dim1, thr = 32791, 50, 3, 47, 0.25
    rows = rng.standard_normal((n, dim))
    rows[:3000, dim0] = thr
    rows[2000:5000, dim1] = thr
    forests = [_rf.random_forest(rng, nt, 7, rows[:400]) for nt in (3, 10, 5)]
    pick = np.array([O.pick_model(dim0, dim1, thr, r) for r in rows])
    ref = np.choose(pick, [_oracle(f, rows) for f in forests])
    assert hmt.predict_tile_rows(n, dim) == 64 and len(set(pick[:64].tolist())) > 1 and set(pick.tolist()) == {0, 1, 2}
    clf = _load(ctx, tmp_path, forests, distributor_args=(dim0, dim1, thr))
    assert _same(clf.predict(rows), ref) and _same(clf.predict(torch.from_numpy(rows).cuda()).cpu().numpy(), ref)


def test_staging_limit_is_the_declared_one(ctx, tmp_path):
    """GLIA_HMT_PREDICT_STAGE_MAX_DIM (include/glia_hmt.h) = hmt.PREDICT_STAGE_MAX_DIM = what the library does: the longest staged row
    and the first one that is walked from global memory, both against the oracle"""
    import _rf
    from glia_amd import hmt
    lim = hmt.PREDICT_STAGE_MAX_DIM
    hdr = open(os.path.join(ROOT, "include", "glia_hmt.h")).read()
    assert "#define GLIA_HMT_PREDICT_STAGE_MAX_DIM %d\n" % lim in hdr
    rng = np.random.default_rng(lim)
    for dim, tile in ((lim, 8), (lim + 1, 0)):
        assert hmt.predict_tile_rows(70, dim) == tile and hmt.predict_tile_rows(10 ** 7, dim) == tile
        rows = rng.standard_normal((70, dim))
        forest = _rf.random_forest(rng, 5, 8, rows)
        assert _max_var(forest) > dim - 60                       # the last columns are read
        assert _same(_load(ctx, tmp_path, forest).predict(rows), _oracle(forest, rows))


def test_mincap_chunks_and_remainder(ctx, cases, tmp_path):
    """GLIA_HMT_MINCAP: the host entry streams 256 rows at a time -- three full chunks and a remainder of 232"""
    from glia_amd import hmt
    rows, forest, ref = cases[("104", 15)]
    clf = _load(ctx, tmp_path, forest)
    with hmt.options(GLIA_HMT_MINCAP=1):
        assert _same(clf.predict(rows), ref)
        assert _same(clf.predict(rows[:257]), ref[:257]) and _same(clf.predict(rows[:256]), ref[:256])


@pytest.mark.parametrize("kind", ["104", "above-staging"])
def test_device_entry_row_stride_with_poisoned_padding(ctx, cases, tmp_path, kind):
    import torch
    rows, forest, ref = cases[(kind, 15)]
    dim = rows.shape[1]
    for pad, poison in ((5, float("nan")), (1, -1e300)):
        buf = torch.full((N_ROWS, dim + pad), poison, dtype=torch.float64, device="cuda")
        buf[:, :dim] = torch.from_numpy(np.array(rows)).cuda()
        view = buf[:, :dim]
        assert view.stride(0) == dim + pad
        assert _same(_load(ctx, tmp_path, forest).predict(view).cpu().numpy(), ref)


def _level_forest(rng, ntree, depth, splits):
    """complete trees whose nodes of depth l all test variable l against splits[l]; random leaf classes"""
    nrn = 2 ** (depth + 1) - 1
    f = dict(xbestsplit=np.zeros((ntree, nrn)), treemap=np.zeros((ntree, nrn, 2), np.int32), nodestatus=np.full((ntree, nrn), -1, np.int32),
             nodeclass=np.zeros((ntree, nrn), np.int32), bestvar=np.zeros((ntree, nrn), np.int32), ndbigtree=np.full(ntree, nrn, np.int32),
             orig_labels=np.array([-1, 1], np.int32))
    for k in range(nrn):
        lvl = int(np.log2(k + 1))
        if lvl < depth:
            f["nodestatus"][:, k] = 1
            f["bestvar"][:, k] = lvl + 1
            f["xbestsplit"][:, k] = splits[lvl]
            f["treemap"][:, k] = (2 * k + 2, 2 * k + 3)        # 1-based daughters
        else:
            f["nodeclass"][:, k] = rng.integers(1, 3, ntree)
    return f


def test_ties_and_special_values(ctx, tmp_path):
    """x[var] == split at every node of the path of every tree (left: <=), its two neighbours, NaN (right), +-inf, -0.0 against +0.0"""
    rng = np.random.default_rng(5)
    depth = 6
    splits = np.array([0.0, 0.5, -1.25, 3.0, 1e-300, -7.0])
    forest = _level_forest(rng, 15, depth, splits)
    pool = np.stack([splits, np.nextafter(splits, np.inf), np.nextafter(splits, -np.inf), np.full(depth, np.nan), np.full(depth, np.inf),
                     np.full(depth, -np.inf), np.full(depth, -0.0), np.full(depth, 0.0)])
    rows = pool[rng.integers(0, len(pool), (300, depth)), np.arange(depth)]
    rows[0] = splits                       # the tie at every level
    rows[1] = -0.0
    rows[2] = np.nan
    rows = np.concatenate([rows, rng.standard_normal((300, 3))], axis=1)          # columns no tree reads
    ref = _oracle(forest, rows)
    # known answers, the oracle aside: a tie or -0.0 <= +0.0 goes left at every level (leaf 2^depth - 1), a NaN right (the last leaf)
    first, last = 2 ** depth - 1, 2 ** (depth + 1) - 2
    assert ref[0] == (forest["nodeclass"][:, first] == 1).mean() and ref[2] == (forest["nodeclass"][:, last] == 1).mean()
    assert _same(_load(ctx, tmp_path, forest).predict(rows), ref)


def test_single_terminal_node_trees(ctx, tmp_path):
    rng = np.random.default_rng(6)
    forest = _level_forest(rng, 4, 0, np.zeros(0))
    forest["nodeclass"][:, 0] = (1, 2, 1, 1)
    rows = rng.standard_normal((70, 3))
    got = _load(ctx, tmp_path, forest).predict(rows)
    assert _same(got, np.full(70, 0.75)) and _same(got, _oracle(forest, rows))
    assert _same(_load(ctx, tmp_path, forest).predict(rows[:, :1]), np.full(70, 0.75))       # no variable is read: one column is enough


def test_ensemble_of_three_with_rows_on_the_threshold(ctx, tmp_path):
    """opt::ThresholdModelDistributor (type/function.hxx:71-85): model 0 iff x[dim1] < thr, else 1 iff x[dim0] < thr, else 2"""
    import _rf
    from oracle import pyoracle as O
    rng = np.random.default_rng(8)
    dim, dim0, dim1, thr = 50, 3, 47, 0.25
    rows = rng.standard_normal((600, dim))
    edge = np.array([thr, np.nextafter(thr, 1.0), np.nextafter(thr, 0.0), np.nan])
    rows[:200, dim0] = edge[rng.integers(0, 4, 200)]
    rows[100:300, dim1] = edge[rng.integers(0, 4, 200)]
    forests = [_rf.random_forest(rng, nt, 7, rows) for nt in (7, 64, 255)]
    pick = np.array([O.pick_model(dim0, dim1, thr, r) for r in rows])
    assert set(pick.tolist()) == {0, 1, 2} and set(pick[100:200].tolist()) == {0, 1, 2}
    refs = [_oracle(f, rows) for f in forests]
    ref = np.choose(pick, refs)
    clf = _load(ctx, tmp_path, forests, distributor_args=(dim0, dim1, thr))
    assert _same(clf.predict(rows), ref)
    import torch
    assert _same(clf.predict(torch.from_numpy(rows).cuda()).cpu().numpy(), ref)
    # a distributor dimension beyond the row is an argument error
    from glia_amd import hmt
    with pytest.raises(hmt.HmtError) as e:
        clf.predict(rows[:, :dim1])
    assert e.value.code == hmt.ERR_ARG


def test_stub_classifier(ctx):
    import torch
    from glia_amd import hmt
    rows = np.random.default_rng(9).standard_normal((N_ROWS, 104))
    rows[3, 31] = np.nan
    stub = hmt.FeatureStubClassifier(ctx, 31)
    assert _same(stub.predict(rows), 1.0 - rows[:, 31])
    assert _same(stub.predict(torch.from_numpy(rows).cuda()).cpu().numpy(), 1.0 - rows[:, 31])
    with pytest.raises(hmt.HmtError) as e:
        stub.predict(rows[:, :31])
    assert e.value.code == hmt.ERR_ARG


def test_errors_and_empty_input(ctx, cases, tmp_path):
    from glia_amd import hmt
    rows, forest, ref = cases[("104", 15)]
    clf = _load(ctx, tmp_path, forest)
    with pytest.raises(hmt.HmtError) as e:
        clf.predict(rows[:, :_max_var(forest)])                 # dim == max_var: the last variable is out of the row
    assert e.value.code == hmt.ERR_ARG and "column" in str(e.value)
    out = np.empty(4)
    L = hmt.lib()
    r4 = np.ascontiguousarray(rows[:4])
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.glia_hmt_forest_predict(ctx.h, None, ptr(r4), C.c_int64(4), C.c_int(104), ptr(out)) == hmt.ERR_ARG          # NULL forest
    assert L.glia_hmt_forest_predict_device(ctx.h, None, None, C.c_int64(4), C.c_int(104), C.c_int64(104), None) == hmt.ERR_ARG
    assert L.glia_hmt_forest_predict_device(ctx.h, clf.h, None, C.c_int64(0), C.c_int(104), C.c_int64(100), None) == hmt.ERR_ARG   # stride < dim
    assert L.glia_hmt_forest_predict(ctx.h, clf.h, None, C.c_int64(0), C.c_int(104), None) == 0                            # no rows: ok
    assert clf.predict(rows[:0]).shape == (0,)


def _gpu_rm(ctx, labels, pb):
    import torch
    from glia_amd import hmt
    d_lab = torch.from_numpy(labels.view(np.int32)).cuda()
    d_pb = torch.from_numpy(pb).cuda()
    cfg = hmt.make_config(d_pb, rb=[(d_pb, 8, 0.0, 1.0)])
    return hmt.RegionMap(ctx, d_lab, pb=d_pb, cfg=cfg)


def test_consistent_with_the_classifier_loop(ctx, tmp_path):
    """the rows merge_order_bc scored its merges with, scored again: the saliencies bit for bit"""
    import _rf
    from oracle import pyoracle as O
    labels, pb = O.synth((24, 24, 24), 8, 16)
    cfg = O.make_cfg(pb, rb=[(pb, 8, 0.0, 1.0)])
    _, _, f0 = O.Rag(labels).merge_order_bc(cfg, None, stub_index=31, want_feats=True)
    clf = _load(ctx, tmp_path, _rf.random_forest(np.random.default_rng(7), 63, 8, f0))
    order, sal, rows = _gpu_rm(ctx, labels, pb).merge_order_bc(clf, want_feats=True)
    assert len(order) > 10 and rows.shape == (len(order), 104) and len(np.unique(sal)) > 5
    assert _same(clf.predict(rows), sal)


def test_pipeline_pb_order_bc_feat_predict(ctx, tmp_path):
    """merge_order_pb -> bc_feat -> pred_rf: the predictions of the oracle's rows (splits lie between observed values, so the last-ulp
    differences of the entropy columns decide no walk)"""
    import _rf
    from oracle import pyoracle as O
    labels, pb = O.synth((24, 24, 24), 8, 16)
    cfg = O.make_cfg(pb, rb=[(pb, 8, 0.0, 1.0)])
    rm = _gpu_rm(ctx, labels, pb)
    order, _ = rm.merge_order_pb(type=2)
    rows_ref = O.Rag(labels).bc_feat(cfg, order)
    forest = _rf.random_forest(np.random.default_rng(11), 31, 8, rows_ref)
    assert _same(_load(ctx, tmp_path, forest).predict(rm.bc_feat(order)), _oracle(forest, rows_ref))


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "-C", CLI])
    return CLI


def _write_rows(path, rows):
    with open(path, "w") as f:
        for r in rows:
            f.write("".join("%.17g " % v for v in r) + "\n")      # writeData(..., " ", "\n"): every element followed by the delimiter


def _expected_bytes(tools, tmp, values):
    """bytes of writeDoubles(file, values, n, 8): the same ostream at precision 8 writes the rows of cli/text_io_check (whose bytes the CPU
    suite pins against the reference's writer) -- one column, every value followed by a blank that writeDoubles does not write"""
    d = os.path.join(str(tmp), "expect%d" % len(os.listdir(str(tmp))))
    os.mkdir(d)
    text = "0\n0\n%d 1\n" % len(values) + "".join("%.17g\n" % v for v in values)
    subprocess.run([os.path.join(tools, "text_io_check"), d], input=text.encode(), check=True)
    return open(os.path.join(d, "feats.txt"), "rb").read().replace(b" ", b"")


def test_pred_rf_cli(tools, cases, tmp_path):
    import _rf
    rows, forest, ref = cases[("104", 15)]
    model, f0, f1, f2, p0, p1, p2 = (str(tmp_path / n) for n in ("m.bin", "f0.txt", "f1.txt", "f2.txt", "p0.txt", "p1.txt", "p2.txt"))
    _rf.write_model(model, forest)
    _write_rows(f0, rows[:300])
    _write_rows(f1, rows[300:307])
    open(f2, "w").close()                                          # an empty file gives an empty output
    subprocess.check_call([os.path.join(tools, "pred_rf"), "--m", model, "--f", f0, f1, f2, "--l", "-1", "--p", p0, p1, p2])
    assert open(p0, "rb").read() == _expected_bytes(tools, tmp_path, ref[:300])
    assert open(p1, "rb").read() == _expected_bytes(tools, tmp_path, ref[300:307])
    assert open(p2, "rb").read() == b""
    assert len(set(open(p0).read().split())) > 3
    # rows of unequal length
    with open(f1, "a") as f:
        f.write("1 2 3 \n")
    r = subprocess.run([os.path.join(tools, "pred_rf"), "--m", model, "--f", f1, "--l", "-1", "--p", p1], capture_output=True)
    assert r.returncode == 1 and b"dimension" in r.stderr
    # usage errors: a required option missing; several models without the three --md values (the reference's message, exit status 1)
    r = subprocess.run([os.path.join(tools, "pred_rf"), "--m", model, "--f", f0, "--p", p0], capture_output=True)
    assert r.returncode == 1 and b"'--l' is required" in r.stderr
    r = subprocess.run([os.path.join(tools, "pred_rf"), "--m", model, model, model, "--md", "0", "1", "--f", f0, "--l", "-1", "--p", p0], capture_output=True)
    assert r.returncode == 1 and b"Error: model distributor needs 3 arguments..." in r.stderr


def test_pred_rf_cli_ensemble(tools, tmp_path):
    import _rf
    from oracle import pyoracle as O
    rng = np.random.default_rng(12)
    rows = rng.standard_normal((120, 20))
    rows[:40, 2] = 0.5
    rows[20:60, 9] = 0.5
    forests = [_rf.random_forest(rng, nt, 6, rows) for nt in (3, 31, 8)]
    models = [str(tmp_path / ("m%d.bin" % i)) for i in range(3)]
    for m, f in zip(models, forests):
        _rf.write_model(m, f)
    feats, preds = str(tmp_path / "f.txt"), str(tmp_path / "p.txt")
    _write_rows(feats, rows)
    subprocess.check_call([os.path.join(tools, "pred_rf"), "--m"] + models + ["--md", "2", "9", "0.5", "--f", feats, "--l", "-1", "--p", preds])
    pick = np.array([O.pick_model(2, 9, 0.5, r) for r in rows])
    assert set(pick.tolist()) == {0, 1, 2}
    ref = np.choose(pick, [_oracle(f, rows) for f in forests])
    assert open(preds, "rb").read() == _expected_bytes(tools, tmp_path, ref)
