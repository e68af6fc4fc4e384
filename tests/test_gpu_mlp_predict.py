"""-m gpu: the MLP / logsig batch predictors (glia_hmt_mlp_predict / _device, glia_amd/csrc/mlp_predict.hip; hmt.MLP, hmt.Logsig) against
the second author of the definition (tests/_mlpdef.py).  Logits are compared bit for bit; the host-rows route also in its
probabilities (the sigmoid is the host's); the device-side sigmoid within DEVICE_SIGMOID_ULPS of the host's."""

import numpy as np
import pytest

import _mlpdef as D

pytestmark = pytest.mark.gpu
N_ROWS = 1000
# one row, a pair, the sizes around a tile of 64 rows (and of 32: wide layers take smaller tiles), several tiles with a partial last one.
# The further row tier -- a launch takes 2^23 tiles, more rows take further launches -- has tests of its own: test_second_launch (the
# real size) and test_small_chunks_and_launches (GLIA_HMT_MINCAP: 3 tiles per launch, 256 rows per host chunk).
N_CASES = (1, 2, 31, 32, 33, 63, 64, 65, 255, 257, N_ROWS)
# The largest distance, in ulps, between the device's 1 / (1 + exp(-h)) and the same expression through the host's libm, measured on an
# MI355X over the sweep of test_device_sigmoid: 3.  The bar is four times that: other libm and device-library versions.
DEVICE_SIGMOID_ULPS = 12


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    c.close()


_CACHE = {}


def _case(dim, n1, n2, n_models=1, n_rows=N_ROWS):
    """(weights, rows, mn, mx, {rescale: reference logits [, picks]}) -- computed once, read-only"""
    key = (dim, n1, n2, n_models, n_rows)
    if key not in _CACHE:
        w, rows, mn, mx = D.random_case(dim, n1, n2, n_rows=n_rows, n_models=n_models)
        ref = {}
        for rescale in (False, True):
            mm = (mn, mx) if rescale else (None, None)
            r = D.logits(w, n1, n2, rows, *mm, dist=D.DIST if n_models == 3 else None, want_pick=True)
            for a in r:
                a.setflags(write=False)
            ref[rescale] = r
        _CACHE[key] = (w, rows, mn, mx, ref)
    return _CACHE[key]


def _model(ctx, w, n1, n2, mn=None, mx=None, dist=None):
    from glia_amd import hmt
    return hmt.MLP.from_arrays(ctx, w, n1, n2, mn, mx, dist)


def _device_logits(clf, rows, stride=None):
    """logits (and predictions) of device rows, optionally at a padded stride whose padding holds NaN"""
    import torch
    rows = np.asarray(rows)
    if stride is None:
        d = torch.from_numpy(np.array(rows)).cuda()
    else:
        buf = np.full((rows.shape[0], stride), np.nan)
        buf[:, :rows.shape[1]] = rows
        d = torch.from_numpy(buf).cuda()[:, :rows.shape[1]]
        assert d.stride(0) == stride or rows.shape[0] <= 1
    pred, logit = clf.predict(d, want_logits=True)
    return pred.cpu().numpy(), logit.cpu().numpy()


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("dim,n1,n2", D.SIZES)
def test_sizes_and_row_counts(ctx, dim, n1, n2, rescale):
    w, rows, mn, mx, ref = _case(dim, n1, n2)
    want = ref[rescale][0]
    clf = _model(ctx, w, n1, n2, *((mn, mx) if rescale else (None, None)))
    assert clf.dim == dim
    for n in N_CASES:
        assert D.same(_device_logits(clf, rows[:n])[1], want[:n]), n
    # the host-rows route: logits and probabilities, the sigmoid is the host's
    pred, logit = clf.predict(rows, want_logits=True)
    assert D.same(logit, want) and D.same(pred, D.sigmoid(want))
    clf.close()


def _tier_sizes():
    """(dim, n1, n2): rows at the staging limit of a small net and one column above it; layers at the hidden-unit block (16), one above,
    at what four slots take in one pass (64), one above, and at the largest supported size; the longest rows the issue names"""
    from glia_amd import hmt
    lim = hmt.mlp_limits(10, 10)
    ub, slots, big = lim["unit_block"], lim["slots"], lim["max_hidden"]
    out = [(lim["stage_max_dim"], 10, 10), (lim["stage_max_dim"] + 1, 10, 10)]
    lim0 = hmt.mlp_limits(0, 0)["stage_max_dim"]
    out += [(lim0, 0, 0), (lim0 + 1, 0, 0)]
    for n in (ub, ub + 1, ub * slots, ub * slots + 1, big):
        out += [(7, n, n)]
    out += [(7, big, 1), (7, 1, big), (33, ub + 1, ub * slots + 1), (4096, 3, 5), (4096, 0, 0)]
    return out


def test_tier_queries():
    from glia_amd import hmt
    lim = hmt.mlp_limits(10, 10)
    assert (lim["unit_block"], lim["slots"]) == (16, 4) and lim["max_hidden"] >= 256 and lim["max_dim"] >= 4096
    assert hmt.mlp_tile_rows(lim["stage_max_dim"], 10, 10)[1] and not hmt.mlp_tile_rows(lim["stage_max_dim"] + 1, 10, 10)[1]
    tiles = {hmt.mlp_tile_rows(d, a, b) for d, a, b in _tier_sizes()}
    assert {t[0] for t in tiles} == {64, 32, 16, 8} and {t[1] for t in tiles} == {True, False}, tiles


@pytest.mark.parametrize("i", range(14))
def test_tiers(ctx, i):
    sizes = _tier_sizes()
    assert len(sizes) == 14
    dim, n1, n2 = sizes[i]
    n_rows = 130 if dim < 1000 else 67
    w, rows, mn, mx, ref = _case(dim, n1, n2, n_rows=n_rows)
    for rescale in (False, True):
        clf = _model(ctx, w, n1, n2, *((mn, mx) if rescale else (None, None)))
        want = ref[rescale][0]
        assert D.same(_device_logits(clf, rows)[1], want), (dim, n1, n2, rescale)
        assert D.same(_device_logits(clf, rows[:65], stride=dim + 3)[1], want[:65])
        assert D.same(clf.predict(rows[:33], want_logits=True)[1], want[:33])
        clf.close()


@pytest.mark.parametrize("dim,n1,n2", [(7, 3, 17), (104, 10, 10), (33, 64, 33), (104, 0, 0)])
def test_padded_stride(ctx, dim, n1, n2):
    w, rows, mn, mx, ref = _case(dim, n1, n2)
    clf = _model(ctx, w, n1, n2, mn, mx)
    for n, stride in ((1, dim + 1), (65, dim + 1), (257, dim + 8), (N_ROWS, 2 * dim + 5)):
        assert D.same(_device_logits(clf, rows[:n], stride=stride)[1], ref[True][0][:n]), (n, stride)       # NaN in the padding: never read
    clf.close()


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("dim,n1,n2", [(7, 3, 17), (104, 10, 10), (33, 64, 33), (104, 0, 0)])
def test_ensemble(ctx, dim, n1, n2, rescale):
    from glia_amd import hmt
    ws, rows, mn, mx, ref = _case(dim, n1, n2, n_models=3)
    want, picks = ref[rescale]
    counts = np.bincount(picks, minlength=3)
    assert counts.min() >= 50, counts                                       # all three models are reached
    assert len(set(picks[:64].tolist())) == 3                               # ... within one wave
    clf = _model(ctx, ws, n1, n2, *((mn, mx) if rescale else (None, None)), dist=D.DIST)
    for n in (1, 65, N_ROWS):
        assert D.same(_device_logits(clf, rows[:n])[1], want[:n]), n
    pred, logit = clf.predict(rows, want_logits=True)
    assert D.same(logit, want) and D.same(pred, D.sigmoid(want))
    clf.close()
    # the pick reads the rescaled, bias-appended vector: index dim is the appended 1.0
    for thr, model in ((1.5, 0), (0.5, None)):
        clf = _model(ctx, ws, n1, n2, *((mn, mx) if rescale else (None, None)), dist=(0, dim, thr))
        w1 = D.logits(ws, n1, n2, rows[:130], *((mn, mx) if rescale else (None, None)), dist=(0, dim, thr))
        assert D.same(_device_logits(clf, rows[:130])[1], w1)
        if model is not None:
            assert D.same(w1, D.logits(ws[model], n1, n2, rows[:130], *((mn, mx) if rescale else (None, None))))
        clf.close()
    for bad in ((dim + 1, 0, 0.0), (0, dim + 1, 0.0), (-1, 0, 0.0)):
        with pytest.raises(hmt.HmtError) as e:
            _model(ctx, ws, n1, n2, dist=bad)
        assert e.value.code == hmt.ERR_ARG and "distributor" in str(e.value)


def test_special_rows(ctx):
    for name, w, n1, n2, rows in D.special_cases():
        want = D.logits(w, n1, n2, rows)
        clf = _model(ctx, w, n1, n2)
        pred_d, logit_d = _device_logits(clf, rows)
        assert D.same(logit_d, want), name
        assert (pred_d[np.isposinf(want)] == 1.0).all() and (pred_d[np.isneginf(want)] == 0.0).all() and np.isnan(pred_d[np.isnan(want)]).all()
        pred, logit = clf.predict(rows, want_logits=True)
        assert D.same(logit, want) and D.same(pred, D.sigmoid(want)), name
        clf.close()
    w, rows, mn, mx = D.random_case(7, 3, 17, n_rows=70)
    rows = rows.copy()
    rows[3, 0], rows[4, 1], rows[5, 2], rows[6, 3], rows[69, 6] = np.nan, np.inf, -np.inf, -0.0, np.nan
    for mm in ((None, None), (mn, mx)):
        clf = _model(ctx, w, 3, 17, *mm)
        assert D.same(_device_logits(clf, rows)[1], D.logits(w, 3, 17, rows, *mm))
        clf.close()


@pytest.mark.parametrize("dim,n1,n2,n_models", [(104, 10, 10, 1), (7, 3, 17, 3), (33, 64, 33, 1), (7, 65, 65, 1), (7, 256, 256, 1), (104, 0, 0, 1), (300, 10, 10, 1)])
def test_small_chunks_and_launches(ctx, dim, n1, n2, n_models):
    """GLIA_HMT_MINCAP: the host entry streams 256 rows at a time -- three full chunks and a remainder of 232 -- and a launch takes 3
    tiles (of 64, 32 or 8 rows here), so every later chunk and launch starts at an offset into rows, logits and predictions"""
    from glia_amd import hmt
    w, rows, mn, mx, ref = _case(dim, n1, n2, n_models=n_models)
    want = ref[True][0]
    clf = _model(ctx, w, n1, n2, mn, mx, dist=D.DIST if n_models == 3 else None)
    with hmt.options(GLIA_HMT_MINCAP=1):
        pred, logit = clf.predict(rows, want_logits=True)
        pred_d, logit_d = _device_logits(clf, rows)
        _, logit_s = _device_logits(clf, rows[:777], stride=dim + 5)
    assert D.same(logit, want) and D.same(pred, D.sigmoid(want))
    assert D.same(logit_d, want) and D.same(logit_s, want[:777])
    assert int(_ulps(pred_d, pred).max()) <= DEVICE_SIGMOID_ULPS
    clf.close()


def test_second_launch(ctx):
    """More rows than one launch takes (2^23 tiles of 64 rows): a logsig model of one column at 2^29 + 65 rows, 4.3 GB of rows.  The
    rows on both sides of the launch boundary and the tail are compared bit for bit, logits and predictions of the second launch land
    at their offsets."""
    import torch
    from glia_amd import hmt
    assert hmt.mlp_tile_rows(1, 0, 0) == (64, True)
    edge = (1 << 23) * 64
    n = edge + 65
    w = np.array([0.75, -0.125])
    clf = _model(ctx, w, 0, 0)
    g = torch.Generator(device="cuda").manual_seed(3)
    rows = torch.rand((n, 1), dtype=torch.float64, device="cuda", generator=g)
    rows.mul_(8.0).sub_(4.0)
    pred, logit = clf.predict(rows, want_logits=True)
    for a, b in ((0, 130), (edge - 130, n)):
        x = rows[a:b].cpu().numpy()
        want = D.logits(w, 0, 0, x)
        assert len(np.unique(want)) > 100
        assert D.same(logit[a:b].cpu().numpy(), want), (a, b)
        assert int(_ulps(pred[a:b].cpu().numpy(), D.sigmoid(want)).max()) <= DEVICE_SIGMOID_ULPS
    # every row was written: a logit is 0.75 x - 0.125 with x in [-4, 4), a prediction lies in (0, 1)
    assert float(logit.min()) >= -3.125 and float(logit.max()) < 2.875 and float(pred.min()) > 0.0 and float(pred.max()) < 1.0
    clf.close()
    del rows, pred, logit
    torch.cuda.empty_cache()


def _ulps(a, b):
    """distance in representable doubles between finite values of one sign"""
    return np.abs(a.view(np.int64) - b.view(np.int64))


def test_device_sigmoid(ctx):
    """d_pred against 1 / (1 + math.exp(-h3)) evaluated on the device's own logits: a logsig model of one column with weights (1, 0)
    hands the column through (0.0 + x * 1.0 + 1.0 * 0.0), so the sweep is the logits"""
    rng = np.random.default_rng(11)
    x = np.concatenate([np.linspace(-750.0, 750.0, 30001), rng.uniform(-750.0, 750.0, 20000), rng.uniform(-40.0, 40.0, 20000),
                        rng.standard_normal(5000) * 1e-3, [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-320, -1e-320, 709.9, -709.9, 745.2, -745.2]])
    clf = _model(ctx, np.array([1.0, 0.0]), 0, 0)
    pred, logit = _device_logits(clf, x[:, None])
    clf.close()
    assert D.same(logit, np.where(x == 0.0, 0.0, x))                 # (a chain starts at +0.0: the logit of -0.0 is +0.0)
    want = D.sigmoid(logit)
    nan = np.isnan(logit)
    assert nan.sum() == 1 and np.isnan(pred[nan]).all() and not np.isnan(pred[~nan]).any()
    assert (pred[np.isposinf(logit)] == 1.0).all() and (pred[np.isneginf(logit)] == 0.0).all()
    assert (pred[~nan] >= 0.0).all() and (pred[~nan] <= 1.0).all()
    d = _ulps(pred[~nan], want[~nan])
    worst = int(d.max())
    print("device sigmoid: largest distance %d ulps at logit %r (%d of %d values differ)" % (worst, float(logit[~nan][d.argmax()]), int((d > 0).sum()), d.size))
    assert worst <= DEVICE_SIGMOID_ULPS


def test_statuses(ctx):
    import ctypes as C
    import torch
    from glia_amd import hmt
    w, rows, mn, mx, ref = _case(104, 10, 10)
    clf = _model(ctx, w, 10, 10, mn, mx)
    a = _device_logits(clf, rows)
    b = _device_logits(clf, rows)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()            # two calls: identical bytes
    p1, l1 = clf.predict(rows, want_logits=True)
    p2, l2 = clf.predict(rows, want_logits=True)
    assert p1.tobytes() == p2.tobytes() and l1.tobytes() == l2.tobytes()
    assert clf.predict(rows[:0]).shape == (0,)                                               # no rows: OK
    assert tuple(clf.predict(torch.empty((0, 104), dtype=torch.float64, device="cuda")).shape) == (0,)
    for bad in (rows[:, :103], np.concatenate([rows, rows[:, :1]], axis=1)):
        with pytest.raises(hmt.HmtError) as e:
            clf.predict(np.ascontiguousarray(bad))
        assert e.value.code == hmt.ERR_ARG and "columns" in str(e.value)
        with pytest.raises(hmt.HmtError) as e:
            clf.predict(torch.from_numpy(np.ascontiguousarray(bad)).cuda())
        assert e.value.code == hmt.ERR_ARG
    # only one of the two outputs
    d = torch.from_numpy(np.array(rows)).cuda()
    only = torch.full((N_ROWS,), 7.0, dtype=torch.float64, device="cuda")
    hmt._check(hmt.lib().glia_hmt_mlp_predict_device(ctx.h, clf.h, C.c_void_p(d.data_ptr()), C.c_int64(N_ROWS), C.c_int(104), C.c_int64(104), None,
                                                     C.c_void_p(only.data_ptr())))
    ctx.sync()
    assert D.same(only.cpu().numpy(), ref[True][0])
    assert hmt.lib().glia_hmt_mlp_predict_device(ctx.h, clf.h, C.c_void_p(d.data_ptr()), C.c_int64(N_ROWS), C.c_int(104), C.c_int64(104), None, None) == hmt.ERR_ARG
    clf.close()
    # beyond the limits: GLIA_HMT_ERR_UNSUPPORTED with a message
    lim = hmt.mlp_limits(10, 10)
    for n1, n2 in ((lim["max_hidden"] + 1, 1), (1, lim["max_hidden"] + 1)):
        with pytest.raises(hmt.HmtError) as e:
            _model(ctx, np.zeros(D.n_weights(3, n1, n2)), n1, n2)
        assert e.value.code == -3 and "not supported" in str(e.value)
    with pytest.raises(hmt.HmtError) as e:
        _model(ctx, np.zeros(lim["max_dim"] + 2), 0, 0)
    assert e.value.code == -3 and "columns" in str(e.value)
    # a host-only model has no device side
    host_only = _model(None, w, 10, 10)
    with pytest.raises(hmt.HmtError) as e:
        hmt._check(hmt.lib().glia_hmt_mlp_predict(ctx.h, host_only.h, hmt._np(np.array(rows)), C.c_int64(4), C.c_int(104), hmt._np(np.empty(4)), None))
    assert e.value.code == hmt.ERR_ARG
    host_only.close()


def test_tensor_route_equals_numpy_route(ctx):
    import torch
    from glia_amd import hmt
    w, rows, mn, mx, ref = _case(104, 17, 3)
    clf = _model(ctx, w, 17, 3, mn, mx)
    buf = torch.full((N_ROWS, 120), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, 5:109] = torch.from_numpy(np.array(rows)).cuda()
    view = buf[:, 5:109]                                                     # a padded stride and an offset start
    assert view.stride(0) == 120
    pred_t, logit_t = clf.predict(view, want_logits=True)
    pred_n, logit_n = clf.predict(rows, want_logits=True)
    assert D.same(logit_t.cpu().numpy(), logit_n) and D.same(logit_n, ref[True][0])
    assert int(_ulps(pred_t.cpu().numpy(), pred_n).max()) <= DEVICE_SIGMOID_ULPS
    assert isinstance(clf.predict(view), torch.Tensor) and isinstance(clf.predict(rows), np.ndarray)
    clf.close()
    # the logsig wrapper
    import os
    import tempfile
    wl, rl, _, _, refl = _case(104, 0, 0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "logsig.txt")
        D.write_values(path, wl)
        lg = hmt.Logsig(ctx, path)
    assert D.same(lg.predict(rl, want_logits=True)[1], refl[False][0])
    assert D.same(lg.predict(torch.from_numpy(np.array(rl)).cuda(), want_logits=True)[1].cpu().numpy(), refl[False][0])
    lg.close()
