"""The MLP / logsig predictors without a GPU: the exports, the second author (_mlpdef) against its own triple loop and against the
oracle's rescale and pick_model, glia_hmt_mlp_predict_host (glia_amd/csrc/mlp_model.hpp) against _mlpdef bit for bit, the parser's
refusals, and cli/mlp_model_check."""
import os
import subprocess

import numpy as np
import pytest

import _mlpdef as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hmt():
    from glia_amd import hmt
    return hmt


def test_exports():
    hmt = _hmt()
    L = hmt.lib()
    for name in ("glia_hmt_mlp_file_parse", "glia_hmt_mlp_create", "glia_hmt_mlp_load", "glia_hmt_mlp_dim", "glia_hmt_mlp_free",
                 "glia_hmt_mlp_predict_host", "glia_hmt_mlp_predict_device", "glia_hmt_mlp_predict", "glia_hmt_mlp_limits",
                 "glia_hmt_mlp_predict_tile_rows"):
        assert hasattr(L, name), name
    for name in ("MLP", "Logsig", "mlp_predict_host", "mlp_limits", "mlp_tile_rows", "mlp_file_parse"):
        assert hasattr(hmt, name), name
    lim = hmt.mlp_limits(10, 10)
    assert lim["unit_block"] == 16 and lim["slots"] == 4 and lim["max_hidden"] >= 256 and lim["max_dim"] >= 4096
    assert 104 <= lim["stage_max_dim"] < 4096
    assert hmt.mlp_tile_rows(lim["stage_max_dim"], 10, 10)[1] and not hmt.mlp_tile_rows(lim["stage_max_dim"] + 1, 10, 10)[1]
    assert hmt.mlp_tile_rows(104, 10, 10) == (64, True)
    assert hmt.mlp_limits(256, 256)["stage_max_dim"] == 0 and hmt.mlp_tile_rows(104, 256, 256) == (8, False)


@pytest.mark.parametrize("dim,n1,n2", D.SIZES)
@pytest.mark.parametrize("rescale", [False, True])
def test_numpy_form_is_the_triple_loop(dim, n1, n2, rescale):
    w, rows, mn, mx = D.random_case(dim, n1, n2, n_rows=6)
    mm = (mn, mx) if rescale else (None, None)
    assert D.same(D.logits(w, n1, n2, rows, *mm), D.triple_loop(w, n1, n2, rows, *mm))
    if dim >= 4:
        ws, rows, mn, mx = D.random_case(dim, n1, n2, n_rows=12, n_models=3)
        got, m = D.logits(ws, n1, n2, rows, *mm, dist=D.DIST, want_pick=True)
        assert len(set(m.tolist())) >= 2
        assert D.same(got, D.triple_loop(ws, n1, n2, rows, *mm, dist=D.DIST))


def test_special_rows_reach_what_they_are_for():
    for name, w, n1, n2, rows in D.special_cases():
        lg = D.logits(w, n1, n2, rows)
        assert D.same(lg, D.triple_loop(w, n1, n2, rows)), name
        p = D.sigmoid(lg)
        if name != "mlp_b":
            assert np.isposinf(lg).any() and np.isneginf(lg).any(), name
            assert (p[np.isposinf(lg)] == 1.0).all() and (p[np.isneginf(lg)] == 0.0).all()
        if name != "mlp_a":
            assert np.isnan(lg).any() and np.isnan(p[np.isnan(lg)]).all(), name
    # hidden sums of exactly 0.0 in the first layer of the crafted model: x0 - x1 for (3, 3), and the -0.0 products of (-0.0, 0.0)
    _, w, n1, n2, rows = D.special_cases()[0]
    h1 = D._dense(D.prepare(rows), D.split(w, 2, n1, n2)[0])
    assert D.same(h1[0, 0], 0.0) and D.same(h1[1, 0], 0.0) and D.same(h1[2, 1], 0.0)


def test_rescale_is_the_oracles():
    from oracle import pyoracle as O
    rng = np.random.default_rng(5)
    dim = 23
    mn = -1.0 - rng.random(dim)
    mx = 1.0 + rng.random(dim)
    mx[::4] = mn[::4]                                   # max == min: the denominator is FEPS
    rows = rng.standard_normal((40, dim)) * 1.5         # inside and outside the bounds
    rows[0] = mn
    rows[1] = mx
    rows[2] = mn - 1.0
    rows[3] = mx + 1.0
    rows[4, :3] = [np.inf, -np.inf, -0.0]
    assert (rows < mn).any() and (rows > mx).any()
    got = D.rescale(rows, mn, mx)
    ref = O.rescale(rows.ravel(), np.tile(mn, rows.shape[0]), np.tile(mx, rows.shape[0])).reshape(rows.shape)
    assert D.same(got, ref)
    keep = np.ones(dim, bool)
    keep[::4] = False
    assert (got[0, keep] == -1.0).all() and (np.abs(got[1, keep] - 1.0) < 1e-15).all() and (got[0, ~keep] == -1.0).all()


def test_pick_is_the_oracles():
    from oracle import pyoracle as O
    rng = np.random.default_rng(6)
    x = rng.standard_normal((200, 9))
    x[0, 1] = np.nan
    x[1, 3] = np.nan
    x[2, 1] = 0.25
    x[3, 3] = 0.25
    for dist in ((3, 1, 0.25), (0, 8, -0.5), (8, 8, 0.0), (2, 2, 100.0)):
        got = D.pick(x, dist)
        ref = np.array([O.pick_model(dist[0], dist[1], dist[2], r) for r in x])
        assert (got == ref).all()
    assert sorted(set(D.pick(x, (3, 1, 0.25)).tolist())) == [0, 1, 2]


@pytest.mark.parametrize("dim,n1,n2", D.SIZES)
@pytest.mark.parametrize("rescale", [False, True])
def test_predict_host_is_the_definition(dim, n1, n2, rescale):
    hmt = _hmt()
    w, rows, mn, mx = D.random_case(dim, n1, n2)
    assert rows.shape[0] == 257
    mm = (mn, mx) if rescale else (None, None)
    pred, logit = hmt.mlp_predict_host(w, n1, n2, rows, *mm)
    ref = D.logits(w, n1, n2, rows, *mm)
    assert D.same(logit, ref) and D.same(pred, D.sigmoid(ref))
    assert np.isfinite(ref).all() and (dim < 7 or len(np.unique(ref)) > 100)      # not degenerate (a net of one unit per layer may be dead)


@pytest.mark.parametrize("dim,n1,n2", [(7, 3, 17), (104, 10, 10), (104, 0, 0)])
@pytest.mark.parametrize("rescale", [False, True])
def test_predict_host_ensemble(dim, n1, n2, rescale):
    hmt = _hmt()
    ws, rows, mn, mx = D.random_case(dim, n1, n2, n_models=3)
    mm = (mn, mx) if rescale else (None, None)
    ref, m = D.logits(ws, n1, n2, rows, *mm, dist=D.DIST, want_pick=True)
    assert min(np.bincount(m, minlength=3)) >= 10, np.bincount(m, minlength=3)        # all three models are reached
    pred, logit = hmt.mlp_predict_host(ws, n1, n2, rows, *mm, distributor_args=D.DIST)
    assert D.same(logit, ref) and D.same(pred, D.sigmoid(ref))
    # the pick sees the rescaled, bias-appended vector: index dim is the appended 1.0
    ref1 = D.logits(ws, n1, n2, rows, *mm, dist=(0, dim, 1.5))
    assert D.same(hmt.mlp_predict_host(ws, n1, n2, rows, *mm, distributor_args=(0, dim, 1.5))[1], ref1)
    assert D.same(ref1, D.logits(ws[0], n1, n2, rows, *mm))                           # 1.0 < 1.5: always model 0


def test_predict_host_special_rows():
    hmt = _hmt()
    for name, w, n1, n2, rows in D.special_cases():
        ref = D.logits(w, n1, n2, rows)
        pred, logit = hmt.mlp_predict_host(w, n1, n2, rows)
        assert D.same(logit, ref) and D.same(pred, D.sigmoid(ref)), name
    # special values through the rescale as well
    w, rows, mn, mx = D.random_case(7, 3, 17, n_rows=20)
    rows = rows.copy()
    rows[3, 0], rows[4, 1], rows[5, 2], rows[6, 3] = np.nan, np.inf, -np.inf, -0.0
    ref = D.logits(w, 3, 17, rows, mn, mx)
    pred, logit = hmt.mlp_predict_host(w, 3, 17, rows, mn, mx)
    assert D.same(logit, ref) and D.same(pred, D.sigmoid(ref))


def test_files_and_refusals(tmp_path):
    hmt = _hmt()
    w, rows, mn, mx = D.random_case(7, 3, 17, n_rows=9)
    model = str(tmp_path / "model.txt")
    D.write_values(model, w)
    assert D.same(hmt.mlp_file_parse(model), w)
    mm = str(tmp_path / "minmax.txt")
    D.write_rows(mm, [np.concatenate([mn, [5.0, 6.0]]), np.concatenate([mx, [7.0]])])      # extra entries are ignored
    m = hmt.MLP(None, model, 3, 17, minmax=mm)
    assert m.dim == 7
    assert D.same(m.predict_host(rows, want_logits=True)[1], D.logits(w, 3, 17, rows, mn, mx))
    with pytest.raises(hmt.HmtError) as e:                                                  # a wrong dim
        m.predict_host(rows[:, :6])
    assert e.value.code == hmt.ERR_ARG and "columns" in str(e.value)
    assert m.predict_host(rows[:0]).shape == (0,)                                           # no rows: OK
    with pytest.raises(hmt.HmtError) as e:                                                  # a host-only model has no device side
        m.predict(rows)
    assert e.value.code == hmt.ERR_ARG and "predict_host" in str(e.value)
    m.close()
    lg = hmt.Logsig(None, model)                                                            # any file of >= 2 values is a logsig model
    assert lg.dim == w.size - 1
    lg.close()

    def refused(code, text, *a, **kw):
        with pytest.raises(hmt.HmtError) as e:
            hmt.MLP(None, *a, **kw)
        assert e.value.code == code and text in str(e.value), str(e.value)

    rem = str(tmp_path / "remainder.txt")
    D.write_values(rem, np.concatenate([w, [1.0]]))
    refused(hmt.ERR_ARG, "do not fit", rem, 3, 17)                                          # the reference truncates silently
    small = str(tmp_path / "small.txt")
    D.write_values(small, np.ones(D.n_weights(0, 3, 2)))
    refused(hmt.ERR_ARG, "D < 2", small, 3, 2)
    empty = str(tmp_path / "empty.txt")
    open(empty, "w").close()
    refused(-6, "no weights", empty, 3, 17)
    blank = str(tmp_path / "blank.txt")
    with open(blank, "w") as f:
        f.write(" \n\n\t \n")
    refused(-6, "no weights", blank, 3, 17)
    refused(-6, "cannot open", str(tmp_path / "missing.txt"), 3, 17)
    short = str(tmp_path / "short.txt")
    D.write_rows(short, [mn[:6], mx])
    refused(hmt.ERR_ARG, "min/max", model, 3, 17, minmax=short)
    one = str(tmp_path / "one.txt")
    D.write_rows(one, [mn])
    refused(-6, "two rows", model, 3, 17, minmax=one)
    refused(hmt.ERR_ARG, "both", model, 3, 0)
    refused(-3, "not supported", model, 257, 1)                                             # GLIA_HMT_ERR_UNSUPPORTED
    refused(hmt.ERR_ARG, "distributor", [model] * 3, 3, 17)
    refused(hmt.ERR_ARG, "distributor", [model] * 3, 3, 17, distributor_args=(8, 0, 0.0))   # indices lie in [0, dim]
    refused(hmt.ERR_ARG, "distributor", [model] * 3, 3, 17, distributor_args=(0, -1, 0.0))
    hmt.MLP(None, [model] * 3, 3, 17, distributor_args=(7, 0, 0.0)).close()
    refused(hmt.ERR_ARG, "three models", [model] * 2, 3, 17, distributor_args=(0, 1, 0.0))
    # trailing blanks and a missing final newline change nothing
    tail = str(tmp_path / "tail.txt")
    with open(tail, "w") as f:
        f.write("  ".join("%.17g" % v for v in w) + "   \n\n  ")
    assert D.same(hmt.mlp_file_parse(tail), w)


def test_mlp_model_check_builds_and_passes():
    cli = os.path.join(ROOT, "cli")
    subprocess.check_call(["make", "-C", cli, "mlp_model_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(cli, "mlp_model_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
