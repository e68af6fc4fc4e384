"""The MLP / logsig trainer on the host (glia_hmt_mlp_train_host: glia_amd/csrc/mlp_backward.hpp, the definition of DESIGN 3.14) against
the second author tests/_mlptraindef.py: weights after every round, trace and sigmas bit for bit on every shared case; properties of the
step rules read from the trace; refusals; limits; the second author's gradient against a central difference of its own energy; a toy
set.  No GPU."""
import math

import numpy as np
import pytest

import _mlpdef
import _mlptrain_cases as K
import _mlptraindef as T


def _hmt():
    from glia_amd import hmt
    return hmt


def _train(kw, **more):
    o = dict(kw["opts"])
    o.update(more)
    return _hmt().train_mlp_host(kw["rows"], kw["labels"], kw["n1"], kw["n2"], kw["minmax"], kw["init"], **o)


def _kw(name):
    return K.CASES[K.IDS.index(name)][1]


@pytest.mark.parametrize("name", K.IDS)
def test_host_equals_second_author(name):
    m = _train(_kw(name))
    K.assert_same_as_reference(m, K.reference(name))
    m.close()


def test_cases_reach_what_they_are_for():
    """read from the second author's results: the properties the cases were chosen for"""
    for opt in (1, 2, 3):
        tr = K.reference("adaptive_big_lr_opt%d" % opt)["trace"]
        assert tr[0][5:8] == (0, 0, 0) and tr[0][8] >= 2, "the first iteration rolls back at least twice"
        fixed = K.reference("fixed_lrdi2_opt%d" % opt)["trace"]
        steps = [r[3] for r in fixed if r[5] == 0]
        assert steps == [0.05, 0.05, 0.025, 0.025, 0.0125, 0.0125]          # t = 0 .. 4, then the final statistics
    r = K.reference("uss_floor")
    assert r["sigma2"] == [10.0] * 3 and all(0.0 < v < 10.0 for v in r["sigma2_eval"])
    r = K.reference("uss")
    assert len(set(r["sigma2"])) == 3 and r["sigma2"] == r["sigma2_eval"]
    r = K.reference("lrds")
    assert [x[3] for x in r["trace"] if x[6] == 0] == [0.05, 0.025, 0.0125]
    kw = _kw("label0_interleaved")
    X, t = T.prepare(kw["rows"], kw["labels"])
    assert len(t) == int(np.isin(kw["labels"], (1, -1)).sum()) < len(kw["labels"]) - 40
    assert set(T.prepare(_kw("one_class")["rows"], _kw("one_class")["labels"])[1].tolist()) == {0.05}
    # every e_i exactly 0: L exactly 0, the gradient exactly wr * w = 0, so the first evaluation ends the round
    r = K.reference("logsig_e_zero")
    kw = _kw("logsig_e_zero")
    X, t = T.prepare(kw["rows"], kw["labels"], None, None, 0.5, 0.5)
    L, g = T.loss_grad(np.zeros(8), 0, 0, X, t)
    assert L == 0.0 and not g.any()
    assert [x[2] for x in r["trace"]] == [0.0] * 4 and r["sigma2_eval"] == [0.0] * 3
    assert r["trace"][0][0] == 129 * math.log(0.25) / 2.0
    # dead units: hidden sums of exactly 0.0 on the zero rows
    kw = _kw("zero_row_dead_units")
    X, _ = T.prepare(kw["rows"], kw["labels"])
    W0, W1, _ = _mlpdef.split(kw["init"], 7, 3, 17)
    h1 = _mlpdef._dense(X, W0)
    assert not h1[3].any() and not h1[64].any() and not _mlpdef._dense(_mlpdef._relu1(h1), W1)[3].any()
    _, G = T.row_gradients(kw["init"], 3, 17, X)
    assert not G[3, :-1].any() and G[3, -1] != 0.0 and G[0, :24].any()           # only the output bias sees the zero row
    # the sigmoid saturates to exactly 0 and 1
    kw = _kw("logsig_saturated")
    X, _ = T.prepare(kw["rows"], kw["labels"])
    f = T.forward(kw["init"], 0, 0, X)
    assert (f == 0.0).any() and (f == 1.0).any()
    for name in ("divergent_fixed", "divergent_adaptive"):
        r = K.reference(name)
        assert r["stopped_nonfinite"] and r["trace"][-1][7] == 2 and len(r["round_w"]) == 1
        assert _mlpdef.same(r["round_w"][0], T.init_weights(0, r["round_w"][0].size)), "the weights from before the step are restored"


def test_literal_loops_agree_with_the_numpy_form():
    for name in ("shape_n65_d7_3_17", "shape_n129_d104_0_0", "zero_row_dead_units", "label0_interleaved"):
        kw = _kw(name)
        X, t = T.prepare(kw["rows"], kw["labels"])
        w = kw["init"] if kw["init"] is not None else T.init_weights(3, _mlpdef.n_weights(X.shape[1] - 1, kw["n1"], kw["n2"])) * 20.0
        ps = sorted(set([0, 1, X.shape[1] - 1, X.shape[1], w.size // 2, w.size - 2, w.size - 1]) & set(range(w.size)))
        L, g = T.loss_grad(w, kw["n1"], kw["n2"], X, t)
        L2, g2 = T.literal_grad(w, kw["n1"], kw["n2"], X, t, ps)
        assert _mlpdef.same(L, L2) and _mlpdef.same(g[ps], g2), name
    assert _mlpdef.same(_hmt().mlp_init_weights(5, 40), T.init_weights(5, 40))
    w = T.init_weights(0, 20000)
    assert abs(w.mean()) < 3e-4 and abs(w.std() - 0.01) < 3e-4 and np.abs(w).max() <= 0.06


def test_adaptive_step_never_accepts_a_higher_energy():
    """a property of the rule: with the adaptive step every accepted iteration's fx is below the one before"""
    hmt = _hmt()
    seen = 0
    for name, kw in K.CASES:
        if T._isfeq(kw["opts"].get("step_decay", 1.0), 1.0) or name.startswith("divergent"):
            continue
        m = _train(kw)
        tr = m.trace
        assert (tr["step"] > T.MIN_STEP).all()
        for rnd in range(m.rounds):
            fx = tr["fx"][(tr["round"] == rnd) & (tr["kind"] <= 1)]          # iterations, then the final statistics (fx after the last step)
            assert (np.diff(fx) < 0.0).all(), (name, rnd, fx)
            seen += len(fx) - 1
        m.close()
    assert seen > 40


def test_limits_and_defaults():
    hmt = _hmt()
    lim = hmt.mlp_train_limits()
    assert lim == dict(chunk_rows=T.CHUNK, max_hidden=32, max_dim=384)
    assert lim["max_hidden"] == hmt.mlp_loop_limits()["max_hidden"]
    o = hmt.MLPTrainOpts()
    import ctypes
    hmt.lib().glia_hmt_mlp_train_opts_default(ctypes.byref(o))
    for k, v in T.DEFAULTS.items():
        assert getattr(o, k) == v, k
    assert (o.n1, o.n2, o.wu, o.update_sigma_u, o.sup_batch_size, o.uns_batch_size, o.balance_sup_batch, o.alt_su) == (10, 10, 0.0, 0, -1, -1, 0, 0)
    # the limits themselves are taken
    rng = np.random.default_rng(1)
    m = hmt.train_mlp_host(rng.standard_normal((3, 384)), [1, -1, 1], 32, 32, ws=1.0, sigma_s=1.0, step=0.1, max_iterations=1, n_sigma_updates=1)
    assert m.n_weights == 385 * 32 + 33 * 32 + 33 and m.rounds == 1 and m.n_used_rows == 3
    m.close()


ARG, UNSUPPORTED = -1, -3
OK = dict(ws=1.0, sigma_s=1.0, step=0.1, max_iterations=1, n_sigma_updates=1)


@pytest.mark.parametrize("n1,n2,opts,code,words", [
    (3, 3, dict(OK, ws=0.0, wr=0.0), ARG, ["wr and ws are both 0"]),
    (3, 3, dict(OK, sigma_s=0.0), ARG, ["sigma_s is 0", "update_sigma_s"]),
    (0, 3, OK, ARG, ["both 0", "logsig"]),
    (3, 0, OK, ARG, ["both 0", "logsig"]),
    (3, 3, dict(OK, optimizer=4), ARG, ["unsupported optimizer type"]),
    (3, 3, dict(OK, max_iterations=-1), ARG, ["max_iterations"]),
    (3, 3, dict(OK, step=math.nan), ARG, ["not finite"]),
    (3, 3, dict(OK, wu=0.5), UNSUPPORTED, ["wu", "unsupervised"]),
    (3, 3, dict(OK, update_sigma_u=1), UNSUPPORTED, ["update_sigma_u", "--usu"]),
    (3, 3, dict(OK, sup_batch_size=16), UNSUPPORTED, ["sup_batch_size", "--bss"]),
    (3, 3, dict(OK, uns_batch_size=16), UNSUPPORTED, ["uns_batch_size", "--bsu"]),
    (3, 3, dict(OK, balance_sup_batch=1), UNSUPPORTED, ["balance_sup_batch", "--bb"]),
    (3, 3, dict(OK, alt_su=1), UNSUPPORTED, ["alt_su"]),
    (33, 3, OK, UNSUPPORTED, ["more than 32 units"]),
    (3, 33, OK, UNSUPPORTED, ["more than 32 units"]),
])
def test_option_errors_and_refusals(n1, n2, opts, code, words):
    hmt = _hmt()
    rows = np.arange(12.0).reshape(4, 3)
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_mlp_host(rows, [1, -1, 1, -1], n1, n2, **opts)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_argument_errors():
    hmt = _hmt()
    rows = np.arange(12.0).reshape(4, 3)
    lab = [1, -1, 1, -1]

    def refused(code, word, *a, **k):
        with pytest.raises(hmt.HmtError) as e:
            hmt.train_mlp_host(*a, **dict(OK, **k))
        assert e.value.code == code and word in str(e.value), str(e.value)

    bad = rows.copy()
    bad[2, 1] = np.nan
    refused(ARG, "row 2", bad, lab, 3, 3)
    refused(ARG, "no row is labelled", rows, [0, 2, 3, 0], 3, 3)
    w = np.zeros(_mlpdef.n_weights(3, 3, 3))
    w[4] = np.inf
    refused(ARG, "initial weight 4", rows, lab, 3, 3, None, w)
    refused(ARG, "do not fit", rows, lab, 3, 3, None, np.zeros(5))
    refused(ARG, "min/max", rows, lab, 3, 3, (np.zeros(3), np.array([1.0, np.inf, 1.0])))
    refused(ARG, "fewer min/max", rows, lab, 3, 3, (np.zeros(2), np.ones(2)))
    refused(UNSUPPORTED, "more than 384 columns", np.zeros((2, 385)), [1, -1], 3, 3)
    m = hmt.train_mlp_host(rows, lab, 3, 3, **OK)
    for call in (lambda: m.weights(1), lambda: m.weights(-2), lambda: m.mlp(None, 5)):
        with pytest.raises(hmt.HmtError) as e:
            call()
        assert e.value.code == ARG and "rounds 0 to 0" in str(e.value)
    m.close()


def test_rows_minmax_and_the_classifier_of_a_model():
    hmt = _hmt()
    rng = np.random.default_rng(8)
    a, b = rng.standard_normal((5, 4)), rng.standard_normal((9, 4)) - 3.0
    a[:, 2] = -np.abs(a[:, 2]); b[:, 2] = -np.abs(b[:, 2])            # a column without a positive value: the maximum stays at DBL_MIN
    mn, mx = hmt.rows_minmax([a, b])
    both = np.concatenate([a, b])
    assert _mlpdef.same(mn, both.min(0)) and _mlpdef.same(mx[[0, 1, 3]], both.max(0)[[0, 1, 3]]) and mx[2] == 2.2250738585072014e-308
    lab = np.where(both[:, 0] > -1.5, 1, -1)
    m = hmt.train_mlp_host(both, lab, 4, 5, (mn, mx), ws=1.0, sigma_s=0.5, step=0.5, optimizer=2, max_iterations=5, n_sigma_updates=2)
    ref = T.train(both, lab, 4, 5, (mn, mx), ws=1.0, sigma_s=0.5, step=0.5, optimizer=2, max_iterations=5, n_sigma_updates=2)
    K.assert_same_as_reference(m, ref)
    for rnd in (0, 1, -1):
        clf = m.mlp(None, rnd)
        assert clf.dim == 4
        assert _mlpdef.same(clf.predict_host(both), _mlpdef.sigmoid(_mlpdef.logits(ref["round_w"][rnd], 4, 5, both, mn, mx)))
        clf.close()
    m.close()


GRAD_CASES = [("shape_n129_d7_3_17", 30.0), ("shape_n65_d104_10_10", 8.0), ("shape_n192_d104_0_0", 1.0), ("shape_n63_d7_3_17", 30.0)]
GRAD_H = 1e-6
GRAD_TOL = 1.1e-8


def test_gradient_against_a_central_difference():
    """The second author's analytic gradient of the energy (wr 0.01, ws 1, sigma 0.5) against the central difference
    (E(w + h u_p) - E(w - h u_p)) / 2h of its own energy, h = 1e-6, on 40 weights per case; the weights are the definition's initial
    ones scaled up, under the first seed that keeps every pre-activation 1e-4 (100 steps) away from 0 (asserted): the difference crosses
    no kink of a ReLU.  Error measure: max_p |analytic - numeric| / max_p |analytic|.  Largest value measured on these cases on the CPU:
    1.03e-9; the tolerance is that with a x10 margin, rounded up: 1.1e-8."""
    worst = 0.0
    for name, scale in GRAD_CASES:
        kw = _kw(name)
        X, t = T.prepare(kw["rows"], kw["labels"])
        n1, n2 = kw["n1"], kw["n2"]
        for seed in range(11, 31):      # the first seed whose weights keep every pre-activation 1e-4 (100 steps) away from 0
            w = T.init_weights(seed, _mlpdef.n_weights(X.shape[1] - 1, n1, n2)) * scale
            if not n1:
                break
            W0, W1, _ = _mlpdef.split(w, X.shape[1] - 1, n1, n2)
            h1 = _mlpdef._dense(X, W0)
            h2 = _mlpdef._dense(_mlpdef._relu1(h1), W1)
            if min(np.abs(h1).min(), np.abs(h2).min()) > 1e-4:
                break
        if n1:
            assert min(np.abs(h1).min(), np.abs(h2).min()) > 1e-4, name
            assert (h1 > 0).any() and (h1 < 0).any() and (h2 > 0).any()
        E = T.Energy(n1, n2, X, t, 0.01, 1.0, 0.25)
        _, g = E(w, True)
        rng = np.random.default_rng(5)
        ps = rng.choice(w.size, size=min(w.size, 40), replace=False)
        num = np.empty(len(ps))
        for i, p in enumerate(ps):
            wp, wm = w.copy(), w.copy()
            wp[p] += GRAD_H; wm[p] -= GRAD_H
            num[i] = (E(wp, False)[0] - E(wm, False)[0]) / (wp[p] - wm[p])
        err = np.abs(g[ps] - num).max() / np.abs(g).max()
        print("central difference, %s: relative error %.3g" % (name, err))
        worst = max(worst, err)
    print("central difference, largest relative error %.3g (tolerance %.3g)" % (worst, GRAD_TOL))
    assert worst < GRAD_TOL


TOY_ITERATIONS = 200


def test_toy_set_is_separated():
    """40 rows in two columns, separable by the line x0 + x1 = 0 with a margin of 0.5: the definition (logsig and a 3 + 3 MLP, Adam,
    step 0.05, 200 iterations in one round) puts every row on its own side of 0.5 -- label +1 below (target 0.05), -1 above (0.95).
    Checked on the second author alone, then on the library."""
    rng = np.random.default_rng(2)
    rows = rng.uniform(-2.0, 2.0, (400, 2))
    rows = rows[np.abs(rows.sum(1)) > 0.5][:40]
    labels = np.where(rows.sum(1) > 0.0, 1, -1)
    assert len(rows) == 40 and 10 < (labels == 1).sum() < 30
    opts = dict(ws=1.0, sigma_s=1.0, optimizer=2, step=0.05, max_iterations=TOY_ITERATIONS, n_sigma_updates=1)
    for n1, n2 in ((0, 0), (3, 3)):
        ref = T.train(rows, labels, n1, n2, **opts)
        X, _ = T.prepare(rows, labels)
        f = T.forward(ref["round_w"][-1], n1, n2, X)
        assert ((f < 0.5) == (labels == 1)).all() and (np.abs(f - 0.5) > 0.05).all(), (n1, f)
        m = _hmt().train_mlp_host(rows, labels, n1, n2, **opts)
        K.assert_same_as_reference(m, ref)
        m.close()
