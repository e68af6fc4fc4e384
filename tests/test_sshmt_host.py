"""The merge-path (unsupervised) term on the host (glia_hmt_sshmt_train_host, glia_hmt_merge_paths: glia_amd/csrc/sshmt_paths.hpp, the
definition of DESIGN 3.15) against the second author tests/_sshmtdef.py: known merge paths and the paths the reference's own
genMergePaths wrote (tests/golden/sshmt/merge_paths.npz); weights after every round, trace and both sigma series bit for bit on every
shared case; the order of the energy's terms; the second author's gradient against a central difference of its own energy; the
supervised path unchanged; refusals and defaults.  No GPU."""
import os

import numpy as np
import pytest

import _mlpdef
import _mlptrain_cases as MK
import _mlptraindef as T
import _sshmt_cases as K
import _sshmtdef as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sshmt", "merge_paths.npz")
KNOWN = np.array([[1, 2, 7], [3, 4, 8], [7, 8, 9], [5, 6, 10], [9, 10, 11]], np.uint32)


def _hmt():
    from glia_amd import hmt
    return hmt


def _train(kw, **more):
    o = dict(kw["opts"])
    o.update(more)
    return _hmt().train_sshmt_host(kw["rows"], kw["labels"], kw["unlabelled"], kw["n1"], kw["n2"], kw["minmax"], kw["init"], **o)


def _kw(name):
    return K.CASES[K.IDS.index(name)][1]


def test_known_merge_paths():
    """two leaf merges under one parent under the root, and a third leaf merge under the root alone: at (3, 2) the two full paths and the
    short one that starts at a leaf merge; the parent's own path (2 members, children created) is not kept"""
    hmt = _hmt()
    want = [[0, 2, 4], [1, 2, 4], [3, 4]]
    assert [p.tolist() for p in hmt.merge_paths(KNOWN, 3, 2)] == want == S.merge_paths(KNOWN, 3, 2)
    assert [p.tolist() for p in hmt.merge_paths(KNOWN, 1, 1)] == [[0], [1], [2], [3], [4]]
    assert [p.tolist() for p in hmt.merge_paths(KNOWN, 2, 2)] == [[0, 2], [1, 2], [2, 4], [3, 4]]
    assert [p.tolist() for p in hmt.merge_paths(KNOWN, 8, 1)] == [[0, 2, 4], [1, 2, 4], [3, 4]]
    assert hmt.merge_paths(np.zeros((0, 3), np.uint32)) == []
    assert hmt.merge_paths([[5, 9, 2]], 3, 2) == [] and [p.tolist() for p in hmt.merge_paths([[5, 9, 2]], 3, 1)] == [[0]]


def test_merge_paths_equal_the_references_own():
    """every order of the fixture at (3, 2), (2, 1) and (5, 3): the library and the second author give the paths genMergePaths wrote"""
    hmt = _hmt()
    z = np.load(GOLDEN)
    names = [k[len("order_"):] for k in z.files if k.startswith("order_")]
    assert len(names) >= 10 and "synth32_pb_mean" in names
    total = 0
    for name in names:
        order = z["order_" + name]
        for mx, mn in ((3, 2), (2, 1), (5, 3)):
            off, mem = z["offsets_%s_%d_%d" % (name, mx, mn)], z["members_%s_%d_%d" % (name, mx, mn)]
            want = [mem[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
            assert [p.tolist() for p in hmt.merge_paths(order, mx, mn)] == want, (name, mx, mn)
            assert S.merge_paths(order, mx, mn) == want, (name, mx, mn)
            total += len(want)
    assert total > 5000


@pytest.mark.parametrize("name", K.IDS)
def test_host_equals_second_author(name):
    m = _train(_kw(name))
    K.assert_same_as_reference(m, K.reference(name))
    m.close()


def test_cases_reach_what_they_are_for():
    """read from the second author's results: the properties the cases were chosen for"""
    for P in (1, 63, 64, 65, 129):
        assert K.reference("paths_%d" % P)["n_paths"] == P
    for N in (2, 63, 64, 65, 130):
        r = K.reference("rows_%d" % N)
        assert r["n_uns_rows"] == N == r["n_paths"]
    assert K.reference("no_path")["n_paths"] == 0 and K.reference("no_path")["n_uns_rows"] == 1
    # the term off: the supervised trainer's answer, and sigma_u never evaluated
    a, b = K.reference("no_path"), K.reference("no_blocks")
    assert all(_mlpdef.same(x, y) for x, y in zip(a["round_w"], b["round_w"])) and a["sigma_u2_eval"] == [0.0] * 3
    # one path holds the root max_len times over (caterpillar); a level-2 merge lies on 7 paths at max 3 (balanced)
    assert S.merge_paths(K.caterpillar(70), 8, 8)[-1] == list(range(62, 70))
    on = [sum(p.count(16 + 8) for p in S.merge_paths(K.balanced(5), 3, 2))]
    assert on == [7]
    kw = _kw("row_on_no_path")
    named = {r for p in S.merge_paths(kw["unlabelled"][0][1], 3, 3) for r in p}
    assert 0 < len(named) < len(kw["unlabelled"][0][1])
    u = K.reference("three_blocks")
    assert u["n_uns_rows"] == 50 + 1 + 66 and u["n_paths"] > 64
    # sigma_u: fixed, updated, held at the floor
    assert K.reference("wu_one")["sigma_u2"] == [0.7 * 0.7] * 3
    r = K.reference("usu")
    assert r["sigma_u2"] == r["sigma_u2_eval"] and len(set(r["sigma_u2"])) == 3 and min(r["sigma_u2"]) > 0.0
    r = K.reference("usu_floor")
    assert r["sigma_u2"] == [10.0] * 3 == r["sigma_u2_eval"]
    # every path skipped: e = 0 exactly, the weights never move, L_U = 0
    r = K.reference("logsig_e_zero")
    assert all((w == 0.0).all() for w in r["round_w"]) and r["sigma_u2_eval"] == [0.0] * 3 and r["n_paths"] == 30
    assert K.reference("divergent_fixed")["stopped_nonfinite"]
    # the term changes the answer
    kw = _kw("wu_one")
    sup = T.train(kw["rows"], kw["labels"], kw["n1"], kw["n2"], None, None, **{k: v for k, v in kw["opts"].items() if k not in ("wu", "sigma_u")})
    assert not _mlpdef.same(sup["round_w"][-1], K.reference("wu_one")["round_w"][-1])


def _terms(kw, w):
    """the three terms of the energy at w, each evaluated alone by the second author"""
    o = dict(S.DEFAULTS)
    o.update(kw["opts"])
    X, t = T.prepare(kw["rows"], kw["labels"])
    U = S.Uns(kw["unlabelled"], None, None, o["max_path_length"], o["min_path_length"], o["merge_target"], o["path_target"])
    s2, su2 = o["sigma_s"] ** 2, o["sigma_u"] ** 2
    return [S.Energy(kw["n1"], kw["n2"], X, t, U, wr, wu, ws, s2, su2)(w, False)[0]
            for wr, wu, ws in ((o["wr"], 0.0, 0.0), (0.0, o["wu"], 0.0), (0.0, 0.0, o["ws"]))]


def test_energy_takes_its_terms_in_the_order_r_u_s():
    """fx of the first evaluation is ((0 + r) + u) + s; on the cases named here adding s before u gives another last bit"""
    seen = 0
    for name in ("paths_63", "wu_one", "all_one", "two_blocks", "path_target", "len_3_2_balanced"):
        kw = _kw(name)
        ref = K.reference(name)
        w0 = T.init_weights(kw["opts"].get("seed", 0), ref["round_w"][0].size)
        r, u, s = _terms(kw, w0)
        assert ref["trace"][0][0] == (r + u) + s, name
        m = _train(kw)
        assert m.trace["fx"][0] == (r + u) + s
        m.close()
        seen += (r + s) + u != (r + u) + s
    assert seen >= 1


GRAD_H = 1e-6
GRAD_TOL = 1.4e-6
GRAD_CASES = [("wu_one", 30.0), ("len_8_2_caterpillar", 30.0), ("two_blocks", 30.0), ("logsig", 1.0), ("shape_d104_10_10", 10.0)]


def test_gradient_against_a_central_difference():
    """The second author's analytic gradient of the three-term energy (wr 0.01, wu 0.5, ws 1, sigma_u 0.7, sigma_s 0.5) against the
    central difference (E(w + h u_p) - E(w - h u_p)) / 2h of its own energy, h = 1e-6, on 40 weights per case; the weights are the
    definition's initial ones scaled up, under the first seed that keeps every pre-activation of labelled and unlabelled rows 1e-4
    (100 steps) away from 0 (asserted): the difference crosses no kink of a ReLU.  Error measure: max_p |analytic - numeric| /
    max_p |analytic|, for the three-term energy and for the term alone (wr = ws = 0), where its own gradient is the scale.  Largest
    value measured on these cases on the CPU: 1.38e-7 (the term alone at path length 8, where its gradient is 0.006 under an energy of
    tens: the difference's own rounding; every other figure is below 3.3e-9); the tolerance is that with a x10 margin, rounded up:
    1.4e-6."""
    worst = 0.0
    for name, scale in GRAD_CASES:
        kw = _kw(name)
        o = dict(S.DEFAULTS)
        o.update(kw["opts"])
        X, t = T.prepare(kw["rows"], kw["labels"])
        U = S.Uns(kw["unlabelled"], None, None, o["max_path_length"], o["min_path_length"], o["merge_target"], o["path_target"])
        assert U.P > 0
        n1, n2 = kw["n1"], kw["n2"]
        XX = np.concatenate([X, U.X], axis=0)
        for seed in range(11, 61):
            w = T.init_weights(seed, _mlpdef.n_weights(X.shape[1] - 1, n1, n2)) * scale
            if not n1:
                w = np.array(kw["init"])
                break
            W0, W1, _ = _mlpdef.split(w, X.shape[1] - 1, n1, n2)
            h1 = _mlpdef._dense(XX, W0)
            h2 = _mlpdef._dense(_mlpdef._relu1(h1), W1)
            if min(np.abs(h1).min(), np.abs(h2).min()) > 1e-4:
                break
        if n1:
            assert min(np.abs(h1).min(), np.abs(h2).min()) > 1e-4, name
            assert (h1 > 0).any() and (h1 < 0).any() and (h2 > 0).any()
        rng = np.random.default_rng(5)
        ps = rng.choice(w.size, size=min(w.size, 40), replace=False)
        # the three-term energy, then the term alone: in the sum the supervised term can dwarf it
        for what, E in (("r + u + s", S.Energy(n1, n2, X, t, U, 0.01, 0.5, 1.0, 0.25, 0.49)), ("u alone", S.Energy(n1, n2, X, t, U, 0.0, 0.5, 0.0, 0.25, 0.49))):
            _, g = E(w, True)
            assert np.abs(g).max() > 0.0
            num = np.empty(len(ps))
            for i, p in enumerate(ps):
                wp, wm = w.copy(), w.copy()
                wp[p] += GRAD_H; wm[p] -= GRAD_H
                num[i] = (E(wp, False)[0] - E(wm, False)[0]) / (wp[p] - wm[p])
            err = np.abs(g[ps] - num).max() / np.abs(g).max()
            print("central difference, %s, %s: relative error %.3g (largest |g| %.3g)" % (name, what, err, np.abs(g).max()))
            worst = max(worst, err)
    print("central difference, largest relative error %.3g (tolerance %.3g)" % (worst, GRAD_TOL))
    assert worst < GRAD_TOL


def test_dnf_derivative_against_a_central_difference():
    """a_i = dD/df_i of the second author against (D(f + h) - D(f - h)) / 2h, n = 1 .. 8: below 1e-8 (measured: at most 7e-11)"""
    rng = np.random.default_rng(3)
    for n in range(1, S.MAX_PATH + 1):
        f = rng.uniform(0.1, 0.9, n).tolist()
        Tn = 0.95 ** n
        _, _, a = S.path_terms(f, Tn, 1.0)
        for i in range(n):
            fp, fm = list(f), list(f)
            fp[i] += 1e-6; fm[i] -= 1e-6
            num = (S.path_terms(fp, Tn, 1.0, False)[0] - S.path_terms(fm, Tn, 1.0, False)[0]) / (fp[i] - fm[i])
            assert abs(a[i] - num) < 1e-8, (n, i)


@pytest.mark.parametrize("name", ["shape_n65_d7_3_17", "uss", "adaptive_big_lr_opt2", "label0_interleaved", "minmax", "shape_n129_d104_0_0"])
def test_without_the_term_the_supervised_trainer_is_unchanged(name):
    """train_sshmt_host with wu = 0 (with and without blocks) returns the bytes train_mlp_host returns"""
    hmt = _hmt()
    kw = MK.CASES[MK.IDS.index(name)][1]
    a = hmt.train_mlp_host(kw["rows"], kw["labels"], kw["n1"], kw["n2"], kw["minmax"], kw["init"], **kw["opts"])
    blk = [K._block(K.balanced(4), kw["rows"].shape[1], 1)]
    for unl in ([], blk):
        b = hmt.train_sshmt_host(kw["rows"], kw["labels"], unl, kw["n1"], kw["n2"], kw["minmax"], kw["init"], **kw["opts"])
        assert a.rounds == b.rounds and a.trace.tobytes() == b.trace.tobytes()
        for r in range(a.rounds):
            assert a.weights(r).tobytes() == b.weights(r).tobytes()
        assert a.sigma2.tobytes() == b.sigma2.tobytes() and a.sigma2_eval.tobytes() == b.sigma2_eval.tobytes()
        assert (b.sigma_u2 == 0.0).all() and b.n_paths == (12 if unl else 0)
    assert a.n_paths == 0 and a.n_uns_rows == 0 and (a.sigma_u2 == 0.0).all()


@pytest.mark.parametrize("name,kw", MK.NO_TERM_CASES, ids=[n for n, _ in MK.NO_TERM_CASES])
def test_no_block_and_no_wu_is_the_supervised_trainer_byte_for_byte(name, kw):
    """mlp_backward.hpp: "without U not one operation differs from the supervised trainer" -- both entry points run one routine"""
    hmt = _hmt()
    a = hmt.train_mlp_host(kw["rows"], kw["labels"], kw["n1"], kw["n2"], kw["minmax"], kw["init"], **kw["opts"])
    b = hmt.train_sshmt_host(kw["rows"], kw["labels"], (), kw["n1"], kw["n2"], kw["minmax"], kw["init"], **dict(kw["opts"], wu=0.0))
    assert a.rounds == 2 and a.n_used_rows == 65 and int((a.trace["kind"] == 0).sum()) > 0
    MK.assert_identical_models(a, b)
    assert b.n_paths == 0 and (b.sigma_u2 == 0.0).all()


def test_defaults():
    hmt = _hmt()
    import ctypes as C
    o = hmt.SSHMTTrainOpts()
    hmt.lib().glia_hmt_sshmt_train_opts_default(C.byref(o))
    assert (o.sigma_u, o.merge_target, o.path_target, o.max_path_length, o.min_path_length) == (0.0, 0.95, 1.0, 3, 2)
    assert (o.base.n1, o.base.n2, o.base.wu, o.base.update_sigma_u, o.base.pos_target, o.base.neg_target) == (10, 10, 0.0, 0, 0.05, 0.95)
    assert (S.MAX_PATH, S.PATH_CHUNK, S.CHUNK) == (8, 64, hmt.mlp_train_limits()["chunk_rows"])


ROWS = np.arange(12.0).reshape(4, 3)
LAB = [1, -1, 1, -1]
UNL = [(np.arange(15.0).reshape(5, 3) / 7.0, KNOWN)]
GOOD = dict(ws=1.0, wu=1.0, sigma_s=0.5, sigma_u=0.5, step=0.01, max_iterations=1, n_sigma_updates=1)


@pytest.mark.parametrize("opts,code,words", [
    (dict(ws=0.0, wu=0.0), "arg", "wr, wu and ws"),
    (dict(sigma_u=0.0), "arg", "sigma_u"),
    (dict(sigma_s=0.0), "arg", "sigma_s"),
    (dict(wu=float("nan")), "arg", "not finite"),
    (dict(merge_target=float("inf")), "arg", "merge_target"),
    (dict(max_path_length=-1), "unsupported", "max_path_length < 0"),
    (dict(max_path_length=9), "unsupported", "max_path_length above 8"),
    (dict(min_path_length=0), "unsupported", "min_path_length"),
    (dict(min_path_length=4), "unsupported", "min_path_length"),
    (dict(uns_batch_size=8), "unsupported", "uns_batch_size"),
    (dict(sup_batch_size=8), "unsupported", "sup_batch_size"),
    (dict(balance_sup_batch=1), "unsupported", "balance_sup_batch"),
    (dict(alt_su=1), "unsupported", "alt_su"),
])
def test_option_errors_and_refusals(opts, code, words):
    hmt = _hmt()
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_sshmt_host(ROWS, LAB, UNL, 3, 3, **dict(GOOD, **opts))
    assert e.value.code == (hmt.ERR_ARG if code == "arg" else -3) and words in str(e.value)


def test_argument_errors():
    hmt = _hmt()
    m = hmt.train_sshmt_host(ROWS, LAB, UNL, 3, 3, **GOOD)
    assert m.n_paths == 3 and m.n_uns_rows == 5 and m.rounds == 1
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_sshmt_host(ROWS, LAB, UNL, 33, 33, **GOOD)
    assert e.value.code == -3 and "32 units" in str(e.value)
    with pytest.raises(hmt.HmtError) as e:      # rows and merges disagree (caught before the library: it takes one count)
        hmt.train_sshmt_host(ROWS, LAB, [(UNL[0][0][:4], KNOWN)], 3, 3, **GOOD)
    assert e.value.code == hmt.ERR_ARG and "one row" in str(e.value)
    for bad_order, merge in (([[1, 2, 7], [1, 3, 8]], 1), ([[7, 3, 8], [1, 2, 7]], 0), ([[1, 2, 7], [3, 4, 7]], 1), ([[1, 1, 7]], 0)):
        with pytest.raises(hmt.HmtError) as e:
            hmt.train_sshmt_host(ROWS, LAB, [(np.ones((len(bad_order), 3)), bad_order)], 3, 3, **GOOD)
        assert e.value.code == hmt.ERR_ARG and "block 0: merge %d" % merge in str(e.value)
        with pytest.raises(hmt.HmtError) as e:
            hmt.merge_paths(bad_order)
        assert e.value.code == hmt.ERR_ARG and "merge %d" % merge in str(e.value)
    bad = np.array(UNL[0][0])
    bad[2, 1] = np.nan
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_sshmt_host(ROWS, LAB, [UNL[0], (bad, KNOWN)], 3, 3, **GOOD)
    assert e.value.code == hmt.ERR_ARG and "block 1: row 2" in str(e.value) and "not finite" in str(e.value)
    with pytest.raises(hmt.HmtError) as e:      # ws on without labelled rows
        hmt.train_sshmt_host(None, None, UNL, 3, 3, **GOOD)
    assert e.value.code == hmt.ERR_ARG and "no row is labelled" in str(e.value)
    m2 = hmt.train_sshmt_host(None, None, UNL, 3, 3, **dict(GOOD, ws=0.0))
    assert m2.n_used_rows == 0 and m2.n_paths == 3
    with pytest.raises(hmt.HmtError) as e:
        hmt.merge_paths(KNOWN, 9, 2)
    assert e.value.code == -3 and "above 8" in str(e.value)
    with pytest.raises(TypeError):
        hmt.train_sshmt_host(ROWS, LAB, UNL, 3, 3, **dict(GOOD, nonsense=1))
    # the supervised entry point keeps refusing the term by name
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_mlp_host(ROWS, LAB, 3, 3, **dict(ws=1.0, sigma_s=0.5, wu=1.0))
    assert e.value.code == -3 and "wu" in str(e.value)


def test_model_feeds_the_predictor_and_a_file_round_trip(tmp_path):
    hmt = _hmt()
    kw = _kw("label0_minmax")
    m = _train(kw)
    p = tmp_path / "model.txt"
    m.write(p)
    w = hmt.mlp_file_parse(str(p))
    assert np.asarray(w).tobytes() == m.weights().tobytes()
    clf = m.mlp(None)
    mn, mx = kw["minmax"]
    got = clf.predict_host(np.ascontiguousarray(kw["unlabelled"][0][0]))
    assert _mlpdef.same(got, hmt.mlp_predict_host(m.weights(), kw["n1"], kw["n2"], kw["unlabelled"][0][0], mn, mx)[0])
    clf.close()
