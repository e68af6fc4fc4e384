"""Shared cases of the merge-path term's tests: small inputs at every count of paths and unlabelled rows where a chunked
reduction or a kernel can go wrong, every tree shape that changes how paths share rows, and the option paths of the trainer with the
term on.  A case is (name, kwargs) for train(rows, labels, unlabelled, n1, n2, minmax, init, **opts); arrays are read-only.  The second
author's answer is computed once per case (reference())."""
import numpy as np

import _mlpdef as D
import _mlptrain_cases as MK
import _mlptraindef as T
import _sshmtdef as S


def caterpillar(n, key0=0):
    """n merges over n + 1 leaves, every merge joins the last created region with the next leaf: one path holds the root max_len times over"""
    R = n + 1
    o = [(key0, key0 + 1, key0 + R)]
    for k in range(1, n):
        o.append((key0 + R + k - 1, key0 + k + 1, key0 + R + k))
    return np.array(o, np.uint32).reshape(-1, 3)


def balanced(levels):
    """2^levels leaves merged level by level: at max 3 a level-2 merge lies on 7 paths"""
    R = 1 << levels
    live, o, nxt = list(range(R)), [], R
    while len(live) > 1:
        new = []
        for i in range(0, len(live), 2):
            o.append((live[i], live[i + 1], nxt))
            new.append(nxt)
            nxt += 1
        live = new
    return np.array(o, np.uint32)


def forest(n, R, seed):
    """n < R - 1 random merges over R leaves: several roots"""
    rng = np.random.default_rng([n, R, seed])
    live, o = list(range(R)), []
    for k in range(n):
        i, j = sorted(rng.choice(len(live), 2, replace=False))
        o.append((live[i], live[j], R + k))
        live.pop(j); live.pop(i)
        live.append(R + k)
    return np.array(o, np.uint32).reshape(-1, 3)


def _rows(n, dim, seed):
    rows = np.random.default_rng([n, dim, seed, 7]).standard_normal((n, dim))
    rows.setflags(write=False)
    return rows


def _block(order, dim, seed):
    order = np.array(order, np.uint32).reshape(-1, 3)
    order.setflags(write=False)
    return _rows(len(order), dim, seed), order


def _case(name, rows, labels, unlabelled, n1, n2, minmax=None, init=None, **opts):
    return name, dict(rows=rows, labels=labels, unlabelled=unlabelled, n1=n1, n2=n2, minmax=minmax, init=init, opts=opts)


BASE = dict(MK.BASE, wu=0.5, sigma_u=0.7)      # wr 0.01, ws 1, sigma_s 0.5, step 0.05, 3 iterations, 2 rounds


def cases():
    out = []
    rows, labels = MK._data(129, 7, 2)
    i = 0
    # P paths from a caterpillar of P + 2 merges at (3, 2): the path chunk short by one, exact, over by one, a last chunk of one path
    for P in (1, 63, 64, 65, 129):
        o = dict(BASE, optimizer=1 + i % 3, seed=i)
        if i % 2:
            o.update(step_decay=0.5)
        out.append(_case("paths_%d" % P, rows, labels, [_block(caterpillar(P + 2), 7, i)], 3, 17, **o))
        i += 1
    # N_u unlabelled rows, every one a path of its own at (1, 1); forests, so several roots
    for N in (2, 63, 64, 65, 130):
        o = dict(BASE, optimizer=1 + i % 3, seed=i, max_path_length=1, min_path_length=1)
        if i % 2:
            o.update(step_decay=0.5)
        out.append(_case("rows_%d" % N, rows, labels, [_block(forest(N, N + 9, i), 7, i)], 3, 17, **o))
        i += 1
    cat, bal, fst = caterpillar(70), balanced(5), forest(90, 120, 3)
    for mx, mn in ((1, 1), (2, 1), (3, 2), (8, 2), (8, 8)):
        for nm, order in (("caterpillar", cat), ("balanced", bal), ("forest", fst)):
            o = dict(BASE, optimizer=1 + i % 3, seed=i, max_path_length=mx, min_path_length=mn)
            if i % 2:
                o.update(step_decay=0.5)
            out.append(_case("len_%d_%d_%s" % (mx, mn, nm), rows, labels, [_block(order, 7, i)], 3, 17, **o))
            i += 1
    # the only merge yields no path at (3, 2): the term is off, as without blocks
    out.append(_case("no_path", rows, labels, [_block(caterpillar(1), 7, 1)], 3, 17, **BASE))
    out.append(_case("no_blocks", rows, labels, [], 3, 17, **BASE))
    # blocks of different row counts; members of later blocks are offset; keys of a block are its own
    out.append(_case("two_blocks", rows, labels, [_block(caterpillar(40), 7, 1), _block(balanced(4), 7, 2)], 3, 17, **BASE))
    out.append(_case("three_blocks", rows, labels, [_block(forest(50, 70, 5), 7, 1), _block(caterpillar(1), 7, 2), _block(caterpillar(66, key0=1000), 7, 3)], 3, 17,
                     **dict(BASE, step_decay=0.5, optimizer=2)))
    # a forest's small trees: merges on no path at (3, 3)
    out.append(_case("row_on_no_path", rows, labels, [_block(forest(40, 90, 8), 7, 4)], 3, 17, **dict(BASE, max_path_length=3, min_path_length=3)))
    # the term alone, without labelled rows; with the regulariser; all three; weights that isfeq 1
    ub = [_block(balanced(5), 7, 9)]
    out.append(_case("wu_only_no_labelled", None, None, ub, 3, 17, **dict(BASE, ws=0.0, wr=0.0)))
    out.append(_case("wu_wr", rows, labels, ub, 3, 17, **dict(BASE, ws=0.0, wr=1.0)))
    out.append(_case("wu_one", rows, labels, ub, 3, 17, **dict(BASE, wu=1.0)))
    out.append(_case("all_one", rows, labels, ub, 3, 17, **dict(BASE, wu=1.0, ws=1.0, wr=1.0, step_decay=0.5)))
    # sigma_u fixed (above), updated, held at the floor; together with sigma_s
    out.append(_case("usu", rows, labels, ub, 3, 17, **dict(BASE, update_sigma_u=1, sigma_u=0.0)))
    out.append(_case("usu_floor", rows, labels, ub, 3, 17, **dict(BASE, update_sigma_u=1, min_sigma2=10.0)))
    out.append(_case("usu_uss", rows, labels, ub, 3, 17, **dict(BASE, update_sigma_u=1, update_sigma_s=1, sigma_u=0.0, sigma_s=0.0, n_sigma_updates=3)))
    out.append(_case("lrds_fsdi", rows, labels, ub, 3, 17, **dict(BASE, n_sigma_updates=3, sigma_update_step_period=1, fixed_step_decay_iterations=2, max_iterations=4)))
    for opt in (1, 2, 3):
        out.append(_case("adaptive_big_lr_opt%d" % opt, rows, labels, ub, 3, 17, **dict(BASE, optimizer=opt, step=1e3 if opt != 2 else 50.0, step_decay=0.25)))
    # logsig at zero weights: f = 0.5 exactly; n = 1, merge_target 0.5: F_0 = F_1 = 0, D = 1, e = 1 - 1 = 0 exactly: every path is skipped
    out.append(_case("logsig_e_zero", rows, labels, [_block(forest(30, 40, 2), 7, 5)], 0, 0,
                     **dict(BASE, ws=0.0, wr=1.0, merge_target=0.5, max_path_length=1, min_path_length=1)))
    out.append(_case("logsig", rows, labels, ub, 0, 0, init=np.linspace(-0.3, 0.3, 8), **BASE))
    out.append(_case("path_target", rows, labels, ub, 3, 17, **dict(BASE, path_target=0.9, merge_target=0.8)))
    # shapes: one unit, 10 + 10 and 32 + 32 units, one column and 104 columns
    for dim, n1, n2 in ((1, 1, 1), (104, 10, 10), (104, 32, 32), (1, 0, 0), (104, 0, 0)):
        r2, l2 = MK._data(65, dim, 3)
        o = dict(BASE, seed=i)
        init = None if n1 else np.linspace(-0.3, 0.3, dim + 1)
        out.append(_case("shape_d%d_%d_%d" % (dim, n1, n2), r2, l2, [_block(forest(70, 80, i), dim, i)], n1, n2, init=init, **o))
        i += 1
    # dropped labelled rows; a min/max table over both kinds of rows
    lab0 = np.array(labels)
    lab0[::3] = 0
    urows, uorder = ub[0]
    out.append(_case("label0_minmax", rows, lab0, ub, 3, 17, minmax=(np.minimum(rows.min(axis=0), urows.min(axis=0)) - 0.5,
                                                                  np.maximum(rows.max(axis=0), urows.max(axis=0)) + 0.25), **BASE))
    # zero rows under zero biases: dead units by the <= rule, in the unlabelled rows too
    zu = np.array(urows)
    zu[3, :] = 0.0
    zu[30, :] = 0.0
    zw = np.array(T.init_weights(7, D.n_weights(7, 3, 17))) * 30.0
    zw[7::8][:3] = 0.0
    zw[8 * 3 + 3::4][:17] = 0.0
    out.append(_case("zero_row_dead_units", rows[:65], labels[:65], [(zu, uorder)], 3, 17, init=zw, **BASE))
    # a saturated sigmoid: f exactly 0 and 1 on the paths
    sat = np.zeros(8)
    sat[0] = 2000.0
    out.append(_case("logsig_saturated", rows, labels, ub, 0, 0, init=sat, **dict(BASE, wr=0.0)))
    out.append(_case("divergent_fixed", rows, labels, ub, 3, 17, **dict(BASE, wr=1.0, step=1e200)))
    for _, kw in out:
        for a in (kw["init"],) + (kw["minmax"] or ()) + tuple(b[0] for b in kw["unlabelled"]):
            if a is not None:
                a.setflags(write=False)
    return out


CASES = cases()
IDS = [name for name, _ in CASES]
_REF = {}


def reference(name):
    """the second author's result for a case, computed once"""
    if name not in _REF:
        kw = CASES[IDS.index(name)][1]
        _REF[name] = S.train(kw["rows"], kw["labels"], kw["unlabelled"], kw["n1"], kw["n2"], kw["minmax"], kw["init"], **kw["opts"])
    return _REF[name]


def assert_same_as_reference(model, ref, exact=True, rtol=1e-9):
    """as _mlptrain_cases.assert_same_as_reference, and the sigma_u series, the paths and the unlabelled rows"""
    MK.assert_same_as_reference(model, ref, exact, rtol)
    for k in ("sigma_u2", "sigma_u2_eval"):
        a, b = np.asarray(getattr(model, k), np.float64), np.asarray(ref[k], np.float64)
        assert D.same(a, b) if exact else (a.shape == b.shape and np.allclose(a, b, rtol=rtol, atol=0.0, equal_nan=True)), k + " differs"
    assert model.n_paths == ref["n_paths"] and model.n_uns_rows == ref["n_uns_rows"]
