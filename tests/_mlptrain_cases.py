"""Shared cases of the MLP / logsig trainer's tests: small inputs at every shape where the chunked reduction or the chunk
kernel can go wrong, and the option paths of the trainer.  A case is (name, kwargs) for train(rows, labels, n1, n2, minmax, init, **opts);
arrays are read-only.  The second author's answer is computed once per case (reference())."""
import numpy as np

import _mlpdef as D
import _mlptraindef as T

N_ROWS = [1, 63, 64, 65, 129, 192]          # one row; a chunk short by one, exact, over by one; a last chunk of one row; three chunks
SHAPES = [(1, 1, 1), (7, 3, 17), (104, 10, 10), (104, 32, 32), (1, 0, 0), (104, 0, 0)]      # (dim, n1, n2); 0, 0: logsig


def _data(n, dim, seed, labels=None):
    rng = np.random.default_rng([n, dim, seed])
    rows = rng.standard_normal((n, dim))
    if labels is None:
        labels = np.where(rows[:, 0] + 0.3 * rng.standard_normal(n) > 0.0, 1, -1)
    rows.setflags(write=False)
    labels = np.asarray(labels, np.int32)
    labels.setflags(write=False)
    return rows, labels


def _case(name, rows, labels, n1, n2, minmax=None, init=None, **opts):
    return name, dict(rows=rows, labels=labels, n1=n1, n2=n2, minmax=minmax, init=init, opts=opts)


BASE = dict(ws=1.0, wr=0.01, sigma_s=0.5, step=0.05, max_iterations=3, n_sigma_updates=2)


def cases():
    out = []
    i = 0
    for n in N_ROWS:
        for dim, n1, n2 in SHAPES:
            rows, labels = _data(n, dim, 1)
            o = dict(BASE, optimizer=1 + i % 3)
            if i % 2:
                o.update(step_decay=0.5)                      # the adaptive rule on every other shape
            if n1:
                o.update(seed=i)
            else:
                o.update(init=np.linspace(-0.3, 0.3, dim + 1))
            init = o.pop("init", None)
            out.append(_case("shape_n%d_d%d_%d_%d" % (n, dim, n1, n2), rows, labels, n1, n2, init=init, **o))
            i += 1
    rows, labels = _data(129, 7, 2)
    for opt in (1, 2, 3):
        out.append(_case("fixed_lrdi2_opt%d" % opt, rows, labels, 3, 17, **dict(BASE, optimizer=opt, max_iterations=5, fixed_step_decay_iterations=2)))
        out.append(_case("adaptive_big_lr_opt%d" % opt, rows, labels, 3, 17, **dict(BASE, optimizer=opt, step=1e3 if opt != 2 else 50.0, step_decay=0.25, max_iterations=3)))
    out.append(_case("lrds", rows, labels, 3, 17, **dict(BASE, n_sigma_updates=3, sigma_update_step_period=1, max_iterations=2)))
    out.append(_case("uss", rows, labels, 3, 17, **dict(BASE, update_sigma_s=1, sigma_s=0.0)))
    out.append(_case("uss_floor", rows, labels, 3, 17, **dict(BASE, update_sigma_s=1, min_sigma2=10.0)))
    out.append(_case("wr_only", rows, labels, 3, 17, **dict(BASE, ws=0.0, wr=1.0)))
    out.append(_case("ws_only", rows, labels, 3, 17, **dict(BASE, wr=0.0)))
    out.append(_case("ws_half", rows, labels, 3, 17, **dict(BASE, ws=0.5, wr=1.0)))
    lab0 = np.array(labels)
    lab0[::3] = 0
    lab0[5] = 2
    out.append(_case("label0_interleaved", rows, lab0, 3, 17, **BASE))
    out.append(_case("one_class", rows, np.ones(129, np.int32), 3, 17, **BASE))
    out.append(_case("minmax", rows, labels, 3, 17, minmax=(rows.min(axis=0) - 0.5, rows.max(axis=0) + 0.25), **BASE))
    out.append(_case("no_rounds", rows, labels, 3, 17, **dict(BASE, n_sigma_updates=0)))
    # logsig at zero weights with both targets 0.5: every e_i is exactly 0, the gradient is exactly wr * w = 0 and L exactly 0
    out.append(_case("logsig_e_zero", rows, labels, 0, 0, **dict(BASE, pos_target=0.5, neg_target=0.5, wr=1.0)))
    # a row of zeros under zero biases: hidden sums of exactly 0.0, dead by the <= rule
    zrows = np.array(rows[:65])
    zrows[3, :] = 0.0
    zrows[64, :] = 0.0
    zw = np.array(T.init_weights(7, D.n_weights(7, 3, 17))) * 30.0
    zw[7::8][:3] = 0.0                                     # first-layer biases (row D - 1 of each column)
    o1 = 8 * 3
    zw[o1 + 3::4][:17] = 0.0                               # second-layer biases
    out.append(_case("zero_row_dead_units", zrows, labels[:65], 3, 17, init=zw, **BASE))
    # weights that saturate the sigmoid to exactly 0 and 1
    sat = np.zeros(8)
    sat[0] = 2000.0
    out.append(_case("logsig_saturated", rows, labels, 0, 0, init=sat, **dict(BASE, wr=0.0)))
    # a step so large that the energy overflows: stopped_nonfinite, weights restored
    out.append(_case("divergent_fixed", rows, labels, 3, 17, **dict(BASE, wr=1.0, step=1e200)))
    out.append(_case("divergent_adaptive", rows, labels, 3, 17, **dict(BASE, wr=1.0, step=1e300, step_decay=0.999999)))
    for _, kw in out:
        for a in (kw["init"],) + (kw["minmax"] or ()):
            if a is not None:
                a.setflags(write=False)
    return out


CASES = cases()
IDS = [name for name, _ in CASES]


def _no_term_cases():
    """train_sshmt given no unlabelled block and wu = 0 must be train_mlp byte for byte (one routine runs both): 65 rows are a chunk and
    a row, 3 + 17 units the kernel's <32> instantiation; Adam with the adaptive rule asks for L alone as well as for the gradient."""
    rows, labels = _data(65, 5, 3)
    adaptive_adam = dict(BASE, optimizer=2, step_decay=0.5, n_sigma_updates=2)
    return [_case("mlp_3_17_n65_d5_adam_adaptive", rows, labels, 3, 17, **dict(adaptive_adam, seed=11)),
            _case("logsig_n65_d5_adam_adaptive", rows, labels, 0, 0, init=np.linspace(-0.3, 0.3, 6), **adaptive_adam)]


NO_TERM_CASES = _no_term_cases()


def assert_identical_models(a, b):
    """the weights of every round, the trace and sigma2: the same bytes"""
    assert a.rounds == b.rounds and a.stopped_nonfinite == b.stopped_nonfinite
    for r in range(a.rounds):
        assert a.weights(r).tobytes() == b.weights(r).tobytes(), "weights after round %d differ" % r
    assert len(a.trace) > 0 and a.trace.tobytes() == b.trace.tobytes()
    assert a.sigma2.tobytes() == b.sigma2.tobytes() and a.sigma2_eval.tobytes() == b.sigma2_eval.tobytes()
_REF = {}


def reference(name):
    """the second author's result for a case, computed once"""
    if name not in _REF:
        kw = dict(CASES[IDS.index(name)][1])
        _REF[name] = T.train(kw["rows"], kw["labels"], kw["n1"], kw["n2"], kw["minmax"], kw["init"], **kw["opts"])
    return _REF[name]


def trace_array(trace):
    """trace tuples -> (floats [n, 5], ints [n, 4])"""
    f = np.array([r[:5] for r in trace], np.float64).reshape(-1, 5)
    i = np.array([r[5:] for r in trace], np.int64).reshape(-1, 4)
    return f, i


def model_trace_array(model):
    tr = model.trace
    f = np.stack([tr[k] for k in ("fx", "xnorm", "gnorm", "step", "sigma2")], axis=1).reshape(-1, 5) if len(tr) else np.zeros((0, 5))
    i = np.stack([tr[k] for k in ("round", "t", "kind", "rollbacks")], axis=1).astype(np.int64).reshape(-1, 4) if len(tr) else np.zeros((0, 4), np.int64)
    return f, i


def assert_same_as_reference(model, ref, exact=True, rtol=1e-9):
    """weights after every round, trace and sigmas: bit for bit, or (exact=False) to rtol"""
    def same(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        if exact:
            return D.same(a, b)
        return a.shape == b.shape and np.allclose(a, b, rtol=rtol, atol=0.0, equal_nan=True)
    assert model.stopped_nonfinite == ref["stopped_nonfinite"]
    assert model.rounds == len(ref["round_w"])
    for r in range(model.rounds):
        assert same(model.weights(r), ref["round_w"][r]), "weights after round %d differ" % r
    f, i = model_trace_array(model)
    rf, ri = trace_array(ref["trace"])
    assert i.shape == ri.shape and (i == ri).all(), "trace structure differs"
    assert same(f, rf), "trace values differ"
    assert same(model.sigma2, ref["sigma2"]) and same(model.sigma2_eval, ref["sigma2_eval"])
