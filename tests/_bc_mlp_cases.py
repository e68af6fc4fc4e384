"""One-column MLP models for the classifier loop's tests (test_gpu_bc_mlp.py): the first layer is non-zero only in row STUB (x0.b0.mean,
the stub scorer's column) and in the bias row, w1 and w2 are dense.  Every other column then adds +-0 to a chain that starts at +0.0, so
the probability is a function F(mean) alone and tests/_loopdef.py -- the loop under a one-column scorer -- gives the expected order.
F is computed by tests/_mlpdef.py on rows that are zero except that column, never by the library."""
import numpy as np

import _featdef
import _mlpdef

NAMES = _featdef.column_names(2, 3, [8], [], [8])          # the common configuration: pb on the region and boundary lists, 8 bins
DIM = len(NAMES)
STUB = NAMES.index("x0.b0.mean")


def one_column_weights(rng, n1, n2, gain=1.0, first=None):
    """weights of a model file (w0 | w1 | w2, column-major); first: (slopes [n1], offsets [n1]) of layer 1, default random"""
    D = DIM + 1
    w0 = np.zeros((n1, D))                                  # unit k: w0[k, j] = file value j + D k
    slope, offset = first if first is not None else (rng.standard_normal(n1) * 3.0, rng.standard_normal(n1))
    w0[:, STUB], w0[:, DIM] = slope, offset
    w1 = rng.standard_normal((n2, n1 + 1))
    w2 = rng.standard_normal(n2 + 1) * gain
    return np.concatenate([w0.ravel(), w1.ravel(), w2])


def minmax(rng):
    """arbitrary finite entries in all columns, max above min"""
    mn = rng.standard_normal(DIM)
    return mn, mn + 0.5 + rng.random(DIM) * 4.0


def score_of(weights, n1, n2, mn=None, mx=None, dist=None):
    """F: an array of means -> the model's probabilities, by _mlpdef"""
    def F(mean):
        mean = np.asarray(mean, np.float64)
        rows = np.zeros((mean.size, DIM))
        rows[:, STUB] = mean.ravel()
        return _mlpdef.sigmoid(_mlpdef.logits(weights, n1, n2, rows, mn, mx, dist)).reshape(mean.shape)
    return F


def models(limit):
    """name -> dict(weights, n1, n2, mn, mx, dist); limit: the loop's largest hidden layer"""
    rng = np.random.default_rng(20261020)
    out = {}
    out["10+10"] = dict(weights=one_column_weights(rng, 10, 10), n1=10, n2=10)
    out["1+1"] = dict(weights=one_column_weights(rng, 1, 1, first=(np.array([2.5]), np.array([-0.25]))), n1=1, n2=1)
    out["limit"] = dict(weights=one_column_weights(rng, limit, limit, gain=0.3), n1=limit, n2=limit)
    mn, mx = minmax(rng)
    out["10+10 minmax"] = dict(weights=one_column_weights(rng, 10, 10), n1=10, n2=10, mn=mn, mx=mx)
    # every unit of layer 1 is relu(a_k (mean - 0.3)), a_k > 0: below 0.3 the first layer is dead and F is constant
    a = 1.0 + rng.random(10) * 4.0
    out["dead relu"] = dict(weights=one_column_weights(rng, 10, 10, first=(a, -0.3 * a)), n1=10, n2=10)
    # logit = 4000 (0.5 - mean) through two positive units: probabilities from exactly 1.0 down to below 1e-300
    sat = np.zeros(2 * (DIM + 1) + 3 * 2 + 3)
    D = DIM + 1
    sat[STUB], sat[D + DIM] = 1.0, 1.0                      # unit 0 = mean, unit 1 = 1
    sat[2 * D:2 * D + 6] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]  # layer 2: the same two values
    sat[2 * D + 6:] = [-4000.0, 2000.0, 0.0]
    out["saturated"] = dict(weights=sat, n1=2, n2=2)
    # three members behind the distributor: rescaled column STUB below the threshold -> 0, else the bias column (1.0) below it -> 1
    # (never, with a threshold below 1) else 2; and with the dimensions exchanged members 1 and 2
    mn2, mx2 = minmax(rng)
    thr = _mlpdef.rescale(np.array([0.45]), mn2[STUB], mx2[STUB])[0]
    ws = [one_column_weights(rng, 10, 10) for _ in range(3)]
    out["ensemble 0/2"] = dict(weights=ws, n1=10, n2=10, mn=mn2, mx=mx2, dist=(float(DIM), float(STUB), float(thr)))
    out["ensemble 1/2"] = dict(weights=ws, n1=10, n2=10, mn=mn2, mx=mx2, dist=(float(STUB), float(DIM), float(thr)))
    for m in out.values():
        for k in ("mn", "mx", "dist"):
            m.setdefault(k, None)
    return out


def picks(model, mean):
    """the members the means reach"""
    rows = np.zeros((np.size(mean), DIM))
    rows[:, STUB] = np.ravel(mean)
    return _mlpdef.logits(model["weights"], model["n1"], model["n2"], rows, model["mn"], model["mx"], model["dist"], want_pick=True)[1]
