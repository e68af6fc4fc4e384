"""The MLP / logsig predictors' arithmetic written a second time, for the tests of glia_amd/csrc/mlp_model.hpp and
mlp_predict.hip.  NumPy form: whole columns, `acc = acc + x[:, j] * w[j, :]` for j ascending -- elementwise IEEE operations, a multiply and
an add rounded separately.  Step 7 goes through math.exp row by row: the process's own libm (np.exp may use NumPy's vector routine).
A literal pure-Python triple loop stands beside it and checks the NumPy form on a handful of rows."""
import math

import numpy as np

FEPS = 2.22e-16


def n_weights(dim, n1, n2):
    D = dim + 1
    return D * n1 + (n1 + 1) * n2 + n2 + 1 if n1 else D


def rescale(x, mn, mx):
    """stats::rescale(x, minmax, -1, 1) (util/stats.hxx:265-277) on an [n, dim] array"""
    with np.errstate(all="ignore"):
        return ((2.0 * (x - mn)) / ((mx - mn) + FEPS)) + (-1.0)


def prepare(rows, mn=None, mx=None):
    """steps 1 and 2: the rescaled rows with the 1.0 appended, [n, dim + 1]"""
    rows = np.asarray(rows, np.float64)
    x = rescale(rows, np.asarray(mn, np.float64)[:rows.shape[1]], np.asarray(mx, np.float64)[:rows.shape[1]]) if mn is not None else rows
    return np.concatenate([x, np.ones((rows.shape[0], 1))], axis=1)


def pick(x, dist):
    """step 3 on prepared rows: opt::ThresholdModelDistributor(dim0, dim1, thr) (type/function.hxx:80-84); a NaN compares false"""
    if dist is None:
        return np.zeros(x.shape[0], np.int64)
    d0, d1, thr = int(dist[0]), int(dist[1]), float(dist[2])
    with np.errstate(all="ignore"):
        return np.where(x[:, d1] < thr, 0, np.where(x[:, d0] < thr, 1, 2)).astype(np.int64)


def _dense(x, w):
    """x [n, din], w [din, nout] -> the chains sum_j x[:, j] * w[j, k], j ascending from 0.0"""
    acc = np.zeros((x.shape[0], w.shape[1]))
    with np.errstate(all="ignore"):
        for j in range(x.shape[1]):
            acc = acc + x[:, j:j + 1] * w[j:j + 1, :]
    return acc


def _relu1(h):
    with np.errstate(all="ignore"):
        a = np.where(h > 0.0, h, 0.0)
    return np.concatenate([a, np.ones((h.shape[0], 1))], axis=1)


def split(w, dim, n1, n2):
    """the column-major matrices of a model's weights as [din, nout] arrays"""
    D = dim + 1
    w = np.asarray(w, np.float64)
    assert w.size == n_weights(dim, n1, n2)
    if n1 == 0:
        return (w.reshape(D, 1),)
    o1 = D * n1
    o2 = o1 + (n1 + 1) * n2
    return w[:o1].reshape(n1, D).T, w[o1:o2].reshape(n2, n1 + 1).T, w[o2:].reshape(n2 + 1, 1)


def logits_prepared(x, w, n1, n2):
    mats = split(w, x.shape[1] - 1, n1, n2)
    if n1 == 0:
        return _dense(x, mats[0])[:, 0]
    a1 = _relu1(_dense(x, mats[0]))
    a2 = _relu1(_dense(a1, mats[1]))
    return _dense(a2, mats[2])[:, 0]


def logits(weights, n1, n2, rows, mn=None, mx=None, dist=None, want_pick=False):
    """steps 1-6; weights: one array or a list of three"""
    if isinstance(weights, np.ndarray):
        weights = [weights]
    x = prepare(rows, mn, mx)
    m = pick(x, dist if len(weights) == 3 else None)
    out = np.zeros(x.shape[0])
    for i, w in enumerate(weights):
        sel = m == i
        if sel.any():
            out[sel] = logits_prepared(x[sel], w, n1, n2)
    return (out, m) if want_pick else out


def _exp(v):
    try:
        return math.exp(v)
    except OverflowError:        # C's exp returns +inf
        return math.inf


def sigmoid(h3):
    """step 7 with the process's libm, one row at a time"""
    return np.array([1.0 / (1.0 + _exp(-float(h))) for h in np.asarray(h3, np.float64)], np.float64)


def triple_loop(weights, n1, n2, rows, mn=None, mx=None, dist=None):
    """the definition as literal loops over Python floats: logits of a handful of rows"""
    if isinstance(weights, np.ndarray):
        weights = [weights]
    rows = np.asarray(rows, np.float64)
    dim = rows.shape[1]
    D = dim + 1
    out = []
    for r in range(rows.shape[0]):
        x = []
        for j in range(dim):
            v = np.float64(rows[r, j])
            if mn is not None:
                with np.errstate(all="ignore"):      # np.float64 scalars: a division by 0.0 gives inf / NaN, not an exception
                    num = np.float64(2.0) * (v - np.float64(mn[j]))
                    den = (np.float64(mx[j]) - np.float64(mn[j])) + np.float64(FEPS)
                    v = (num / den) + np.float64(-1.0)
            x.append(float(v))
        x.append(1.0)
        m = 0
        if len(weights) == 3:
            m = 0 if x[int(dist[1])] < dist[2] else (1 if x[int(dist[0])] < dist[2] else 2)
        w = [float(v) for v in weights[m]]
        h3 = 0.0
        if n1 == 0:
            for j in range(D):
                h3 = h3 + x[j] * w[j]
        else:
            a1 = []
            for k in range(n1):
                h = 0.0
                for j in range(D):
                    h = h + x[j] * w[j + D * k]
                a1.append(h if h > 0.0 else 0.0)
            a1.append(1.0)
            o1 = D * n1
            a2 = []
            for k in range(n2):
                h = 0.0
                for j in range(n1 + 1):
                    h = h + a1[j] * w[o1 + j + (n1 + 1) * k]
                a2.append(h if h > 0.0 else 0.0)
            a2.append(1.0)
            o2 = o1 + (n1 + 1) * n2
            for j in range(n2 + 1):
                h3 = h3 + a2[j] * w[o2 + j]
        out.append(h3)
    return np.array(out, np.float64)


def same(a, b):
    """bit for bit (so -0.0 is not 0.0); NaN positions are compared as positions"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def write_values(path, values):
    """a model file: whitespace-separated doubles (readData(w, file, true))"""
    with open(path, "w") as f:
        f.write("\n".join("%.17g" % v for v in np.asarray(values, np.float64).ravel()) + "\n")


def write_rows(path, rows):
    """a feature or min/max file: one row per line"""
    with open(path, "w") as f:
        for r in rows:                         # (rows may differ in length)
            f.write(" ".join("%.17g" % v for v in r) + "\n")


# ---- shared cases ----
SIZES = [(1, 1, 1), (7, 3, 17), (104, 10, 10), (104, 17, 3), (33, 64, 33), (1, 0, 0), (104, 0, 0)]      # (dim, N1, N2); 0, 0: logsig
DIST = (3.0, 1.0, 0.0)      # columns 3 and 1 have zero mean, rescaled or not: rows reach all three models (dim >= 4)


def random_case(dim, n1, n2, n_rows=257, n_models=1, seed=0):
    """weights (one array or three), rows, min/max table -- all read-only"""
    rng = np.random.default_rng([dim, n1, n2, n_models, seed])
    ws = [rng.standard_normal(n_weights(dim, n1, n2)) * 0.5 for _ in range(n_models)]
    rows = rng.standard_normal((n_rows, dim)) * 2.0
    mn = -3.0 - rng.random(dim)
    mx = 3.0 + rng.random(dim)
    mx[::5] = mn[::5]                     # max == min: the denominator is FEPS
    if dim > 2:
        mn[2], mx[2] = mx[2], mn[2]       # a table the wrong way round: a negative denominator
    rows[0, :] = mn                       # on the lower bounds
    if n_rows > 1:
        rows[1, :] = mx                   # on the upper bounds
    for a in ws + [rows, mn, mx]:
        a.setflags(write=False)
    return (ws[0] if n_models == 1 else ws), rows, mn, mx


def special_cases():
    """(name, weights, n1, n2, rows): NaN, +-inf and -0.0 inputs; hidden sums of exactly 0.0, also from -0.0 products (a chain starts at
    +0.0, so it cannot end at -0.0: 0.0 + -0.0 = 0.0); logits of +-inf (probability exactly 1 / 0) and NaN"""
    inf, nan = np.inf, np.nan
    rows = np.array([[3.0, 3.0], [-0.0, 0.0], [-0.0, -0.0], [1e308, 1e308], [1e308, -1e308], [inf, 0.0], [inf, inf], [-inf, 5.0], [nan, 1.0],
                     [1.0, nan], [0.5, -0.25], [-1e308, 1e308], [0.0, 1e308]])
    # layer 1: units x0 - x1, x0 + x1; layer 2: units a1_1 - a1_0, a1_0 + 0.5; output 1e308 * a2_0 - 1e308 * a2_1
    mlp_a = np.array([1.0, -1.0, 0.0, 1.0, 1.0, 0.0, -1.0, 1.0, 0.0, 1.0, 0.0, 0.5, 1e308, -1e308, 0.0])
    mlp_b = mlp_a.copy()
    mlp_b[12:] = [inf, 1.0, -2.0]         # 0 * inf in the output chain
    logsig = np.array([1e308, -1e308, 0.0])
    return [("mlp_a", mlp_a, 2, 2, rows), ("mlp_b", mlp_b, 2, 2, rows), ("logsig", logsig, 0, 0, rows)]
