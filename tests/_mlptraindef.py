"""The MLP / logsig trainer's arithmetic written a second time, for the tests of glia_amd/csrc/mlp_backward.hpp and
mlp_train.hip.  Restated from the reference's text (alg/nn.hxx:73-107, alg/function.hxx:36-40,171-209,257-267,
type/energy_function.hxx:164-230, alg/gd.hxx, sshmt/sshmt_util.hxx:140-207, sshmt/main_train_sshmt_mlp.cxx:133-166) and the definition;
nothing is imported from the library.  NumPy form: whole columns per operation (elementwise IEEE operations, a multiply and an add
rounded separately), math.exp row by row, the 64-row chunks of the gradient's reduction as an explicit loop.  A literal pure-Python
loop over a handful of rows and weights stands beside it (literal_grad)."""
import math

import numpy as np

import _mlpdef as D

CHUNK = 64                  # kMlpTrainChunk: part of the definition
FEPS = 2.22e-16
MIN_STEP, GRAD_TOL, FIXED_DECAY = 1e-10, 1e-16, 0.5
MU, BETA1, BETA2, ADAM_EPS = 0.5, 0.5, 0.9, 1e-8
M64 = (1 << 64) - 1

DEFAULTS = dict(wr=0.0, ws=0.0, sigma_s=0.0, update_sigma_s=0, optimizer=1, step=0.0, step_decay=1.0, fixed_step_decay_iterations=-1,
                sigma_update_step_period=-1, max_iterations=0, n_sigma_updates=0, pos_target=0.05, neg_target=0.95, min_sigma2=0.0, seed=0)


def _mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def init_weights(seed, n):
    """Gaussian(0, 0.01) by Irwin-Hall from splitmix64 keyed by (seed, p)"""
    out = []
    for p in range(n):
        h = _mix(_mix(seed) ^ p)
        s = 0.0
        for k in range(12):
            s = s + float(_mix(h ^ (k + 1)) >> 11) * 2.0 ** -53
        out.append((s - 6.0) * 0.01)
    return np.array(out, np.float64)


def prepare(rows, labels, mn=None, mx=None, pos_target=0.05, neg_target=0.95):
    """rows with label +1 / -1 in input order, rescaled, a 1.0 appended; their targets"""
    rows = np.asarray(rows, np.float64)
    labels = np.asarray(labels).reshape(-1)
    keep = (labels == 1) | (labels == -1)
    X = D.prepare(rows[keep], mn, mx)
    t = np.where(labels[keep] == 1, pos_target, neg_target).astype(np.float64)
    return X, t


def row_gradients(w, n1, n2, X):
    """f [n] and the per-row gradients G [n, d] (column p = weight p of the model file)"""
    n, Dd = X.shape
    mats = D.split(w, Dd - 1, n1, n2)
    with np.errstate(all="ignore"):
        if n1 == 0:
            f = D.sigmoid(D._dense(X, mats[0])[:, 0])
            dh3 = f * (1.0 - f)
            return f, dh3[:, None] * X
        W0, W1, W2 = mats
        h1 = D._dense(X, W0)
        a1 = D._relu1(h1)
        h2 = D._dense(a1, W1)
        a2 = D._relu1(h2)
        f = D.sigmoid(D._dense(a2, W2)[:, 0])
        dh3 = f * (1.0 - f)
        dh2 = np.where(h2 <= 0.0, 0.0, dh3[:, None] * W2[:n2, 0][None, :])
        acc = np.zeros((n, n1))
        for k in range(n2):
            acc = acc + dh2[:, k:k + 1] * W1[:n1, k][None, :]
        dh1 = np.where(h1 <= 0.0, 0.0, acc)
        G0 = (dh1[:, :, None] * X[:, None, :]).reshape(n, n1 * Dd)                 # p = j + D * k
        G1 = (dh2[:, :, None] * a1[:, None, :]).reshape(n, n2 * (n1 + 1))          # p = j + (n1 + 1) * k
        G2 = a2 * dh3[:, None]
        return f, np.concatenate([G0, G1, G2], axis=1)


def forward(w, n1, n2, X):
    with np.errstate(all="ignore"):
        return D.sigmoid(D.logits_prepared(X, w, n1, n2))


def loss_grad(w, n1, n2, X, t, want_grad=True):
    """L = sum e^2 and grad = -sum g_i e_i in the two-level order: chunk sums over rows ascending, then over chunks ascending"""
    n = X.shape[0]
    with np.errstate(all="ignore"):
        if want_grad:
            f, G = row_gradients(w, n1, n2, X)
        else:
            f = forward(w, n1, n2, X)
        e = t - f
        ee = e * e
        L = 0.0
        grad = np.zeros(np.asarray(w).size) if want_grad else None
        if want_grad:
            T = G * e[:, None]
        for r0 in range(0, n, CHUNK):
            Lc = 0.0
            S = np.zeros(np.asarray(w).size) if want_grad else None
            for r in range(r0, min(n, r0 + CHUNK)):
                Lc = Lc + float(ee[r])
                if want_grad and not abs(float(e[r])) < FEPS:
                    S = S - T[r]
            L = L + Lc
            if want_grad:
                grad = grad + S
    return L, grad


def literal_grad(w, n1, n2, X, t, ps):
    """the definition as literal loops over Python floats: gradient elements ps (and L) over all rows"""
    w = [float(v) for v in np.asarray(w)]
    n, Dd = X.shape
    o1 = Dd * n1
    o2 = o1 + (n1 + 1) * n2
    per_row = []
    for r in range(n):
        x = [float(v) for v in X[r]]
        if n1 == 0:
            h3 = 0.0
            for j in range(Dd):
                h3 = h3 + x[j] * w[j]
            h1 = h2 = a1 = a2 = dh1 = dh2 = []
        else:
            h1 = []
            for k in range(n1):
                h = 0.0
                for j in range(Dd):
                    h = h + x[j] * w[j + Dd * k]
                h1.append(h)
            a1 = [h if h > 0.0 else 0.0 for h in h1] + [1.0]
            h2 = []
            for k in range(n2):
                h = 0.0
                for j in range(n1 + 1):
                    h = h + a1[j] * w[o1 + j + (n1 + 1) * k]
                h2.append(h)
            a2 = [h if h > 0.0 else 0.0 for h in h2] + [1.0]
            h3 = 0.0
            for j in range(n2 + 1):
                h3 = h3 + a2[j] * w[o2 + j]
        f = 1.0 / (1.0 + D._exp(-h3))
        dh3 = f * (1.0 - f)
        if n1:
            dh2 = [0.0 if h2[k] <= 0.0 else dh3 * w[o2 + k] for k in range(n2)]
            dh1 = []
            for j in range(n1):
                acc = 0.0
                for k in range(n2):
                    acc = acc + dh2[k] * w[o1 + j + (n1 + 1) * k]
                dh1.append(0.0 if h1[j] <= 0.0 else acc)
        per_row.append((x, a1, a2, dh1, dh2, dh3, float(t[r]) - f))

    def g_elem(row, p):
        x, a1, a2, dh1, dh2, dh3, _ = row
        if n1 == 0:
            return dh3 * x[p]
        if p < o1:
            return x[p % Dd] * dh1[p // Dd]
        if p < o2:
            q = p - o1
            return a1[q % (n1 + 1)] * dh2[q // (n1 + 1)]
        return a2[p - o2] * dh3

    out = []
    for p in ps:
        grad = 0.0
        for r0 in range(0, n, CHUNK):
            S = 0.0
            for r in range(r0, min(n, r0 + CHUNK)):
                e = per_row[r][6]
                if not abs(e) < FEPS:
                    S = S - g_elem(per_row[r], p) * e
            grad = grad + S
        out.append(grad)
    L = 0.0
    for r0 in range(0, n, CHUNK):
        Lc = 0.0
        for r in range(r0, min(n, r0 + CHUNK)):
            Lc = Lc + per_row[r][6] * per_row[r][6]
        L = L + Lc
    return L, np.array(out, np.float64)


def _isfeq(a, b):
    return abs(a - b) < FEPS


def _max(a, b):
    """std::max(a, b)"""
    return b if a < b else a


def _sqnorm(v):
    s = 0.0
    with np.errstate(all="ignore"):
        sq = (v * v).tolist()
    for x in sq:
        s = s + x
    return s


def _log(v):
    if v == 0.0:
        return -math.inf
    if v < 0.0 or v != v:
        return math.nan
    return math.log(v)


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else math.nan


def _finite(v):
    return math.isfinite(v)


class Energy:
    """fx = wr |w|^2 / 2 + ws (0.5 L / sigma^2 + n log(sigma^2) / 2); g = wr w + ws grad / sigma^2 (a term whose weight isfeq 0 is off)"""

    def __init__(self, n1, n2, X, t, wr, ws, sigma2):
        self.n1, self.n2, self.X, self.t, self.wr, self.ws, self.sigma2 = n1, n2, X, t, wr, ws, sigma2
        self.use_r, self.use_s = not _isfeq(wr, 0.0), not _isfeq(ws, 0.0)

    def __call__(self, w, want_grad):
        with np.errstate(all="ignore"):
            n = self.X.shape[0]
            ret = 0.0
            g = np.zeros(w.size) if want_grad else None
            if self.use_r:
                ret = ret + self.wr * (_sqnorm(w) / 2.0)
                if want_grad:
                    g = g + (w if _isfeq(self.wr, 1.0) else self.wr * w)
            if self.use_s:
                L, grad = loss_grad(w, self.n1, self.n2, self.X, self.t, want_grad)
                s2 = np.float64(self.sigma2)
                ret = ret + self.ws * float(np.float64(0.5 * L) / s2 + np.float64(float(n) * _log(self.sigma2)) / 2.0)
                if want_grad:
                    tt = grad / s2
                    g = g + (tt if _isfeq(self.ws, 1.0) else self.ws * tt)
            return float(ret), g


def train(rows, labels, n1, n2, minmax=None, init=None, **opts):
    """-> dict(round_w, trace, sigma2, sigma2_eval, stopped_nonfinite); trace records are tuples
    (fx, xnorm, gnorm, step, sigma2, round, t, kind, rollbacks)"""
    o = dict(DEFAULTS)
    o.update(opts)
    mn, mx = minmax if minmax is not None else (None, None)
    X, t = prepare(rows, labels, mn, mx, o["pos_target"], o["neg_target"])
    n, Dd = X.shape
    d = D.n_weights(Dd - 1, n1, n2)
    if init is not None:
        w = np.array(init, np.float64)
    elif n1:
        w = init_weights(o["seed"], d)
    else:
        w = np.zeros(d)
    E = Energy(n1, n2, X, t, o["wr"], o["ws"], o["sigma_s"] * o["sigma_s"])
    R = dict(round_w=[], trace=[], sigma2=[], sigma2_eval=[], stopped_nonfinite=False)
    opt = o["optimizer"]

    def update_sigma():
        if not E.use_s:
            R["sigma2"].append(E.sigma2); R["sigma2_eval"].append(0.0)
            return
        L, _ = loss_grad(w, n1, n2, X, t, False)
        with np.errstate(all="ignore"):
            v = float(np.float64(L) / np.float64(float(n)))
        if o["update_sigma_s"]:
            E.sigma2 = _max(o["min_sigma2"], v)
        R["sigma2"].append(E.sigma2)
        R["sigma2_eval"].append(E.sigma2 if o["update_sigma_s"] and E.sigma2 != o["min_sigma2"] else _max(0.0, v))

    state = {}

    def update(w, g, step):
        with np.errstate(all="ignore"):
            if opt == 1:
                return w - g * step
            if opt == 3:
                u = g + MU * state["v"]
                state["v"] = u
                return w - step * u
            state["m"] = BETA1 * state["m"] + (1.0 - BETA1) * g
            state["v"] = BETA2 * state["v"] + ((1.0 - BETA2) * g) * g
            return w - (step * state["m"]) / np.sqrt(state["v"] + ADAM_EPS)

    def rec(rnd, it, kind, fx, xx, gg, step, rb):
        R["trace"].append((fx, _sqrt(xx), _sqrt(gg), step, E.sigma2, rnd, it, kind, rb))

    cur_step = o["step"]
    update_sigma()
    for rnd in range(o["n_sigma_updates"]):
        per = o["sigma_update_step_period"]
        if per > 0 and rnd > 0 and rnd % per == 0:
            cur_step = _max(cur_step * 0.5, MIN_STEP)
        T = o["max_iterations"]
        if T > 0:
            state["m"] = np.zeros(d); state["v"] = np.zeros(d)
            backup = None
            step = cur_step
            if _isfeq(o["step_decay"], 1.0):
                it = 0
                while it <= T:
                    last = it == T
                    fsdi = o["fixed_step_decay_iterations"]
                    if not last and fsdi > 0 and it > 0 and it % fsdi == 0:
                        step = _max(MIN_STEP, step * FIXED_DECAY)
                    fx, g = E(w, True)
                    gg, xx = _sqnorm(g), _sqnorm(w)
                    if not _finite(fx) or not _finite(gg):
                        rec(rnd, it, 2, fx, xx, gg, step, 0)
                        if backup is not None:
                            w = backup
                        R["stopped_nonfinite"] = True
                        break
                    rec(rnd, it, 1 if last else 0, fx, xx, gg, step, 0)
                    if last:
                        break
                    if _sqrt(gg) < GRAD_TOL:
                        it = T
                        continue
                    backup = w
                    w = update(w, g, step)
                    it += 1
            else:
                it = 0
                fx = gg = 0.0
                while it < T:
                    fx, g = E(w, True)
                    gg, xx = _sqnorm(g), _sqnorm(w)
                    if not _finite(fx) or not _finite(gg):
                        rec(rnd, it, 2, fx, xx, gg, step, 0)
                        if backup is not None:
                            w = backup
                        R["stopped_nonfinite"] = True
                        break
                    if _sqrt(gg) < GRAD_TOL:
                        break
                    backup = w
                    w = update(w, g, step)
                    fx_prev = fx
                    rb = 0
                    fx, _ = E(w, False)
                    while step > MIN_STEP and fx >= fx_prev:
                        step = _max(MIN_STEP, step * o["step_decay"])
                        if step == MIN_STEP:
                            break
                        w = update(backup, g, step)
                        fx, _ = E(w, False)
                        rb += 1
                    rec(rnd, it, 0, fx_prev, xx, gg, step, rb)
                    if not _finite(fx):
                        rec(rnd, it, 2, fx, xx, gg, step, rb)
                        w = backup
                        R["stopped_nonfinite"] = True
                        break
                    it += 1
                if not R["stopped_nonfinite"]:
                    rec(rnd, it, 1, fx, _sqnorm(w), gg, step, 0)
        R["round_w"].append(np.array(w))
        if R["stopped_nonfinite"]:
            break
        update_sigma()
    if not R["round_w"]:
        R["round_w"].append(np.array(w))
    return R
