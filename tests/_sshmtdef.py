"""The merge-path (unsupervised) term of train_sshmt_mlp / train_sshmt_logsig written a second time, for the tests of
glia_amd/csrc/sshmt_paths.hpp and sshmt_train.hip.  Restated from the reference's text (hmt/tree_build.hxx:150-180, alg/dnf.hxx:126-326,
sshmt/input.hxx:11-60,115-124, sshmt/sshmt_util.hxx:140-222, type/energy_function.hxx:164-230) and the definition; nothing is imported
from the library.  The forward / backward pass of a row and the optimiser's constants are _mlptraindef's; the per-path arithmetic is a
literal loop over Python floats (IEEE doubles, every operation rounded on its own), the reductions are explicit loops."""
import math

import numpy as np

import _mlpdef as D
import _mlptraindef as T

MAX_PATH = 8                # kSshmtMaxPath
PATH_CHUNK = 64             # kSshmtPathChunk: part of the definition
CHUNK = T.CHUNK
FEPS = T.FEPS

DEFAULTS = dict(T.DEFAULTS, wu=0.0, update_sigma_u=0, sigma_u=0.0, merge_target=0.95, path_target=1.0, max_path_length=3, min_path_length=2)


def merge_paths(order, max_len=3, min_len=2):
    """the bounded genMergePaths: a list of lists of merge indices, bottom-up, by ascending first member"""
    order = [tuple(int(v) for v in m) for m in np.asarray(order).reshape(-1, 3)]
    child_of, created = {}, {}
    for i, (a, b, c) in enumerate(order):
        child_of[a] = i
        child_of[b] = i
        created[c] = i
    out = []
    for i, (a, b, c) in enumerate(order):
        path = [i]
        nxt = child_of.get(c)
        while nxt is not None and len(path) < max_len:
            path.append(nxt)
            nxt = child_of.get(order[nxt][2])
        if len(path) == max_len or (len(path) >= min_len and a not in created and b not in created):
            out.append(path)
    return out


def path_terms(f, Tn, tn, want_q=True):
    """one path with outputs f: (D, e, a) -- a_i = dD/df_i, or None"""
    n = len(f)
    u = [1.0 - v for v in f]

    def x(k, j):
        return f[k] if k < j else u[k]

    F = []
    for j in range(n + 1):
        c = 1.0
        for i in range(n):
            c = c * x(i, j)
        F.append(Tn - c)
    prod = 1.0
    for j in range(n + 1):
        prod = prod * F[j]
    Dp = 1.0 - prod
    e = tn - Dp
    if not want_q:
        return Dp, e, None
    EC = []
    for j in range(n + 1):
        c = 1.0
        for k in range(n + 1):
            if k != j:
                c = c * F[k]
        EC.append(c)
    a = []
    for i in range(n):
        acc = 0.0
        for j in range(n + 1):
            m = 1.0
            for k in range(n):
                if k != i:
                    m = m * x(k, j)
            acc = acc + EC[j] * (-m if j <= i else m)
        a.append(acc)
    return Dp, e, a


class Uns:
    """the unlabelled blocks as the term sees them: prepared rows of all blocks, paths with members offset by the rows before"""

    def __init__(self, blocks, mn, mx, max_len, min_len, merge_target, path_target):
        Xs, self.paths = [], []
        row0 = 0
        for rows, order in blocks:
            rows = np.asarray(rows, np.float64)
            self.paths += [[row0 + i for i in p] for p in merge_paths(order, max_len, min_len)]
            Xs.append(D.prepare(rows, mn, mx))
            row0 += rows.shape[0]
        self.X = np.concatenate(Xs, axis=0) if Xs else np.zeros((0, 1))
        self.N = row0
        self.P = len(self.paths)
        self.Tn = [1.0] + [math.pow(merge_target, n) for n in range(1, MAX_PATH + 1)]
        self.tn = [1.0] + [math.pow(path_target, n) for n in range(1, MAX_PATH + 1)]
        self.inc = [[] for _ in range(self.N)]
        for p, path in enumerate(self.paths):
            for slot, r in enumerate(path):
                self.inc[r].append((p, slot))


def uns_loss_grad(w, n1, n2, U, want_grad=True):
    """L_U = sum e_p^2 over chunks of 64 paths; grad_U = -sum_r c_r g_r over chunks of 64 rows"""
    with np.errstate(all="ignore"):
        if want_grad:
            f, G = T.row_gradients(w, n1, n2, U.X)
        else:
            f = T.forward(w, n1, n2, U.X)
        f = [float(v) for v in f]
        es, qs = [], []
        L = 0.0
        for p0 in range(0, U.P, PATH_CHUNK):
            Lc = 0.0
            for p in range(p0, min(U.P, p0 + PATH_CHUNK)):
                path = U.paths[p]
                n = len(path)
                _, e, a = path_terms([f[r] for r in path], U.Tn[n], U.tn[n], want_grad)
                es.append(e)
                qs.append([e * ai for ai in a] if want_grad else None)
                Lc = Lc + e * e
            L = L + Lc
        if not want_grad:
            return L, None
        d = np.asarray(w).size
        grad = np.zeros(d)
        for r0 in range(0, U.N, CHUNK):
            S = np.zeros(d)
            for r in range(r0, min(U.N, r0 + CHUNK)):
                c, named = 0.0, False
                for p, slot in U.inc[r]:
                    if abs(es[p]) < FEPS:
                        continue
                    c = c + qs[p][slot]
                    named = True
                if named:
                    S = S - G[r] * c
            grad = grad + S
        return L, grad


class Energy:
    """fx = wr |w|^2 / 2 + wu (0.5 L_U / su^2 + P log(su^2) / 2) + ws (0.5 L / ss^2 + n log(ss^2) / 2), the terms in this order"""

    def __init__(self, n1, n2, X, t, U, wr, wu, ws, sigma2, sigma_u2):
        self.n1, self.n2, self.X, self.t, self.U = n1, n2, X, t, U
        self.wr, self.wu, self.ws, self.sigma2, self.sigma_u2 = wr, wu, ws, sigma2, sigma_u2
        self.use_r, self.use_s = not T._isfeq(wr, 0.0), not T._isfeq(ws, 0.0)
        self.use_u = not T._isfeq(wu, 0.0) and U.P > 0

    def __call__(self, w, want_grad):
        with np.errstate(all="ignore"):
            ret = 0.0
            g = np.zeros(w.size) if want_grad else None
            if self.use_r:
                ret = ret + self.wr * (T._sqnorm(w) / 2.0)
                if want_grad:
                    g = g + (w if T._isfeq(self.wr, 1.0) else self.wr * w)
            for use, wt, s2, cnt, fn in ((self.use_u, self.wu, self.sigma_u2, self.U.P, lambda: uns_loss_grad(w, self.n1, self.n2, self.U, want_grad)),
                                         (self.use_s, self.ws, self.sigma2, self.X.shape[0],
                                          lambda: T.loss_grad(w, self.n1, self.n2, self.X, self.t, want_grad))):
                if not use:
                    continue
                L, grad = fn()
                s2 = np.float64(s2)
                ret = ret + wt * float(np.float64(0.5 * L) / s2 + np.float64(float(cnt) * T._log(float(s2))) / 2.0)
                if want_grad:
                    tt = grad / s2
                    g = g + (tt if T._isfeq(wt, 1.0) else wt * tt)
            return float(ret), g


def train(rows, labels, unlabelled, n1, n2, minmax=None, init=None, **opts):
    """-> dict(round_w, trace, sigma2, sigma2_eval, sigma_u2, sigma_u2_eval, stopped_nonfinite, n_paths, n_uns_rows); the optimiser is
    _mlptraindef.train's, restated around the three-term energy"""
    o = dict(DEFAULTS)
    o.update(opts)
    mn, mx = minmax if minmax is not None else (None, None)
    U = Uns(unlabelled, mn, mx, o["max_path_length"], o["min_path_length"], o["merge_target"], o["path_target"])
    dim = np.asarray(rows).shape[1] if rows is not None else U.X.shape[1] - 1
    if rows is None:
        rows, labels = np.zeros((0, dim)), np.zeros(0, np.int32)
    X, t = T.prepare(rows, labels, mn, mx, o["pos_target"], o["neg_target"])
    n = X.shape[0]
    d = D.n_weights(dim, n1, n2)
    w = np.array(init, np.float64) if init is not None else T.init_weights(o["seed"], d) if n1 else np.zeros(d)
    E = Energy(n1, n2, X, t, U, o["wr"], o["wu"], o["ws"], o["sigma_s"] * o["sigma_s"], o["sigma_u"] * o["sigma_u"])
    R = dict(round_w=[], trace=[], sigma2=[], sigma2_eval=[], sigma_u2=[], sigma_u2_eval=[], stopped_nonfinite=False, n_paths=U.P, n_uns_rows=U.N)
    opt = o["optimizer"]
    _max, _isfeq, _sqnorm, _sqrt, _finite = T._max, T._isfeq, T._sqnorm, T._sqrt, T._finite

    def update_sigma():
        if not E.use_s:
            R["sigma2"].append(E.sigma2); R["sigma2_eval"].append(0.0)
        else:
            L, _ = T.loss_grad(w, n1, n2, X, t, False)
            with np.errstate(all="ignore"):
                v = float(np.float64(L) / np.float64(float(n)))
            if o["update_sigma_s"]:
                E.sigma2 = _max(o["min_sigma2"], v)
            R["sigma2"].append(E.sigma2)
            R["sigma2_eval"].append(E.sigma2 if o["update_sigma_s"] and E.sigma2 != o["min_sigma2"] else _max(0.0, v))
        if not E.use_u:
            R["sigma_u2"].append(E.sigma_u2); R["sigma_u2_eval"].append(0.0)
        else:
            L, _ = uns_loss_grad(w, n1, n2, U, False)
            with np.errstate(all="ignore"):
                v = float(np.float64(L) / np.float64(float(U.P)))
            if o["update_sigma_u"]:
                E.sigma_u2 = _max(o["min_sigma2"], v)
            R["sigma_u2"].append(E.sigma_u2)
            R["sigma_u2_eval"].append(E.sigma_u2 if o["update_sigma_u"] else _max(0.0, v))

    state = {}

    def update(w, g, step):
        with np.errstate(all="ignore"):
            if opt == 1:
                return w - g * step
            if opt == 3:
                u = g + T.MU * state["v"]
                state["v"] = u
                return w - step * u
            state["m"] = T.BETA1 * state["m"] + (1.0 - T.BETA1) * g
            state["v"] = T.BETA2 * state["v"] + ((1.0 - T.BETA2) * g) * g
            return w - (step * state["m"]) / np.sqrt(state["v"] + T.ADAM_EPS)

    def rec(rnd, it, kind, fx, xx, gg, step, rb):
        R["trace"].append((fx, _sqrt(xx), _sqrt(gg), step, E.sigma2, rnd, it, kind, rb))

    def stop(rnd, it, fx, xx, gg, step, rb, backup):
        rec(rnd, it, 2, fx, xx, gg, step, rb)
        R["stopped_nonfinite"] = True
        return backup if backup is not None else w

    cur_step = o["step"]
    update_sigma()
    for rnd in range(o["n_sigma_updates"]):
        per = o["sigma_update_step_period"]
        if per > 0 and rnd > 0 and rnd % per == 0:
            cur_step = _max(cur_step * 0.5, T.MIN_STEP)
        Tmax = o["max_iterations"]
        if Tmax > 0:
            state["m"] = np.zeros(d); state["v"] = np.zeros(d)
            backup = None
            step = cur_step
            it = 0
            fx = gg = 0.0
            if _isfeq(o["step_decay"], 1.0):
                while it <= Tmax:
                    last = it == Tmax
                    fsdi = o["fixed_step_decay_iterations"]
                    if not last and fsdi > 0 and it > 0 and it % fsdi == 0:
                        step = _max(T.MIN_STEP, step * T.FIXED_DECAY)
                    fx, g = E(w, True)
                    gg, xx = _sqnorm(g), _sqnorm(w)
                    if not _finite(fx) or not _finite(gg):
                        w = stop(rnd, it, fx, xx, gg, step, 0, backup)
                        break
                    rec(rnd, it, 1 if last else 0, fx, xx, gg, step, 0)
                    if last:
                        break
                    if _sqrt(gg) < T.GRAD_TOL:
                        it = Tmax
                        continue
                    backup = w
                    w = update(w, g, step)
                    it += 1
            else:
                while it < Tmax:
                    fx, g = E(w, True)
                    gg, xx = _sqnorm(g), _sqnorm(w)
                    if not _finite(fx) or not _finite(gg):
                        w = stop(rnd, it, fx, xx, gg, step, 0, backup)
                        break
                    if _sqrt(gg) < T.GRAD_TOL:
                        break
                    backup = w
                    w = update(w, g, step)
                    fx_prev = fx
                    rb = 0
                    fx, _ = E(w, False)
                    while step > T.MIN_STEP and fx >= fx_prev:
                        step = _max(T.MIN_STEP, step * o["step_decay"])
                        if step == T.MIN_STEP:
                            break
                        w = update(backup, g, step)
                        fx, _ = E(w, False)
                        rb += 1
                    rec(rnd, it, 0, fx_prev, xx, gg, step, rb)
                    if not _finite(fx):
                        w = stop(rnd, it, fx, xx, gg, step, rb, backup)
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
