"""The second author of train_forest's out-of-bag outputs: the definition of DESIGN 3.16 restated in plain NumPy / Python on top of
_rfdef (the growing rule, untouched), with no library call.  Every integer array the device trainer returns must equal what this file
computes and every double must have the same bits (tests/test_gpu_forest_oob.py); tests/test_rf_oob_definition.py holds this file to
cases worked out by hand.

Nothing here skips a walk: every out-of-bag row of every tree is walked once per column with that column permuted, whether or not the
row's path tests the column.  The device makes only the walks that can change a class; the results may not differ."""
import math

import numpy as np

import _rfdef
from _rfdef import DEFAULT_SEED, h, mix

A_PERM = 1 << 32          # h's second argument for the permutation of variable v is A_PERM + v


def perm_bits(m):
    """the smallest even number of bits >= 2 with 2^b >= m"""
    b = 2
    while (1 << b) < m:
        b += 2
    return b


def perm(seed, t, v, j, m, count_passes=None):
    """pi(j) of tree t and variable v over [0, m): four Feistel rounds on b bits, repeated until the value lies in [0, m)"""
    half = perm_bits(m) // 2
    mask = (1 << half) - 1
    K = [h(seed, t, A_PERM + v, r) for r in range(4)]
    x = j
    passes = 0
    while True:
        L, R = x >> half, x & mask
        for r in range(4):
            L, R = R, L ^ (mix(K[r] ^ R) & mask)
        x = (L << half) | R
        passes += 1
        if x < m:
            if count_passes is not None:
                count_passes.append(passes)
            return x


def perm_all(seed, t, v, m):
    """[pi(0), ..., pi(m - 1)] -- the same function on NumPy integers"""
    half = np.uint64(perm_bits(m) // 2)
    mask = np.uint64((1 << int(half)) - 1)
    K = [np.uint64(h(seed, t, A_PERM + v, r)) for r in range(4)]
    x = np.arange(m, dtype=np.uint64)
    todo = np.ones(m, bool)
    while todo.any():
        L, R = x[todo] >> half, x[todo] & mask
        for r in range(4):
            L, R = R, L ^ (_rfdef._mix_np(K[r] ^ R) & mask)
        x[todo] = (L << half) | R
        todo &= x >= np.uint64(m)
    return x.astype(np.int64)


def classes(model, t, rows):
    """0-based class of the terminal node every row of `rows` reaches in tree t (left iff x[var] <= split), and that node"""
    st, tm, bv, sp = model["nodestatus"][t], model["treemap"][t], model["bestvar"][t], model["xbestsplit"][t]
    at = np.zeros(len(rows), np.int64)
    while True:
        go = np.nonzero(st[at] == 1)[0]
        if len(go) == 0:
            break
        k = at[go]
        at[go] = tm[k, 0] - 1 + (~(rows[go, bv[k] - 1] <= sp[k])).astype(np.int64)
    return model["nodeclass"][t][at].astype(np.int64) - 1, at


def ratio(num, den):
    return 0.0 if den == 0 else float(np.float64(int(num)) / np.float64(int(den)))


def gini_of(w, n):
    num = 0.0
    den = 0.0
    for k in range(len(w)):
        t = float(w[k]) * float(int(n[k]))
        num = num + t * t
        den = den + t
    return num / den


def node_counts(model, t, X, cls, mult, nclass):
    """in-bag class counts (multiplicity weighted) of every node of tree t: a row counts in every node its walk passes"""
    st, tm, bv, sp = model["nodestatus"][t], model["treemap"][t], model["bestvar"][t], model["xbestsplit"][t]
    cnt = np.zeros((int(model["ndbigtree"][t]), nclass), np.int64)
    for i in np.nonzero(mult)[0]:
        k = 0
        while True:
            cnt[k, cls[i]] += mult[i]
            if st[k] != 1:
                break
            k = int(tm[k, 0 if X[i, bv[k] - 1] <= sp[k] else 1]) - 1
    return cnt


def oob(X, y, model=None, ntree=255, mtry=0, sample_ratio=0.7, nodesize=1, balance=1, max_depth=0, seed=DEFAULT_SEED, importance=True,
        details=None):
    """every out-of-bag output of train_forest(X, y, oob=True, importance=True, ...).  model: _rfdef.train's arrays for the same options
    (grown here when None).  details (a dict) receives the per-tree integers: m, n_k, r_k, d."""
    X = np.ascontiguousarray(X, np.float64)
    N, D = X.shape
    d = _rfdef.derive(y, D, mtry, sample_ratio, balance)
    if model is None:
        model = _rfdef.train(X, y, ntree, mtry, sample_ratio, nodesize, balance, max_depth, seed)
    cls, nclass, w = d["cls"], d["nclass"], d["classwt"]
    counttr = np.zeros((nclass, N), np.int32)
    err_wrong = np.zeros((ntree, nclass + 1), np.int64)
    err_seen = np.zeros((ntree, nclass + 1), np.int64)
    errtr = np.zeros((ntree, nclass + 1))
    s_sum = [[0.0] * (nclass + 1) for _ in range(D)]
    s_sq = [[0.0] * (nclass + 1) for _ in range(D)]
    gini = [0.0] * D
    per_tree = []
    for t in range(ntree):
        mult = _rfdef.bootstrap(seed, t, N, d["sampsize"])
        O = np.nonzero(mult == 0)[0]
        m = len(O)
        p, _ = classes(model, t, X[O])
        np.add.at(counttr, (p, O), 1)
        # the error over trees 0 .. t
        times = counttr.sum(axis=0)
        out = np.where(times > 0, counttr.argmax(axis=0) + 1, 0)            # argmax: the first of the largest = the lowest class
        seen = times > 0
        wrong = seen & (out - 1 != cls)
        for k in range(nclass):
            err_wrong[t, 1 + k] = int((wrong & (cls == k)).sum())
            err_seen[t, 1 + k] = int((seen & (cls == k)).sum())
        err_wrong[t, 0], err_seen[t, 0] = int(wrong.sum()), int(seen.sum())
        for c in range(nclass + 1):
            errtr[t, c] = ratio(err_wrong[t, c], err_seen[t, c])
        if not importance:
            continue
        # permutation importance
        n_k = [int((cls[O] == k).sum()) for k in range(nclass)]
        r_k = [int(((cls[O] == k) & (p == k)).sum()) for k in range(nclass)]
        dt = np.zeros((D, nclass), np.int64)
        tested = set(int(v) - 1 for v in model["bestvar"][t][: int(model["ndbigtree"][t])] if v > 0)
        for v in range(D):
            if m == 0 or v not in tested:                                  # by definition: no node tests v, d = 0
                continue
            pi = perm_all(seed, t, v, m)
            rows = X[O].copy()
            rows[:, v] = X[O[pi], v]
            p2, _ = classes(model, t, rows)
            for k in range(nclass):
                dt[v, k] = r_k[k] - int(((cls[O] == k) & (p2 == k)).sum())
        per_tree.append(dict(m=m, n_k=n_k, r_k=r_k, d=dt, oob=O, p=p))
        if m > 0:
            for v in range(D):
                d_all = 0
                for c in range(nclass + 1):
                    if c < nclass:
                        term = ratio(dt[v, c], n_k[c])
                        d_all += int(dt[v, c])
                    else:
                        term = ratio(d_all, m)
                    s_sum[v][c] = s_sum[v][c] + term
                    s_sq[v][c] = s_sq[v][c] + term * term
        # Gini
        cnt = node_counts(model, t, X, cls, mult, nclass)
        tm, st, bv = model["treemap"][t], model["nodestatus"][t], model["bestvar"][t]
        for q in range(int(model["ndbigtree"][t])):
            if st[q] == 1:
                dec = (gini_of(w, cnt[tm[q, 0] - 1]) + gini_of(w, cnt[tm[q, 1] - 1])) - gini_of(w, cnt[q])
                gini[bv[q] - 1] = gini[bv[q] - 1] + dec
    times = counttr.sum(axis=0).astype(np.int32)
    res = dict(counttr=counttr, votes=np.ascontiguousarray(counttr.T), oob_times=times,
               outcl=np.where(times > 0, counttr.argmax(axis=0) + 1, 0).astype(np.int32), errtr=errtr, err_wrong=err_wrong, err_seen=err_seen)
    if importance:
        imp = np.zeros((D, nclass + 2))
        sd = np.zeros((D, nclass + 1))
        nt = float(ntree)
        for v in range(D):
            for c in range(nclass + 1):
                mean = s_sum[v][c] / nt
                var = (s_sq[v][c] / nt - mean * mean) / nt
                imp[v, c] = mean
                sd[v, c] = math.sqrt(var if var > 0.0 else 0.0)
            imp[v, nclass + 1] = gini[v] / nt
        res.update(importance=imp, importanceSD=sd)
    if details is not None:
        details["trees"] = per_tree
        details["model"] = model
    return res


INT_KEYS = ("outcl", "counttr", "votes", "oob_times", "err_wrong", "err_seen")
BIT_KEYS = ("errtr", "importance", "importanceSD")


def differences(got, want):
    """names of the arrays of `want` that `got` does not hold exactly: integers ==, doubles bit for bit"""
    bad = []
    for k in want:
        if k not in got or got[k].shape != want[k].shape:
            bad.append(k)
        elif k in BIT_KEYS:
            if not (np.ascontiguousarray(got[k], np.float64).view(np.uint64) == np.ascontiguousarray(want[k], np.float64).view(np.uint64)).all():
                bad.append(k)
        elif not (got[k] == want[k]).all():
            bad.append(k)
    return bad
