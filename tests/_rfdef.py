"""The second author of train_forest: the growing rule of DESIGN 3.12 restated in plain NumPy / Python, with no library call and no
oracle.  Every model array the device trainer returns must equal what this file computes, integers exactly and xbestsplit bit for bit
(tests/test_gpu_forest_train.py); tests/test_rf_definition.py holds this file to trees worked out by hand."""
import math

import numpy as np

M64 = (1 << 64) - 1
DEFAULT_SEED = 0x9E3779B97F4A7C15


def mix(z):
    """splitmix64 finaliser on Python integers"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def h(seed, t, a, b):
    return mix(mix(mix(mix(seed) ^ t) ^ a) ^ b)


def _mix_np(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def h_many(seed, t, a, n):
    """h(seed, t, a, b) for b = 0 .. n-1"""
    base = np.uint64(mix(mix(mix(seed) ^ t) ^ a))
    return _mix_np(base ^ np.arange(n, dtype=np.uint64))


def sampsize_of(n_rows, sample_ratio):
    """main_train_rf.cxx:40-44: (int)((float)N * sampleSizeRatio + 0.5)"""
    if sample_ratio > 1e-6:
        return int(float(np.float32(n_rows)) * sample_ratio + 0.5)
    return n_rows


def mtry_of(mtry, dim):
    """ml_rf_train.cxx:362,376"""
    if mtry <= 0 or mtry > dim:
        mtry = int(math.floor(math.sqrt(float(dim))))
    return max(1, min(dim, mtry))


def class_weights(counts, balance):
    """main_train_rf.cxx:46-60"""
    if not balance:
        return [1.0] * len(counts)
    maxcnt = max(counts)
    return [float(maxcnt) / float(c) for c in counts]


def derive(y, dim, mtry=0, sample_ratio=0.7, balance=1):
    y = np.asarray(y)
    orig = sorted(set(int(v) for v in y))
    cls = np.array([orig.index(int(v)) for v in y], np.int64)
    counts = [int((cls == k).sum()) for k in range(len(orig))]
    return dict(orig_labels=orig, cls=cls, nclass=len(orig), classwt=class_weights(counts, balance), cutoff=[1.0 / len(orig)] * len(orig),
                sampsize=sampsize_of(len(y), sample_ratio), mtry=mtry_of(mtry, dim))


def bootstrap(seed, t, n_rows, sampsize):
    """multiplicity of every row in tree t's sample"""
    draws = h_many(seed, t, 0, sampsize) % np.uint64(n_rows)
    return np.bincount(draws.astype(np.int64), minlength=n_rows).astype(np.int64)


def tried_variables(seed, t, node, dim, mtry):
    hv = h_many(seed, t, 1 + node, dim)
    order = sorted(range(dim), key=lambda v: (int(hv[v]), v))
    return sorted(order[:mtry])


def crit_of(w, nL, nR):
    """numL / denL + numR / denR from integer counts, in the stated order (arrays of float64 or scalars)"""
    numL = 0.0
    denL = 0.0
    numR = 0.0
    denR = 0.0
    for k in range(len(w)):
        tL = np.float64(w[k]) * np.asarray(nL[k], np.int64).astype(np.float64)
        numL = numL + tL * tL
        denL = denL + tL
        tR = np.float64(w[k]) * np.asarray(nR[k], np.int64).astype(np.float64)
        numR = numR + tR * tR
        denR = denR + tR
    return numL / denL + numR / denR


def best_cut(X, rows, cls, mult, w, variables):
    """(variable, split, rows going left) of the best cut of a node over `variables` (ascending), or None"""
    nclass = len(w)
    best = None
    n_k = [int(mult[rows][cls[rows] == k].sum()) for k in range(nclass)]
    for v in variables:
        x = X[rows, v] + 0.0                                  # -0.0 -> +0.0
        order = np.argsort(x, kind="stable")
        xs = x[order]
        cut = np.nonzero(xs[:-1] != xs[1:])[0]                # a cut after sorted position i, between distinct values
        if len(cut) == 0:
            continue
        r = rows[order]
        nL = [np.cumsum(np.where(cls[r] == k, mult[r], 0))[cut] for k in range(nclass)]
        nR = [n_k[k] - nL[k] for k in range(nclass)]
        with np.errstate(all="ignore"):
            crit = crit_of(w, nL, nR)
        i = int(np.argmax(crit))                              # first of the largest: lowest x_a
        if best is None or crit[i] > best[0]:
            xa, xb = float(xs[cut[i]]), float(xs[cut[i] + 1])
            s = 0.5 * xa + 0.5 * xb
            if not s < xb:
                s = xa
            best = (float(crit[i]), v, s, r[: cut[i] + 1], r[cut[i] + 1:])
    return best


def grow_tree(X, cls, w, t, seed=DEFAULT_SEED, sampsize=None, mtry=1, nodesize=1, max_depth=0, root_only=False, mult=None):
    """lists over the nodes of tree t: left (1-based daughter, 0 = terminal), bestvar (1-based), split, nodeclass (1-based).  mult: given
    multiplicities in place of the tree's bootstrap (the hand-worked trees of tests/test_rf_definition.py)"""
    n_rows, dim = X.shape
    nclass = len(w)
    mult = bootstrap(seed, t, n_rows, n_rows if sampsize is None else sampsize) if mult is None else np.asarray(mult, np.int64)
    nodes = [dict(rows=np.nonzero(mult)[0], depth=0)]
    left, var, split, ncl = [], [], [], []
    k = 0
    while k < len(nodes):
        rows, depth = nodes[k]["rows"], nodes[k]["depth"]
        n_k = [int(mult[rows][cls[rows] == c].sum()) for c in range(nclass)]
        terminal = len(rows) <= nodesize or sum(1 for c in n_k if c > 0) <= 1 or (max_depth > 0 and depth == max_depth)
        cut = None if terminal else best_cut(X, rows, cls, mult, w, tried_variables(seed, t, k, dim, mtry))
        if root_only:
            return cut
        if cut is None:
            score = [np.float64(w[c]) * np.float64(n_k[c]) for c in range(nclass)]
            left.append(0); var.append(0); split.append(0.0); ncl.append(1 + int(np.argmax(score)))      # ties: lowest class
        else:
            left.append(len(nodes) + 1); var.append(cut[1] + 1); split.append(cut[2]); ncl.append(0)
            nodes.append(dict(rows=cut[3], depth=depth + 1))
            nodes.append(dict(rows=cut[4], depth=depth + 1))
        nodes[k] = None
        k += 1
    return left, var, split, ncl


def train(X, y, ntree=255, mtry=0, sample_ratio=0.7, nodesize=1, balance=1, max_depth=0, seed=DEFAULT_SEED, first_tree=0):
    """the model arrays of train_forest (trees first_tree .. first_tree + ntree - 1 of the seed)"""
    X = np.ascontiguousarray(X, np.float64)
    d = derive(y, X.shape[1], mtry, sample_ratio, balance)
    trees = [grow_tree(X, d["cls"], d["classwt"], first_tree + t, seed, d["sampsize"], d["mtry"], nodesize, max_depth) for t in range(ntree)]
    nrnodes = max(len(t[0]) for t in trees)
    out = dict(xbestsplit=np.zeros((ntree, nrnodes)), treemap=np.zeros((ntree, nrnodes, 2), np.int32), nodestatus=np.zeros((ntree, nrnodes), np.int32),
               nodeclass=np.zeros((ntree, nrnodes), np.int32), bestvar=np.zeros((ntree, nrnodes), np.int32),
               ndbigtree=np.array([len(t[0]) for t in trees], np.int32), classwt=np.array(d["classwt"]), cutoff=np.array(d["cutoff"]),
               orig_labels=np.array(d["orig_labels"], np.int32), new_labels=np.arange(1, d["nclass"] + 1, dtype=np.int32), mtry=d["mtry"])
    for j, (left, var, split, ncl) in enumerate(trees):
        n = len(left)
        out["xbestsplit"][j, :n] = split
        out["treemap"][j, :n, 0] = left
        out["treemap"][j, :n, 1] = [l + 1 if l else 0 for l in left]
        out["nodestatus"][j, :n] = [1 if l else -1 for l in left]
        out["nodeclass"][j, :n] = ncl
        out["bestvar"][j, :n] = var
    return out


def walk(model, j, x):
    """the terminal node (0-based) row x ends in, in tree j: x[var] <= split goes left"""
    k = 0
    while model["nodestatus"][j, k] == 1:
        k = int(model["treemap"][j, k, 0 if x[model["bestvar"][j, k] - 1] <= model["xbestsplit"][j, k] else 1]) - 1
    return k


def predict(model, X, label=-1):
    """votes for `label` / ntree"""
    target = 1 + list(model["orig_labels"]).index(label)
    ntree = model["xbestsplit"].shape[0]
    out = np.zeros(len(X))
    for i, x in enumerate(X):
        out[i] = sum(1 for j in range(ntree) if model["nodeclass"][j, walk(model, j, x)] == target) / ntree
    return out
