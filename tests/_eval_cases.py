"""Segmentation scores: a plain-Python restatement of the reference's eval_ri and eval_vi, shared by test_eval_host.py,
test_gpu_eval.py and test_gpu_eval_cli.py.

The reference tools (gadget/main_eval_ri.cxx, gadget/main_eval_vi.cxx) need ITK and Boost.Multiprecision, which are not available, so
parity rests on this second-author restatement: dicts, Python ints and math.fsum, no code shared with the library.  With the
reference's lines:
  * contingency: the loop of stats::pairStats / stats::centropy on images (util/image_stats.hxx:257-270, :132-147): a voxel counts
    if its mask value is not MASK_OUT_VAL = 0 and its reference label is not BG_VAL = 0 (excluded1 = {BG_VAL}; the proposed label 0
    is a label like any other);
  * pair_stats: util/stats.hxx:189-229;  precision / recall / f1 / rand_index: :232-261 with FEPS = 2.22e-16 (glia_base.hxx:57,71-72);
  * centropy: util/image_stats.hxx:148-157 -- `up.second / bp.second` divides two uints, so mode "reference" takes log2 of the
    INTEGER quotient; mode "exact" takes the real quotient;
  * eval_ri: the four counts are added over the image pairs, then the ratios (main_eval_ri.cxx:41-59);
  * eval_vi: stats::mean of the per-pair entropies (main_eval_vi.cxx:23-27, util/stats.hxx:38-58).
Entropy sums use math.fsum (correctly rounded), so they are the yardstick a sum in any order is held to."""
import math

import numpy as np

FEPS = 2.22e-16


def contingency(res, ref, mask=None, drop_zero_res=False, drop_zero_ref=True):
    """{(a, b): voxels} of two label arrays of equal size (any shape)"""
    a = np.asarray(res).reshape(-1).tolist()
    b = np.asarray(ref).reshape(-1).tolist()
    m = [1] * len(a) if mask is None else np.asarray(mask).reshape(-1).tolist()
    assert len(a) == len(b) == len(m)
    cmap = {}
    for x, y, k in zip(a, b, m):
        if k == 0 or (drop_zero_res and x == 0) or (drop_zero_ref and y == 0):
            continue
        cmap[(x, y)] = cmap.get((x, y), 0) + 1
    return cmap


def marginals(cmap):
    na, nb = {}, {}
    for (a, b), c in cmap.items():
        na[a] = na.get(a, 0) + c
        nb[b] = nb.get(b, 0) + c
    return na, nb


def pair_stats(cmap):
    """(TP, TN, FP, FN) as Python ints (util/stats.hxx:189-229)"""
    n = sum(cmap.values())
    tp = sum(c * (c - 1) // 2 for c in cmap.values())
    na, nb = marginals(cmap)
    n_pair = n * (n - 1) // 2
    key1 = sum(v * (v - 1) // 2 for v in nb.values())        # pairs with identical reference label
    key0 = sum(v * (v - 1) // 2 for v in na.values())        # pairs with identical proposed label
    return tp, n_pair - key1 + tp - key0, key0 - tp, key1 - tp


def _guard(den):
    return den if not abs(den - 0.0) < FEPS else den + FEPS


def precision(tp, fp):
    return float(tp) / _guard(float(tp + fp))


def recall(tp, fn):
    return float(tp) / _guard(float(tp + fn))


def f1(p, r):
    return 2.0 * p * r / (p + r) if p + r != 0.0 else math.nan      # the C++ 0.0 / 0.0


def rand_index(tp, tn, fp, fn):
    num = float(tp + tn)
    den = float(fp + fn)
    den += num
    return num / _guard(den)


def centropy(cmap, given, mode="reference"):
    """H(a | b) for given = "b" (false split), H(b | a) for given = "a" (false merge): sum c log2(q) / n"""
    na, nb = marginals(cmap)
    n = sum(cmap.values())
    if n == 0:
        return math.nan                                             # the C++ 0.0 / 0
    terms = []
    for (a, b), c in cmap.items():
        m = nb[b] if given == "b" else na[a]
        terms.append(c * math.log2(m // c if mode == "reference" else m / c))
    return math.fsum(terms) / n


def scores(cmaps, mode="reference"):
    """what eval_ri and eval_vi compute over a list of contingency tables, keyed like hmt.overlap_scores' result"""
    tp = tn = fp = fn = 0
    fs, fm = 0.0, 0.0
    for cmap in cmaps:
        t = pair_stats(cmap)
        tp, tn, fp, fn = tp + t[0], tn + t[1], fp + t[2], fn + t[3]
        fs += centropy(cmap, "b", mode)
        fm += centropy(cmap, "a", mode)
    p, r = precision(tp, fp), recall(tp, fn)
    return {"TP": tp, "TN": tn, "FP": fp, "FN": fn, "precision": p, "recall": r, "f1": f1(p, r), "rand_index": rand_index(tp, tn, fp, fn),
            "false_split": fs / len(cmaps), "false_merge": fm / len(cmaps)}


def evaluate(res, ref, masks=None, mode="reference"):
    """scores() from lists of label arrays (masks: None or a list that may hold None)"""
    masks = [None] * len(res) if masks is None else masks
    return scores([contingency(p, r, m) for p, r, m in zip(res, ref, masks)], mode)


def entries(cmap):
    """the table as the library lays it out: structured array (a, b, count) ascending by (a, b)"""
    out = np.empty(len(cmap), np.dtype([("a", np.uint32), ("b", np.uint32), ("count", np.uint64)]))
    for i, ((a, b), c) in enumerate(sorted(cmap.items())):
        out[i] = (a, b, c)
    return out


def same_float(x, y):
    return (math.isnan(x) and math.isnan(y)) or x == y


def close(x, y, rel):
    return (math.isnan(x) and math.isnan(y)) or abs(x - y) <= rel * abs(y)


def check_against(got, want, entropy_rel=1e-12):
    """The tolerances of the issue: integers exact; ratios bit-identical whenever every count is below 2^53 (above, the two sides
    each round two integers to nearest and divide: within 1e-15); entropies within 1e-12 relative -- a double sum of E <= 4096
    non-negative terms is within about E * 2^-53 = 4.6e-13 of the correctly rounded one."""
    for k in ("TP", "TN", "FP", "FN"):
        assert got[k] == want[k], (k, got[k], want[k])
    small = all(want[k] < 2 ** 53 for k in ("TP", "TN", "FP", "FN")) and want["TP"] + want["TN"] + want["FP"] + want["FN"] < 2 ** 53
    for k in ("precision", "recall", "f1", "rand_index"):
        assert same_float(got[k], want[k]) if small else close(got[k], want[k], 1e-15), (k, got[k], want[k])
    for k in ("false_split", "false_merge"):
        assert close(got[k], want[k], entropy_rel), (k, got[k], want[k])


def fmt(x):
    """a double as std::ostream prints it by default (precision 6, %g)"""
    return "%g" % x
