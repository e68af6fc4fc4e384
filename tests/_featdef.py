"""The boundary-classifier feature row, stated from the reference's definitions in plain numpy / Python.

No ctypes, no oracle, no device: voxel lists walked in Python, one rule per function, every rule with the place in the
reference (glia/code/...) it restates.  It is the second author of the expected feature values: the oracle
(oracle/hmt_oracle.cc) is compared with it in test_oracle_feat_definitions.py, the device in test_gpu_feat_definitions.py.

    g = Geometry(labels, mask, order)                    # leaves, merged regions, the boundary of every merge
    rows = feature_rows(g, pb, rb=[(img, bins, lo, hi)], thresholds=(0.2, 0.5, 0.8), ...)

Volumes are numpy arrays in (z, y, x) / (y, x) order; a point's coordinate i is axis D-1-i (x first), as in itk::Index.
"""
import math

import numpy as np

FEPS = 2.22e-16                 # glia_base.hxx:57


def sdivide(lhs, rhs, dummy=0.0):          # glia_base.hxx:77-78
    return lhs / rhs if abs(rhs) >= FEPS else dummy


def slog(x, dummy=0.0):                    # glia_base.hxx:80-81
    return math.log(x) if x > 0.0 else dummy


def ssqrt(x, dummy=0.0):                   # glia_base.hxx:83-84
    return math.sqrt(x) if x >= 0.0 else dummy


def isfeq(a, b):                           # glia_base.hxx:71-72
    return abs(a - b) < FEPS


# ---------------------------------------------------------------------------------------------------------------------
# voxel lists
# ---------------------------------------------------------------------------------------------------------------------

def contour_traits(labels, mask, idx):
    """getContourTraits (type/neighbor.hxx:109-126) over traverseNeighbors (neighbor.hxx:72-89): the valid neighbours in the
    order x-1, x+1, y-1, y+1[, z-1, z+1] -- inside the volume and not masked out; returns (first neighbour value that differs
    from the voxel's own, else its own; fewer than 2 D valid neighbours)."""
    D = labels.ndim
    this = int(labels[idx])
    nvs = []
    for i in range(D):
        ax = D - 1 - i
        for d in (-1, 1):
            j = list(idx)
            j[ax] += d
            if 0 <= j[ax] < labels.shape[ax] and (mask is None or mask[tuple(j)] != 0):
                nvs.append(int(labels[tuple(j)]))
    first = next((v for v in nvs if v != this), this)
    return first, len(nvs) < 2 * D


def leaf_lists(labels, mask=None):
    """genPointMap + genContourMap in point-map mode (util/struct.hxx:77-92, 95-124): masked-out voxels belong to no list; a
    voxel is a boundary point of the DIRECTED pair (own label, first differing valid neighbour), else a border point when it
    has fewer than 2 D valid neighbours.  Returns (points, border, boundary): label -> flat indices, (a, b) -> flat indices."""
    pts, border, bnd = {}, {}, {}
    for idx in np.ndindex(*labels.shape):
        if mask is not None and mask[idx] == 0:
            continue
        flat = int(np.ravel_multi_index(idx, labels.shape))
        this = int(labels[idx])
        pts.setdefault(this, []).append(flat)
        nb, short = contour_traits(labels, mask, idx)
        if nb != this:
            bnd.setdefault((this, nb), []).append(flat)
        elif short:
            border.setdefault(this, []).append(flat)
    return pts, border, bnd


class Region:
    """TRegion (type/region.hxx): points and border keyed by leaf label, boundary keyed by directed leaf pair."""

    def __init__(self):
        self.pts, self.border, self.bnd = {}, {}, {}

    def merge(self, other):
        """TRegion::merge(Self const&) (region.hxx:66-75): points and border lists are united; a boundary pair whose REVERSE is
        present cancels it (both go), every other pair -- also one whose partner never pointed back -- stays."""
        self.pts.update(other.pts)
        self.border.update(other.border)
        for (a, b), v in other.bnd.items():
            if (b, a) in self.bnd:
                del self.bnd[(b, a)]
            else:
                self.bnd[(a, b)] = v


def boundary_with(out, r0, r1):
    """TRegion::boundaryWith (region.hxx:42-51): the pairs of r0 whose second key is the FIRST key of some pair r1 still has."""
    firsts = {k[0] for k in r1.bnd}
    for k, v in r0.bnd.items():
        if k[1] in firsts:
            out[k] = v


def get_boundary(r0, r1):
    """getBoundary (util/struct.hxx:10-16): both sides."""
    b = {}
    boundary_with(b, r0, r1)
    boundary_with(b, r1, r0)
    return b


def _cat(d):
    return np.array([p for v in d.values() for p in v], np.int64)


class Geometry:
    """TRegionMap(image, mask, order, false) (type/region_map.hxx:42-48, 79-95, 113-118): the leaves, then region x2 of every
    merge built from an empty region by merging x0 and x1 into it."""

    def __init__(self, labels, mask, order):
        self.labels = np.asarray(labels)
        self.mask = None if mask is None else np.asarray(mask)
        self.shape = self.labels.shape
        self.dim = self.labels.ndim
        self.order = [tuple(int(v) for v in m) for m in order]
        self.leaf_pts, self.leaf_border, self.leaf_bnd = leaf_lists(self.labels, self.mask)
        self.regions = {}
        for l, p in self.leaf_pts.items():
            r = Region()
            r.pts = {l: p}
            if l in self.leaf_border:
                r.border = {l: self.leaf_border[l]}
            r.bnd = {k: v for k, v in self.leaf_bnd.items() if k[0] == l}
            self.regions[l] = r
        for x0, x1, x2 in self.order:
            r = self.regions.setdefault(x2, Region())
            if x2 != x0:
                r.merge(self.regions[x0])
            if x2 != x1:
                r.merge(self.regions[x1])
        self.lists = {k: (_cat(r.pts), _cat(r.bnd), _cat(r.border)) for k, r in self.regions.items()}


# ---------------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------------

def hist_bounds(bins, lo, hi):
    """util/image_stats.hxx:18-22 (= util/stats.hxx:100-104): bounds[0] = interval -- NOT lo + interval --, every further bound
    the previous one plus the interval, accumulated in double."""
    interval = (hi - lo) / bins
    bounds = [interval]
    for _ in range(1, bins):
        bounds.append(bounds[-1] + interval)
    return bounds


def histc(vals, bins, lo, hi):
    """histc (util/image_stats.hxx:12-37): a value strictly inside (lo, hi) counts in the first bin whose bound it is below --
    in NO bin when it is below none --, a value <= lo in bin 0, every other value in the last bin."""
    bounds = hist_bounds(bins, lo, hi)
    hc = [0] * bins
    for v in vals:
        v = float(v)
        if lo < v < hi:
            for i in range(bins):
                if v < bounds[i]:
                    hc[i] += 1
                    break
        elif v <= lo:
            hc[0] += 1
        else:
            hc[bins - 1] += 1
    return hc


def hist(vals, bins, lo, hi):
    """hist (image_stats.hxx:40-53): counts over the number of POINTS (not over the counted ones); zeros for no points."""
    n = len(vals)
    if n == 0:
        return [0.0] * bins
    return [c / float(n) for c in histc(vals, bins, lo, hi)]


def entropy(h):                            # util/stats.hxx:145-152
    ret = 0.0
    for p in h:
        if not isfeq(p, 0.0):
            ret -= p * math.log2(p)
    return ret


def dist_l1(h0, h1):                       # util/stats.hxx:155-163
    return float(sum(abs(p - q) for p, q in zip(h0, h1)))


def dist_x2(h0, h1):                       # util/stats.hxx:177-185
    return float(sum((p - q) ** 2 / (p + q + FEPS) for p, q in zip(h0, h1)))


def real_feats(vals, median_form):
    """ImageRealFeats::generate (type/feat.hxx:706-737): nothing is touched for an empty list (all zeros).  Default form: mean =
    sum / n, stddev = ssqrt(sum of squares / n - mean^2).  GLIA_USE_MEDIAN_AS_FEATS form: amedian (the element at n / 2 of the
    sorted values, util/stats.hxx:83-91), stats::mean, ssqrt(stats::var) (stats.hxx:56-70: mean of the squared deviations)."""
    n = len(vals)
    f = dict(median=0.0, mean=0.0, std=0.0, min=0.0, max=0.0)
    if n == 0:
        return f
    v = np.asarray(vals, np.float64)
    if median_form:
        f["median"] = float(np.sort(v)[n // 2])
        f["mean"] = sdivide(math.fsum(v), n)
        f["std"] = ssqrt(sdivide(math.fsum((v - f["mean"]) ** 2), n))
    else:
        f["mean"] = math.fsum(v) / n
        f["std"] = ssqrt(math.fsum(v * v) / n - f["mean"] * f["mean"])
    f["min"], f["max"] = float(v.min()), float(v.max())
    return f


def image_feats(vals, bins, lo, hi, median_form, label_only=False):
    """ImageLabelFeats (feat.hxx:632-638) [+ ImageRealFeats: ImageFeats, feat.hxx:846-852]"""
    f = dict(hist=hist(vals, bins, lo, hi))
    f["entropy"] = entropy(f["hist"])
    if not label_only:
        f.update(real_feats(vals, median_form))
    return f


# ---------------------------------------------------------------------------------------------------------------------
# feature classes
# ---------------------------------------------------------------------------------------------------------------------

def region_shape(g, key, pb, thresholds, norm_area, norm_len):
    """RegionShapeFeats::generate (feat.hxx:71-90) + ImageRegionShapeFeats::generate (feat.hxx:485-502)"""
    P, B, Bo = g.lists[key]
    D = g.dim
    area = float(len(P))
    perim = float(len(B) + len(Bo))
    s = dict(compactness=sdivide(math.pow(perim, float(D) / (D - 1)), area))
    s["area"] = sdivide(area, norm_area)
    s["perim"] = sdivide(perim, norm_len)
    co = np.array(np.unravel_index(P, g.shape))[::-1]              # rows x, y[, z]
    bb = [float(c.max() - c.min()) for c in co]                    # alg/geometry.hxx:22-39: upper - lower, no + 1
    s["bbox"] = [sdivide(x, norm_len) for x in bb]
    ba = 1.0
    for x in bb:
        ba *= x
    s["bbox_area"] = sdivide(ba, norm_area)
    pv = pb.ravel()[B]
    vps = [int(sum(1 for v in pv if float(v) >= t)) for t in thresholds]
    s["vp"] = [sdivide(vp, norm_len) for vp in vps]
    s["rvp"] = [sdivide(vp, len(B)) for vp in vps]
    return s


def region_feats(g, key, pb, thresholds, r_images, rl_images, b_images, norm_area, norm_len, median_form, saliency):
    """RegionFeats::generate (hmt/bc_feat.hxx:88-127)"""
    P, B, _ = g.lists[key]
    return dict(shape=region_shape(g, key, pb, thresholds, norm_area, norm_len),
                region=[image_feats(img.ravel()[P], bins, lo, hi, median_form) for img, bins, lo, hi in r_images],
                label=[image_feats(img.ravel()[P], bins, lo, hi, median_form, label_only=True) for img, bins, lo, hi in rl_images],
                boundary=[image_feats(img.ravel()[B], bins, lo, hi, median_form) for img, bins, lo, hi in b_images],
                saliency=saliency)


def boundary_feats(bpts, rf0, rf1, rf2, pb, thresholds, b_images, norm_len, median_form):
    """BoundaryFeats::generate (bc_feat.hxx:179-214) over RegionShapeDiffFeats (feat.hxx:124-132), RegionShapeIntraDiffFeats
    (feat.hxx:176-186), ImageRegionShapeIntraDiffFeats (feat.hxx:567-589), ImageLabelDiffFeats (feat.hxx:663-669) and
    ImageRealDiffFeats (feat.hxx:801-810)"""
    s0, s1 = rf0["shape"], rf1["shape"]
    s = {}
    s["area_diff"] = abs(s0["area"] - s1["area"])
    s["r_area_diff"] = [sdivide(s["area_diff"], s0["area"]), sdivide(s["area_diff"], s1["area"])]
    s["perim_diff"] = abs(s0["perim"] - s1["perim"])
    s["r_perim_diff"] = [sdivide(s["perim_diff"], s0["perim"]), sdivide(s["perim_diff"], s1["perim"])]
    s["blen"] = sdivide(math.ceil(len(bpts) / 2.0), norm_len)
    s["r_blen"] = [sdivide(s["blen"], s0["area"]), sdivide(s["blen"], s1["area"]),
                   sdivide(s["blen"], s0["perim"]), sdivide(s["blen"], s1["perim"])]
    pv = pb.ravel()[bpts]
    s["vbl"] = [sdivide(math.ceil(sum(1 for v in pv if float(v) >= t) / 2.0), norm_len) for t in thresholds]
    s["r_vbl"] = [sdivide(v, s["blen"]) for v in s["vbl"]]
    s["r_vbl_p0"] = [sdivide(v, s0["perim"]) for v in s["vbl"]]
    s["r_vbl_p1"] = [sdivide(v, s1["perim"]) for v in s["vbl"]]
    f = dict(shape=s, region=[], label=[], boundary=[], saliency=None)
    for a, b in zip(rf0["region"], rf1["region"]):
        f["region"].append(dict(l1=dist_l1(a["hist"], b["hist"]), x2=dist_x2(a["hist"], b["hist"]),
                                entropy=abs(a["entropy"] - b["entropy"]), median=abs(a["median"] - b["median"]),
                                mean=abs(a["mean"] - b["mean"]), std=abs(a["std"] - b["std"]),
                                min=abs(a["min"] - b["min"]), max=abs(a["max"] - b["max"])))
    for a, b in zip(rf0["label"], rf1["label"]):
        f["label"].append(dict(l1=dist_l1(a["hist"], b["hist"]), x2=dist_x2(a["hist"], b["hist"]),
                               entropy=abs(a["entropy"] - b["entropy"])))
    for img, bins, lo, hi in b_images:
        f["boundary"].append(image_feats(img.ravel()[bpts], bins, lo, hi, median_form))
    if rf0["saliency"] is not None and rf1["saliency"] is not None and rf2["saliency"] is not None:   # bc_feat.hxx:208-213
        d02, d12 = abs(rf0["saliency"] - rf2["saliency"]), abs(rf1["saliency"] - rf2["saliency"])
        f["saliency"] = (min(d02, d12), max(d02, d12))
    return f


def log_region(rf):
    """RegionFeats::log -> ImageRegionShapeFeats::log (bc_feat.hxx:67, feat.hxx:46-52, 463-467): not the compactness, not the
    ratios"""
    s = rf["shape"]
    s["area"], s["perim"], s["bbox_area"] = slog(s["area"]), slog(s["perim"]), slog(s["bbox_area"])
    s["bbox"] = [slog(x) for x in s["bbox"]]
    s["vp"] = [slog(x) for x in s["vp"]]


def log_boundary(bf):
    """BoundaryFeats::log -> ImageRegionShapeIntraDiffFeats::log (bc_feat.hxx:154, feat.hxx:103-106, 148-155, 531-539)"""
    s = bf["shape"]
    s["area_diff"], s["perim_diff"], s["blen"] = slog(s["area_diff"]), slog(s["perim_diff"]), slog(s["blen"])
    s["vbl"] = [slog(x) for x in s["vbl"]]


def _ser_label(f, hist_cols):              # ImageLabelFeats::serialize (feat.hxx:616-623)
    return (list(f["hist"]) if hist_cols else []) + [f["entropy"]]


def _ser_real(f, median_form):             # ImageRealFeats / ImageRealDiffFeats::serialize (feat.hxx:687-696, 782-791)
    return ([f["median"]] if median_form else []) + [f["mean"], f["std"], f["min"], f["max"]]


def serialize_region(rf, hist_cols, median_form):
    """RegionFeats::serialize (bc_feat.hxx:69-77) over RegionShapeFeats / ImageRegionShapeFeats::serialize (feat.hxx:54-62,
    469-476) and ImageFeats::serialize (feat.hxx:835-839)"""
    s = rf["shape"]
    out = [s["area"], s["perim"], s["compactness"], s["bbox_area"]] + s["bbox"] + s["vp"] + s["rvp"]
    for f in rf["region"]:
        out += _ser_label(f, hist_cols) + _ser_real(f, median_form)
    for f in rf["label"]:
        out += _ser_label(f, hist_cols)
    for f in rf["boundary"]:
        out += _ser_label(f, hist_cols) + _ser_real(f, median_form)
    if rf["saliency"] is not None:
        out.append(rf["saliency"])
    return out


def serialize_boundary(bf, hist_cols, median_form):
    """BoundaryFeats::serialize (bc_feat.hxx:156-167) over RegionShapeDiffFeats, RegionShapeIntraDiffFeats and
    ImageRegionShapeIntraDiffFeats::serialize (feat.hxx:108-116, 157-165, 541-556), ImageDiffFeats::serialize (feat.hxx:868-872)"""
    s = bf["shape"]
    out = [s["area_diff"]] + s["r_area_diff"] + [s["perim_diff"]] + s["r_perim_diff"] + [s["blen"]] + s["r_blen"]
    out += s["vbl"] + s["r_vbl"] + s["r_vbl_p0"] + s["r_vbl_p1"]
    for f in bf["region"]:
        out += [f["l1"], f["x2"], f["entropy"]] + _ser_real(f, median_form)
    for f in bf["label"]:
        out += [f["l1"], f["x2"], f["entropy"]]
    for f in bf["boundary"]:
        out += _ser_label(f, hist_cols) + _ser_real(f, median_form)
    if bf["saliency"] is not None:
        out += list(bf["saliency"])
    return out


def select_features(bf, rf0, rf1, median_form):
    """selectFeatures (bc_feat.hxx:247-279)"""
    out = [rf0["shape"]["area"], rf1["shape"]["area"], rf0["shape"]["perim"], rf1["shape"]["perim"], bf["shape"]["blen"]]
    for f in bf["boundary"]:
        out.append(f["mean"])
        if median_form:
            out.append(f["median"])
    for f in bf["region"]:
        out += [f["mean"], f["l1"], f["x2"], f["entropy"]]
    for f in bf["label"]:
        out += [f["l1"], f["x2"]]
    return out


def feat_dim(dim, n_thr, r_bins, rl_bins, b_bins, hist_cols=False, median_form=False, saliency=False, simple=False):
    """dim() of BoundaryClassificationFeats (bc_feat.hxx:57-65, 144-152, 227-230) from the classes' own dim members (feat.hxx:30,
    42, 97, 141, 458, 524, 608-612, 646, 677-682, 772-777), or the length selectFeatures reserves (bc_feat.hxx:250-256)."""
    R = 5 if median_form else 4
    L = (lambda b: b + 1) if hist_cols else (lambda b: 1)
    if simple:
        return 5 + (2 if median_form else 1) * len(b_bins) + 4 * len(r_bins) + 2 * len(rl_bins)
    x0 = 6 + 5 + 4 * n_thr + sum(3 + R for _ in r_bins) + 3 * len(rl_bins) + sum(L(b) + R for b in b_bins) + (2 if saliency else 0)
    reg = 4 + dim + 2 * n_thr + sum(L(b) + R for b in r_bins) + sum(L(b) for b in rl_bins) + sum(L(b) + R for b in b_bins) + (1 if saliency else 0)
    return x0 + 3 * reg


def saliency_map(order, saliencies, init_sal, sal_bias):
    """genSaliencyMap (bc_feat.hxx:12-26)"""
    m = {}
    for (x0, x1, x2), s in zip(order, saliencies):
        m.setdefault(x0, init_sal)
        m.setdefault(x1, init_sal)
        m[x2] = float(s) + sal_bias
    return m


def feature_rows(g, pb, rb=(), r=(), rl=(), b=(), thresholds=(0.2, 0.5, 0.8), norm_area=1.0, norm_len=1.0, use_log=False,
                 use_simple=False, hist_as_feats=False, median_as_feats=False, saliencies=None, init_sal=1.0, sal_bias=1.0):
    """hmt/main_bc_feat.cxx:27-110: one row per merge of g.order.  rb / r / rl / b: lists of (image, bins, lo, hi); the lists
    the classes see are built as prepareImages builds them (hmt/hmt_util.hxx:28-53): region images = rb then r, boundary images
    = rb then b, label images = rl."""
    r_images, rl_images, b_images = list(rb) + list(r), list(rl), list(rb) + list(b)
    smap = None if saliencies is None else saliency_map(g.order, saliencies, init_sal, sal_bias)
    rfs = {}
    for key in g.regions:
        sal = None if smap is None else smap.get(key)           # main_bc_feat.cxx:68: ccpointer(saliencyMap, key)
        rfs[key] = region_feats(g, key, pb, thresholds, r_images, rl_images, b_images, norm_area, norm_len, median_as_feats, sal)
    picks = []
    for x0, x1, x2 in g.order:
        k0, k1 = x0, x1
        if rfs[k0]["shape"]["area"] > rfs[k1]["shape"]["area"]:  # main_bc_feat.cxx:85-89: strictly greater
            k0, k1 = k1, k0
        bpts = _cat(get_boundary(g.regions[k0], g.regions[k1]))
        bf = boundary_feats(bpts, rfs[k0], rfs[k1], rfs[x2], pb, thresholds, b_images, norm_len, median_as_feats)
        picks.append((bf, k0, k1, x2))
    if use_log:                                                  # main_bc_feat.cxx:97-102: after every difference was taken
        for rf in rfs.values():
            log_region(rf)
        for bf, _, _, _ in picks:
            log_boundary(bf)
    rows = []
    for bf, k0, k1, k2 in picks:
        if use_simple:                                           # main_bc_feat.cxx:103-108
            rows.append(select_features(bf, rfs[k0], rfs[k1], median_as_feats))
        else:                                                    # BoundaryClassificationFeats::serialize (bc_feat.hxx:232-238)
            rows.append(serialize_boundary(bf, hist_as_feats, median_as_feats) +
                        serialize_region(rfs[k0], hist_as_feats, median_as_feats) +
                        serialize_region(rfs[k1], hist_as_feats, median_as_feats) +
                        serialize_region(rfs[k2], hist_as_feats, median_as_feats))
    d = len(rows[0]) if rows else 0
    return np.array(rows, np.float64).reshape(len(rows), d)


def column_names(dim, n_thr, r_bins, rl_bins, b_bins, hist_cols=False, median_form=False, saliency=False, simple=False):
    """One name per column, in the order serialize_boundary / serialize_region / select_features write them: 'x0.' the boundary
    block, 'x1.' / 'x2.' / 'x3.' the smaller, the larger and the merged region; image blocks 'r<i>', 'l<i>', 'b<i>'.  The tests
    pick columns by name (masks, stub indices, literals)."""
    real = (["median"] if median_form else []) + ["mean", "std", "min", "max"]
    lab = lambda b: (["h%d" % k for k in range(b)] if hist_cols else []) + ["entropy"]
    if simple:
        out = ["x1.area", "x2.area", "x1.perim", "x2.perim", "x0.blen"]
        for j in range(len(b_bins)):
            out += ["x0.b%d.mean" % j] + (["x0.b%d.median" % j] if median_form else [])
        for j in range(len(r_bins)):
            out += ["x0.r%d.%s" % (j, n) for n in ("mean", "l1", "x2", "entropy")]
        for j in range(len(rl_bins)):
            out += ["x0.l%d.%s" % (j, n) for n in ("l1", "x2")]
        return out
    out = ["x0.area_diff", "x0.r_area_diff0", "x0.r_area_diff1", "x0.perim_diff", "x0.r_perim_diff0", "x0.r_perim_diff1",
           "x0.blen", "x0.r_blen_area0", "x0.r_blen_area1", "x0.r_blen_perim0", "x0.r_blen_perim1"]
    for n in ("vbl", "r_vbl", "r_vbl_p0", "r_vbl_p1"):
        out += ["x0.%s%d" % (n, t) for t in range(n_thr)]
    for j in range(len(r_bins)):
        out += ["x0.r%d.%s" % (j, n) for n in ["l1", "x2", "entropy"] + real]
    for j in range(len(rl_bins)):
        out += ["x0.l%d.%s" % (j, n) for n in ("l1", "x2", "entropy")]
    for j, b in enumerate(b_bins):
        out += ["x0.b%d.%s" % (j, n) for n in lab(b) + real]
    if saliency:
        out += ["x0.sal_min", "x0.sal_max"]
    for x in ("x1", "x2", "x3"):
        out += [x + "." + n for n in ("area", "perim", "compactness", "bbox_area")] + [x + ".bbox%d" % i for i in range(dim)]
        out += [x + ".vp%d" % t for t in range(n_thr)] + [x + ".rvp%d" % t for t in range(n_thr)]
        for j, b in enumerate(r_bins):
            out += ["%s.r%d.%s" % (x, j, n) for n in lab(b) + real]
        for j, b in enumerate(rl_bins):
            out += ["%s.l%d.%s" % (x, j, n) for n in lab(b)]
        for j, b in enumerate(b_bins):
            out += ["%s.b%d.%s" % (x, j, n) for n in lab(b) + real]
        if saliency:
            out.append(x + ".saliency")
    return out
