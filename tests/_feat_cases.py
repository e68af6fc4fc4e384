"""Shared cases of the feature-row tests (test_oracle_feat_definitions.py without a GPU, test_gpu_feat_definitions.py with one).

Every volume has at most about 4 000 voxels: tests/_featdef.py walks voxels in Python, and these are the smallest shapes that
still reach each rule.  A case is a geometry (labels, mask, merge order), named images, the four image lists as
(image name, bins, lo, hi), a threshold list and the layout switches.  case(name) builds one (cached); NAMES lists them all.

Q8 images (multiples of 1/256 in [0, 1), or small integers): every sum and sum of squares is exact in double whatever the
summation order, so the device is compared with the oracle bit for bit.  Edge-value images are not: they hold, for one histogram
spec and threshold list, the float32 neighbourhood of every value at which a count changes.
"""
import functools

import numpy as np

import _featdef as FD

THR_LISTS = [(), (0.5,), (0.25, 0.75), (0.125, 0.25, 0.5, 0.75), (0.8, 0.2, 0.5), (0.5, 0.5)]
SPECS = {"b1": (1, 0.0, 1.0), "b3": (3, 0.0, 1.0), "b7": (7, 0.0, 1.0), "b10": (10, 0.0, 1.0), "b13": (13, 0.0, 1.0),
         "b16": (16, 0.0, 1.0), "b10_01_09": (10, 0.1, 0.9), "b16_labels": (16, -0.5, 7.5),
         # two specs at which the ACCUMULATED bound and (i + 1) * interval put a float32 value into different bins: bound 14 of
         # the first is 0.7500000000000001 (the Q8 value 0.75 is below it), the last bound of the second 7.000000000000001
         "b16_01_09": (16, 0.1, 0.9), "b6_05_75": (6, 0.5, 7.5)}
INTEGER_SPECS = ("b16_labels", "b6_05_75")                        # run on the integer-valued image (0..7)
DEFAULT_THR = (0.2, 0.5, 0.8)

# ---- boxes: closed-form answers -------------------------------------------------------------------------------------
# A 4 x 4 x 8 volume (z, y, x), label 1 where x < 3, label 2 elsewhere; one merge (1, 2 -> 3).
#   region 1: 4 * 4 * 3 = 48 voxels.  Its plane x = 2 faces label 2: 16 boundary points.  Border points are the other voxels with
#             a neighbour outside the volume: all 16 of plane x = 0, and the 4 * 4 - 2 * 2 = 12 rim voxels of plane x = 1: 28.
#             perimeter 16 + 28 = 44; bounding box (upper - lower) = (2, 3, 3), box area 18; compactness 44^(3/2) / 48.
#   region 2: 4 * 4 * 5 = 80 voxels.  Plane x = 3: 16 boundary points; border: plane x = 7 (16) and the rims of x = 4, 5, 6 (36):
#             perimeter 16 + 52 = 68; bounding box (4, 3, 3).
#   shared boundary: 16 + 16 points, length ceil(32 / 2) = 16.  48 < 80: no swap, x1 is region 1.
#   merged region: 128 voxels; the pairs (1, 2) and (2, 1) cancel, the border lists unite: perimeter 28 + 52 = 80 (the rim voxels
#             of the planes x = 2 and x = 3 were boundary points and are in no list now); bounding box (7, 3, 3), box area 63.
BOXES_LITERALS = {
    "x1.area": 48.0, "x2.area": 80.0, "x1.perim": 44.0, "x2.perim": 68.0, "x0.blen": 16.0,
    "x1.bbox0": 2.0, "x1.bbox1": 3.0, "x1.bbox2": 3.0, "x1.bbox_area": 18.0, "x1.compactness": 44.0 ** 1.5 / 48.0,
    "x2.bbox0": 4.0, "x2.bbox_area": 36.0, "x2.compactness": 68.0 ** 1.5 / 80.0,
    "x3.area": 128.0, "x3.perim": 80.0, "x3.bbox0": 7.0, "x3.bbox1": 3.0, "x3.bbox2": 3.0, "x3.bbox_area": 63.0,
    "x0.area_diff": 32.0, "x0.r_area_diff0": 32.0 / 48.0, "x0.r_area_diff1": 32.0 / 80.0, "x0.perim_diff": 24.0,
    "x0.r_blen_area0": 16.0 / 48.0, "x0.r_blen_perim1": 16.0 / 68.0,
}


def ceil_f32(t):
    """smallest float32 >= t: a float32 value v is >= t exactly when v >= ceil_f32(t)"""
    f = np.float32(t)
    return f if float(f) >= t else np.nextafter(f, np.float32(np.inf))


def _q8(shape, seed):
    """multiples of 1/256, half of them multiples of 1/16: thresholds and dyadic bin bounds are hit exactly"""
    rng = np.random.default_rng(seed)
    fine, coarse = rng.integers(0, 256, shape) / 256.0, rng.integers(0, 16, shape) / 16.0
    return np.where(rng.random(shape) < 0.5, fine, coarse).astype(np.float32)


def _aux(shape, seed):
    """a second Q8 volume and a blocky integer-valued 'texton label' volume (values 0..7)"""
    rng = np.random.default_rng(seed)
    z = np.indices(shape).astype(np.float64)
    raw = 0.5 + 0.25 * np.sin(z[0] / 3.0) * np.cos(z[-1] / 4.0) + 0.2 * rng.random(shape)
    raw = (np.clip(np.round(raw * 255), 0, 255) / 256.0).astype(np.float32)
    tex = ((z[0] // 3 + 2 * (z[-1] // 5) + (z[1] // 4 if len(shape) == 3 else 0)) % 8).astype(np.float32)
    return raw, tex


def edge_values(spec, thr):
    """the float32 values at which a histogram or threshold count of (spec, thr) can change, and one far outside each end"""
    bins, lo, hi = spec
    vals = []
    for b in FD.hist_bounds(bins, lo, hi) + [lo, hi]:
        f = np.float32(b)
        vals += [f, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))]
    for t in thr:
        f = ceil_f32(t)
        vals += [f, np.nextafter(f, np.float32(-np.inf))]
    w = hi - lo
    vals += [np.float32(lo - 100.0 * w), np.float32(hi + 100.0 * w)]
    return np.unique(np.array(vals, np.float32))


def edge_image(shape, spec, thr, seed):
    """every edge value of (spec, thr) in turn, shuffled over the voxels: each occurs size / len(values) times"""
    vals = edge_values(spec, thr)
    idx = np.arange(int(np.prod(shape))) % len(vals)
    np.random.default_rng(seed).shuffle(idx)
    return vals[idx].reshape(shape).astype(np.float32)


def _pb_mean_order(labels, pb, mask=None):
    from oracle import pyoracle as O
    return O.Rag(labels, mask=mask, only_contour=True).merge_order_pb(pb, type=2)


@functools.lru_cache(maxsize=None)
def geometry(name):
    """-> (labels uint32, mask or None, order [n, 3], saliencies or None, Q8 pb)"""
    from oracle import pyoracle as O
    mask = None
    if name == "boxes":
        lab = np.ones((4, 4, 8), np.uint32); lab[:, :, 3:] = 2
        order = [[1, 2, 3]]
    elif name in ("equal_ab", "equal_ba"):           # the same two regions of 48 voxels each, given in both label orders
        lab = np.ones((4, 4, 6), np.uint32); lab[:, :, 3:] = 2
        order = [[1, 2, 3]] if name == "equal_ab" else [[2, 1, 3]]
    elif name == "not_adjacent":                     # stripes 1 | 2 | 3: first the two that do not touch
        lab = np.ones((3, 5, 9), np.uint32); lab[:, :, 3:6] = 2; lab[:, :, 6:] = 3
        order = [[1, 3, 4], [4, 2, 5]]
    elif name == "two_pieces":                       # stripes 1 | 2 | 1: one label, two components
        lab = np.ones((3, 5, 9), np.uint32); lab[:, :, 2:7] = 2
        order = [[1, 2, 3]]
    elif name == "plates":                           # one-voxel-thick plates, a one-voxel region, pairs in one direction only
        lab = np.ones((6, 7, 9), np.uint32); lab[:, :, 4:] = 2; lab[:, 3, :] = 3; lab[0, 0, 0] = 4; lab[2:4, 5:, 6:] = 7
        lab[2, 2, 4] = 5                             # its one voxel points at 1 (x-1 comes first): (3, 5) and (2, 5) have no reverse
        order = None
    elif name == "plates2d":
        lab = np.ones((9, 11), np.uint32); lab[:, 5:] = 2; lab[4, :] = 3; lab[0, 0] = 4; lab[6:8, 8:] = 7; lab[3, 5] = 5
        order = None
    elif name in ("synth3d", "masked"):
        lab, pb = O.synth((12, 14, 16), 4, 8)
        order = None
        if name == "masked":                         # about 15 % holes and a masked face
            mask = (np.random.default_rng(12).random(lab.shape) > 0.15).astype(np.uint32)
            mask[:, :, :2] = 0
    elif name == "synth2d":
        lab, pb = O.synth((20, 24), 4, 8)
        order = None
    else:
        raise KeyError(name)
    if not name.startswith("synth") and name != "masked":
        pb = _q8(lab.shape, 1 + sum(map(ord, name)))
    sal = None
    if order is None:
        order, sal = _pb_mean_order(lab, pb, mask)
    order = np.ascontiguousarray(order, np.uint32)
    for a in (lab, pb, order):
        a.setflags(write=False)
    return lab, mask, order, sal, pb


@functools.lru_cache(maxsize=None)
def definition_geometry(name, order_key=None):
    """the definition's voxel lists of a geometry (of its own order, or of the order registered under order_key)"""
    lab, mask, order, _, _ = geometry(name)
    return FD.Geometry(lab, mask, order if order_key is None else _ORDERS[order_key])


_ORDERS = {}


class Case:
    def __init__(self, name, geom, images=None, pb="pb", lists=None, thr=DEFAULT_THR, q8=True, edge=False, saliency=None, **flags):
        self.name, self.geom = name, geom
        self.labels, self.mask, self.order, self.order_sal, gpb = geometry(geom)
        self.images = {"pb": gpb}
        self.images.update({k: (gpb if v is None else v) for k, v in (images or {}).items()})   # None: the geometry's Q8 pb
        self.pb = pb
        self.lists = lists or dict(rb=[("pb", 8, 0.0, 1.0)])
        self.thr = tuple(thr)
        self.edge = edge                               # an edge-value image: the only cases whose standard-deviation columns are left out
        self.q8 = q8                                   # every image Q8 / integer valued: device == oracle bit for bit
        self.saliency = saliency                       # None or (init_sal, sal_bias): the pb-mean saliencies of the order
        self.flags = dict(norm_area=1.0, norm_len=1.0, use_log=False, use_simple=False, hist_as_feats=False, median_as_feats=False)
        self.flags.update(flags)
        self.dim = self.labels.ndim

    # ---- the three authors ----
    def _lists(self, img):
        return {k: [(img[n], b, lo, hi) for n, b, lo, hi in v] for k, v in self.lists.items()}

    def definition_rows(self, order=None, order_key=None):
        g = definition_geometry(self.geom) if order is None else self._geometry_of(order, order_key)
        kw = {}
        if self.saliency is not None:
            kw = dict(saliencies=self.order_sal, init_sal=self.saliency[0], sal_bias=self.saliency[1])
        return FD.feature_rows(g, self.images[self.pb], thresholds=self.thr, **self._lists(self.images), **self.flags, **kw)

    def _geometry_of(self, order, order_key):
        _ORDERS.setdefault(order_key, np.ascontiguousarray(order, np.uint32))
        assert (_ORDERS[order_key] == order).all()
        return definition_geometry(self.geom, order_key)

    def oracle_cfg(self):
        from oracle import pyoracle as O
        return O.make_cfg(self.images[self.pb], thr=self.thr, **self._lists(self.images), **self.flags)

    def oracle_rag(self):
        from oracle import pyoracle as O
        return O.Rag(self.labels, mask=self.mask)

    def oracle_rows(self):
        kw = {}
        if self.saliency is not None:
            kw = dict(saliencies=self.order_sal, init_sal=self.saliency[0], sal_bias=self.saliency[1])
        return self.oracle_rag().bc_feat(self.oracle_cfg(), self.order, **kw)

    def device_map(self, ctx):
        """-> hmt.RegionMap of the case (the caller closes it)"""
        import torch
        from glia_amd import hmt
        dev = {k: torch.from_numpy(np.array(v)).cuda() for k, v in self.images.items()}
        f = self.flags
        cfg = hmt.make_config(dev[self.pb], thresholds=self.thr, normalizing_area=f["norm_area"], normalizing_length=f["norm_len"],
                              use_log_shape=f["use_log"], use_simple_features=f["use_simple"],
                              use_histogram_features=f["hist_as_feats"], use_median_features=f["median_as_feats"], **self._lists(dev))
        d_lab = torch.from_numpy(np.array(self.labels).view(np.int32)).cuda()
        d_mask = None if self.mask is None else torch.from_numpy(self.mask.view(np.int32)).cuda()
        return hmt.RegionMap(ctx, d_lab, pb=dev[self.pb], mask=d_mask, cfg=cfg)

    def device_rows(self, rm):
        if self.saliency is not None:
            return rm.bc_feat(self.order, saliencies=self.order_sal, init_sal=self.saliency[0], sal_bias=self.saliency[1])
        return rm.bc_feat(self.order)

    # ---- columns ----
    def _bins(self):
        L = self.lists
        r = [b for _, b, _, _ in list(L.get("rb", [])) + list(L.get("r", []))]
        rl = [b for _, b, _, _ in L.get("rl", [])]
        bb = [b for _, b, _, _ in list(L.get("rb", [])) + list(L.get("b", []))]
        return r, rl, bb

    def columns(self):
        r, rl, bb = self._bins()
        f = self.flags
        return FD.column_names(self.dim, len(self.thr), r, rl, bb, hist_cols=f["hist_as_feats"], median_form=f["median_as_feats"],
                               saliency=self.saliency is not None and not f["use_simple"], simple=f["use_simple"])

    def feat_dim(self):
        r, rl, bb = self._bins()
        f = self.flags
        return FD.feat_dim(self.dim, len(self.thr), r, rl, bb, hist_cols=f["hist_as_feats"], median_form=f["median_as_feats"],
                           saliency=self.saliency is not None and not f["use_simple"], simple=f["use_simple"])

    def std_mask(self):
        """columns that hold a standard deviation or a difference of two: sqrt(sum of squares / n - mean^2) cancels, and what is
        left depends on the summation order wherever the squares are not exact in double (the edge-value images)"""
        return np.array([c.endswith(".std") for c in self.columns()])

    def order_dependent_mask(self):
        """median layout: mean and standard deviation come from the value vector (stats::mean, stats::var), whose order the
        reference shuffles (util/stats.hxx:87) -- comparable to 1e-12 between device and oracle, every other column bit for bit"""
        if not self.flags["median_as_feats"]:
            return np.zeros(len(self.columns()), bool)
        return np.array([c.endswith(".std") or c.endswith(".mean") for c in self.columns()])


def _build():
    B = {}

    def add(name, geom, **kw):
        assert name not in B
        B[name] = functools.partial(Case, name, geom, **kw)

    for g in ("boxes", "plates", "equal_ab", "equal_ba", "not_adjacent", "two_pieces", "plates2d", "masked", "synth3d", "synth2d"):
        add("geom/" + g, g)
    # histogram specs on the 3D synth volume, each with a Q8 / integer image and with its edge-value image; the threshold lists
    # rotate through the specs, so that every list also meets an edge-value image
    shape3 = (12, 14, 16)
    for i, (sname, spec) in enumerate(SPECS.items()):
        thr = THR_LISTS[i % len(THR_LISTS)]
        if sname in INTEGER_SPECS:
            img = _aux(shape3, 3)[1]
            thr = (0.5, 3.0, 2.5, 7.0)                           # the image is integer valued: thresholds on and between its values
        else:
            img = None
        lists = dict(rb=[("img", ) + spec])
        add("spec/%s/q8" % sname, "synth3d", images={"img": img}, pb="img",
            lists=lists, thr=thr)
        add("spec/%s/edge" % sname, "synth3d", images={"img": edge_image(shape3, spec, thr, 100 + i)}, pb="img", lists=lists,
            thr=thr, q8=False, edge=True)
    # threshold lists on the plates (Q8, thresholds hit exactly) and with edge values in 2D
    for i, thr in enumerate(THR_LISTS):
        add("thr/%d/q8" % i, "plates", thr=thr)
        add("thr/%d/edge" % i, "plates2d", images={"img": edge_image((9, 11), (8, 0.0, 1.0), thr, 200 + i)}, pb="img",
            lists=dict(rb=[("img", 8, 0.0, 1.0)]), thr=thr, q8=False, edge=True)
    # values: a constant image (one bin, entropy 0, standard deviation 0) and signed floats on a range with lo < 0
    add("values/constant", "plates", images={"img": np.full((6, 7, 9), 0.5, np.float32)}, pb="img", lists=dict(rb=[("img", 8, 0.0, 1.0)]),
        thr=(0.5, 0.75))
    gauss = np.random.default_rng(31).standard_normal(shape3).astype(np.float32)
    add("values/gaussian", "synth3d", images={"img": gauss}, pb="img", lists=dict(rb=[("img", 8, -2.0, 2.0)]), thr=(-0.5, 0.0, 1.0), q8=False)
    # layouts
    raw3, tex3 = _aux(shape3, 21)
    raw2, tex2 = _aux((20, 24), 22)
    aux3, aux2 = {"raw": raw3, "tex": tex3}, {"raw": raw2, "tex": tex2}
    rb2 = dict(rb=[("raw", 13, 0.0, 1.0), ("pb", 8, 0.0, 1.0)])
    split = dict(r=[("raw", 10, 0.1, 0.9)], b=[("pb", 8, 0.0, 1.0)], rl=[("tex", 16, -0.5, 7.5)])
    four = dict(rb=[("pb", 8, 0.0, 1.0), ("raw", 7, 0.0, 1.0)], r=[("pb", 3, 0.0, 1.0)], rl=[("tex", 8, -0.5, 7.5)])
    add("layout/log", "synth3d", use_log=True)
    add("layout/log_plates", "plates", use_log=True)             # bounding-box extents of 0: slog's dummy
    add("layout/simple", "synth3d", use_simple=True)
    add("layout/hist", "synth3d", hist_as_feats=True, lists=dict(rb=[("pb", 7, 0.0, 1.0)]), thr=(0.25, 0.75))
    add("layout/median", "synth3d", median_as_feats=True, lists=dict(rb=[("pb", 10, 0.1, 0.9)]), thr=(0.5,))
    add("layout/median_simple", "synth2d", median_as_feats=True, use_simple=True)
    add("layout/saliency", "synth3d", saliency=(0.75, 1.5))
    add("layout/saliency_log", "plates2d", saliency=(1.0, 1.0), use_log=True)
    add("layout/normalised", "synth3d", norm_area=float(12 * 14 * 16), norm_len=float((12 ** 2 + 14 ** 2 + 16 ** 2) ** 0.5))
    add("layout/rb2", "synth3d", images=aux3, lists=rb2, thr=(0.25, 0.75))
    add("layout/split", "synth3d", images=aux3, lists=split, thr=(0.125, 0.25, 0.5, 0.75))
    add("layout/four", "synth3d", images=aux3, lists=four, thr=())
    add("layout/split_hist_2d", "synth2d", images=aux2, lists=split, thr=(0.5, 0.5), hist_as_feats=True)
    add("layout/four_median", "masked", images=aux3, lists=four, thr=(0.8, 0.2, 0.5), median_as_feats=True)
    add("layout/rb2_simple_log", "synth2d", images=aux2, lists=rb2, thr=(0.5,), use_simple=True, use_log=True)
    return B


_BUILDERS = _build()                                            # needs no oracle: cases are built on first use
NAMES = list(_BUILDERS)
SPEC_AND_THR_NAMES = [n for n in NAMES if n.startswith("spec/") or n.startswith("thr/")]
LOOP_NAMES = ["geom/synth3d", "geom/synth2d", "layout/split"]       # cases whose rows also come out of the classifier merge loop


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def definition_rows(name):
    """computed once per session, shared by the tests that need it, never written to"""
    rows = case(name).definition_rows()
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    rows = case(name).oracle_rows()
    rows.setflags(write=False)
    return rows
