"""Wide contractions of the classifier loop (glia_amd/csrc/greedy_bc.hip) and of the median, median x min-size and pre_merge linkages
(greedy_tree.hpp, greedy_window.hpp) on the hub images of tests/_hub_cases.py.

The classifier loop treats a contraction by `total`, the list entries of the two merged regions, and `newcount`, the records of the
new one:
    total > 512          the later passes of phase B read their list entry again (the first pass keeps it in registers)
    total > 1408         neighbour matching on the global mark arrays instead of the LDS table
    newcount > 96        several scoring rounds per contraction (W.cap <= 96); a helper job of hundreds to thousands of records
    newcount > ldsCap    category and extremes of a new record come back from global memory (2252 records with four channels)
Compact supervoxels reach none of these, and the oracle cannot follow where they are reached (its loop re-scores from voxel lists: nine
minutes are not enough for 1801 regions).  The expected order here comes from tests/_loopdef.py, the loop under a one-column scorer
stated a second time and held to the oracle in tests/test_loop_definition.py: the stub scorer 1 - x[31] (x0.b0.mean), or a forest of
255 stumps on that column, whose score is a step function of the same mean -- so the forest route (helper workgroups, votes) has an
exact reference too, ties included.

That the widths are reached is proven from the replayed order (test_width_classes_are_hit, no GPU needed), counted as
_hub_cases.width_classes counts: the live table neighbours of the two regions are a LOWER bound of `total`; the list lengths by the
kernel's rule -- a region's list is created with one entry per region it touches (mutual contact or not) and never changes its length:
when a neighbour is merged away its entry is reused in place for the new region, or dies when the neighbour touched both merged
regions -- are `total` itself, and have to be kMargin below a class's upper edge.  The new table edges are a lower bound of newcount.

The other linkages are compared with the oracle directly (0.5 s and 3 s of oracle time at 1801 regions).  Everything is Q8, every
comparison bit for bit."""
import os
import tempfile

import numpy as np
import pytest

import _featdef
import _loopdef
import _rf
from _hub_cases import CLASSES, hub_image, kMargin, thin_hub_image, width_classes

STUB = 11 + 4 * 3 + 7 + 1          # x0.b0.mean
kCap, kLdsCap4 = 96, 2252          # W.cap's limit; kWsBytes / (8 + 8 K) at K = 4
def _narrow_hub(grid):
    """hub_image(None, grid) with the hub's own pixels pressed into [0.25, 0.75): on random Q8 values the extremes of a boundary of
    thousands of pixels are 0 and 255/256 from either side, so a contraction that took the neighbours' extremes for the hub's, or lost
    some, would go unnoticed; here the hub's side differs from every blob's"""
    lab, pb = hub_image(None, grid=grid)
    return lab, np.where(lab == 1, (np.floor(pb * 128) + 64) / 256, pb).astype(np.float32)


IMAGES = {"hub": lambda: hub_image(None), "hub4": lambda: hub_image(4), "hub36": lambda: hub_image(None, grid=36), "hub36n": lambda: _narrow_hub(36),
          "thin30": lambda: thin_hub_image(30), "thin30_4": lambda: thin_hub_image(30, 4)}
BC_CLASSES = ("several rounds, one pass", "two or three passes", "global marks", "beyond ldsCap (K = 4)")
_cpu, _dev = {}, {}


def _image(name):
    if ("img", name) not in _cpu:
        lab, pb = IMAGES[name]()
        _cpu["img", name] = (lab, pb)
        _cpu["leaves", name] = _loopdef.leaf_pairs(lab, pb)
    return _cpu["img", name]


def _check(name, o, s):
    lab, pb = _image(name)
    return _loopdef.check(lab, pb, o, s, explain=True, leaves=_cpu["leaves", name])


def _stumps(pb):
    """255 thresholds ascending over the image's value range"""
    return np.linspace(float(pb.min()), float(pb.max()), 257)[1:-1]


def _reference(name, forest=False):
    """generate() and stats() of an image under the stub or the stump forest, computed once"""
    key = ("ref", name, forest)
    if key not in _cpu:
        lab, pb = _image(name)
        F = _loopdef.stump_forest_score(_stumps(pb)) if forest else None
        _cpu[key] = _loopdef.generate(lab, pb, F=F, leaves=_cpu["leaves", name], want_stats=True) + (F,)
    return _cpu[key]


def _bc_hits(st):
    lower, total = st["tab0"] + st["tab1"], st["len0"] + st["len1"]
    assert (lower <= total).all()
    return [int(((total <= 512 - kMargin) & (st["new_edges"] > kCap + kMargin)).sum()),
            int(((lower >= 513) & (total <= 1408 - kMargin)).sum()), int((lower >= 1409).sum()),
            int((st["new_edges"] > kLdsCap4 + kMargin).sum())]


@pytest.mark.parametrize("name,forest", [("hub", False), ("hub4", False), ("hub", True), ("hub4", True), ("hub36", False), ("hub36", True),
                                         ("hub36n", False)])
def test_width_classes_are_hit(name, forest):
    o, s, st, _ = _reference(name, forest)
    lab, _ = _image(name)
    assert len(o) == len(np.unique(lab)) - 1
    hits = _bc_hits(st)
    print("%s, %s: %s; largest total %d, largest newcount %d"
          % (name, "stump forest" if forest else "stub", ", ".join("%s %d" % p for p in zip(BC_CLASSES, hits)),
             int((st["len0"] + st["len1"]).max()), int(st["new_records"].max())))
    for cls, h in list(zip(BC_CLASSES, hits))[:4 if name.startswith("hub36") else 3]:
        assert h >= 20, (cls, h)
    if name == "hub4" or forest:      # exact ties: the insertion order decides most of the order
        assert len(np.unique(s)) * 2 < len(o)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    c.close()
    _dev.clear()


def _aux(shape):
    """two more Q8 / integer images for the four-channel layout"""
    rng = np.random.default_rng(36)
    raw = (rng.integers(0, 256, shape) / 256.0).astype(np.float32)
    y, x = np.indices(shape)
    tex = ((y // 3 + 2 * (x // 5)) % 7).astype(np.float32)
    return raw, tex


def _tensors(name):
    if name not in _dev:
        import torch
        lab, pb = _image(name)
        raw, tex = _aux(lab.shape)
        _dev[name] = (torch.from_numpy(lab.view(np.int32)).cuda(),) + tuple(torch.from_numpy(a).cuda() for a in (pb, raw, tex))
    return _dev[name]


def _rm(ctx, name, four=False):
    """one image (the common configuration) or four distinct (volume, histogram) channels; column 31 is x0.b0.mean of pb in both"""
    from glia_amd import hmt
    d_lab, d_pb, d_raw, d_tex = _tensors(name)
    if four:
        cfg = hmt.make_config(d_pb, rb=[(d_pb, 8, 0.0, 1.0)], b=[(d_raw, 8, 0.0, 1.0), (d_tex, 8, -0.5, 7.5), (d_pb, 4, 0.0, 1.0)])
        names = _featdef.column_names(2, 3, [8], [], [8, 8, 8, 4])
    else:
        cfg = hmt.make_config(d_pb, rb=[(d_pb, 8, 0.0, 1.0)])
        names = _featdef.column_names(2, 3, [8], [], [8])
    rm = hmt.RegionMap(ctx, d_lab, pb=d_pb, cfg=cfg)
    assert rm.num_channels() == (4 if four else 1) and rm.feat_dim() == len(names) and names[STUB] == "x0.b0.mean"
    return rm


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _rows_are(f, o, route, n_leaf):
    """The rows the loop scored the popped edges with against the rows `route` (bc_feat / bc_feat_batch of the same map) makes for the
    same order, bit for bit.  One freedom is the reference's own: the two regions trade places only when the first is STRICTLY larger
    (main_merge_order_bc.cxx:77-80, main_bc_feat.cxx:85-89), so on equal areas the loop's row keeps the orientation its edge was created
    with -- for an initial edge the region map's iteration order -- while bc_feat takes (x0, x1) as given.  Such a row must then be the
    row of the swapped pair, and only a merge of two leaves of equal area may be one (on the hub image: 105 of the 320 sibling merges)."""
    names = next(n for n in (_featdef.column_names(2, 3, [8], [], b) for b in ([8], [8, 8, 8, 4])) if len(n) == f.shape[1])
    a1, a2 = names.index("x1.area"), names.index("x2.area")
    r = route(o)
    assert f.shape == r.shape
    bad = ~(_bits(f) == _bits(r)).all(1)
    if bad.any():
        swapped = o.copy()
        swapped[:, [0, 1]] = o[:, [1, 0]]
        assert (_bits(f[bad]) == _bits(route(swapped)[bad])).all()
        assert (f[bad, a1] == f[bad, a2]).all() and (o[bad, :2] <= n_leaf).all()
    return int(bad.sum())


def _same(got, ref):
    return got[0].shape == ref[0].shape and (got[0] == ref[0]).all() and (_bits(got[1]) == _bits(ref[1])).all()


def _stump_forest(ctx, pb):
    """tree i: x[31] <= t_i -> the leaf of class 1 (label -1, the predicted one), else class 2"""
    thr = _stumps(pb)
    n = len(thr)
    forest = dict(xbestsplit=np.zeros((n, 3)), treemap=np.zeros((n, 3, 2), np.int32), nodestatus=np.full((n, 3), -1, np.int32),
                  nodeclass=np.zeros((n, 3), np.int32), bestvar=np.zeros((n, 3), np.int32), ndbigtree=np.full(n, 3, np.int32),
                  orig_labels=np.array([-1, 1], np.int32))
    forest["xbestsplit"][:, 0] = thr
    forest["treemap"][:, 0] = (2, 3)
    forest["nodestatus"][:, 0] = 1
    forest["bestvar"][:, 0] = STUB + 1
    forest["nodeclass"][:, 1], forest["nodeclass"][:, 2] = 1, 2
    return _load(ctx, forest)


def _load(ctx, forest):
    from glia_amd import hmt
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "model.bin")
        _rf.write_model(path, forest)
        return hmt.RandomForest(ctx, path, predict_label=-1)


def _stub_run(ctx, name, four=False):
    """the default instance's (order, saliencies, rows) on an image, once"""
    key = ("stub", name, four)
    if key not in _dev:
        from glia_amd import hmt
        rm = _rm(ctx, name, four)
        _dev[key] = rm.merge_order_bc(hmt.FeatureStubClassifier(ctx, STUB), want_feats=True)
        rm.close()
    return _dev[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hub", "hub4"])
def test_stub_loop_on_the_hub_image(ctx, name):
    """order and saliencies are generate()'s and pass check(); the rows the loop scored the popped edges with are the rows two other
    kernels make of the same map for that order"""
    from glia_amd import hmt
    lab, pb = _image(name)
    ref = _reference(name)
    before = hmt.Context.internal_errors()
    o, s, f = _stub_run(ctx, name)
    assert _check(name, o, s) == (-1, "")
    assert _same((o, s), ref)
    rm = _rm(ctx, name)
    assert f.shape == (len(o), rm.feat_dim())
    assert _rows_are(f, o, rm.bc_feat, int(lab.max())) == _rows_are(f, o, rm.bc_feat_batch, int(lab.max()))
    assert (_bits(1.0 - f[:, STUB]) == _bits(s)).all()
    rm.close()
    assert hmt.Context.internal_errors() == before == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hub", "hub4"])
@pytest.mark.parametrize("env", [dict(GLIA_HMT_BC_NOCOMMON=1), dict(GLIA_HMT_BC_GENERIC=1), dict(GLIA_HMT_MINCAP=1)])
def test_stub_loop_instances_and_smallest_capacities(ctx, name, env):
    from glia_amd import hmt
    ref = _reference(name)
    o0, s0, f0 = _stub_run(ctx, name)
    before = hmt.Context.internal_errors()
    with hmt.options(**env):
        rm = _rm(ctx, name)
        o, s, f = rm.merge_order_bc(hmt.FeatureStubClassifier(ctx, STUB), want_feats=True)
        rm.close()
    assert _same((o, s), ref), env
    assert f.shape == f0.shape and (_bits(f) == _bits(f0)).all(), env
    assert hmt.Context.internal_errors() == before == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hub", "hub4"])
def test_stump_forest_on_the_helper_route(ctx, name):
    """a real forest (clf.kind == 0): jobs of up to 1800 records for the helper workgroups, every count of them, and the loop's own
    workgroup walking the trees (0) -- all equal to generate() under the forest's step function"""
    from glia_amd import hmt
    _, pb = _image(name)
    ref = _reference(name, forest=True)
    clf = _stump_forest(ctx, pb)
    before = hmt.Context.internal_errors()
    rm = _rm(ctx, name)
    o, s, f = rm.merge_order_bc(clf, want_feats=True)
    assert _same((o, s), ref), "default helpers"
    assert (_bits(s) == _bits(clf.predict(f))).all()
    assert (_bits(s) == _bits(ref[3](f[:, STUB]))).all()
    for nh in (5, 0):
        with hmt.options(GLIA_HMT_HELPERS=nh):
            assert _same(rm.merge_order_bc(clf), ref), "helpers = %d" % nh
    rm.close()
    clf.close()
    assert hmt.Context.internal_errors() == before == 0


@pytest.mark.gpu
def test_random_forest_on_the_helper_route(ctx):
    """63 trees of depth 7 over all columns: no CPU reference at this size -- the helper counts agree with each other, the saliencies
    are the forest's values of the returned rows, and the rows are the batch kernel's for the returned order"""
    from glia_amd import hmt
    _, _, f0 = _stub_run(ctx, "hub")
    clf = _load(ctx, _rf.random_forest(np.random.default_rng(63), 63, 7, f0))
    before = hmt.Context.internal_errors()
    rm = _rm(ctx, "hub")
    o, s, f = rm.merge_order_bc(clf, want_feats=True)
    assert len(o) == 1800 and len(np.unique(s)) > 8
    for nh in (5, 0):
        with hmt.options(GLIA_HMT_HELPERS=nh):
            assert _same(rm.merge_order_bc(clf), (o, s)), "helpers = %d" % nh
    assert (_bits(s) == _bits(clf.predict(f))).all()
    _rows_are(f, o, rm.bc_feat_batch, 1801)
    rm.close()
    clf.close()
    assert hmt.Context.internal_errors() == before == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hub36", "hub36n"])
def test_stub_loop_beyond_lds_cap(ctx, name):
    """216 x 216, 2593 regions, four channels: the hub's first contractions create more than 2252 records; hub36n: the hub's extremes
    differ from its neighbours' (see _narrow_hub), so the rows notice whose extremes the top-two pass read"""
    from glia_amd import hmt
    lab, pb = _image(name)
    ref = _reference(name)
    assert _bc_hits(ref[2])[3] >= 20
    before = hmt.Context.internal_errors()
    o, s, f = _stub_run(ctx, name, four=True)
    assert _check(name, o, s) == (-1, "")
    assert _same((o, s), ref)
    rm = _rm(ctx, name, four=True)
    assert _rows_are(f, o, rm.bc_feat, int(lab.max())) == _rows_are(f, o, rm.bc_feat_batch, int(lab.max()))
    rm.close()
    assert hmt.Context.internal_errors() == before == 0


@pytest.mark.gpu
def test_stump_forest_beyond_lds_cap(ctx):
    from glia_amd import hmt
    _, pb = _image("hub36")
    ref = _reference("hub36", forest=True)
    assert _bc_hits(ref[2])[3] >= 20
    clf = _stump_forest(ctx, pb)
    before = hmt.Context.internal_errors()
    rm = _rm(ctx, "hub36", four=True)
    o, s, f = rm.merge_order_bc(clf, want_feats=True)
    assert _same((o, s), ref)
    assert (_bits(s) == _bits(clf.predict(f))).all()
    with hmt.options(GLIA_HMT_HELPERS=5):
        assert _same(rm.merge_order_bc(clf), ref), "helpers = 5"
    rm.close()
    clf.close()
    assert hmt.Context.internal_errors() == before == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["thin30", "thin30_4"])
def test_stub_loop_on_the_thin_hub_image(ctx, name):
    """mostly non-mutual contact: 1801 regions, 900 merges; the hub's records with the right halves carry the fragile entries"""
    from glia_amd import hmt
    lab, pb = _image(name)
    ref = _reference(name)
    st = ref[2]
    print("%s: %d merges of %d regions, largest fragile-pair count on one record %d, largest total %d, largest newcount %d"
          % (name, len(ref[0]), len(np.unique(lab)), int(st["fragile"].max()), int((st["len0"] + st["len1"]).max()), int(st["new_records"].max())))
    assert len(ref[0]) == 900 and st["fragile"].max() >= 1 and (st["len0"] + st["len1"]).max() > 1408
    before = hmt.Context.internal_errors()
    o, s, f = _stub_run(ctx, name)
    assert _check(name, o, s) == (-1, "")
    assert _same((o, s), ref)
    rm = _rm(ctx, name)
    assert _rows_are(f, o, rm.bc_feat, int(lab.max())) == _rows_are(f, o, rm.bc_feat_batch, int(lab.max()))
    rm.close()
    assert hmt.Context.internal_errors() == before == 0


# ---- the other linkages, against the oracle ----------------------------------------------------------------------------------------
kSizes, kRpb = [7, 13], 0.5        # a half has 6 pixels, a blob 12: the hub takes every half whose sibling it reaches first; a blob whose
#                                    halves met first stays out unless its mean pb is above 0.5


def _oracle(name, kind):
    key = ("oracle", name, kind)
    if key not in _cpu:
        from oracle import pyoracle as O
        lab, pb = _image(name)
        if kind == "type1":
            _cpu[key] = O.Rag(lab, only_contour=True).merge_order_pb(pb, type=1)
        elif kind == "type3":
            _cpu[key] = O.Rag(lab, only_contour=False).merge_order_pb(pb, type=3, update_region=True)
        else:
            _cpu[key] = O.Rag(lab).pre_merge(pb, kSizes, kRpb)
    return _cpu[key]


def _pb_run(ctx, name, kind, **env):
    from glia_amd import hmt
    d_lab, d_pb, _, _ = _tensors(name)
    with hmt.options(**env):
        rm = hmt.RegionMap(ctx, d_lab, pb=d_pb, only_contour=kind == "type1")
        out = rm.pre_merge(kSizes, kRpb) if kind == "pre_merge" else rm.merge_order_pb(type=int(kind[-1]))
        rm.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hub", "hub4"])
@pytest.mark.parametrize("kind,env", [("type1", {}), ("type1", dict(GLIA_HMT_MINCAP=1)), ("type3", {}), ("pre_merge", {}),
                                      ("pre_merge", dict(GLIA_HMT_WINCAP=32)), ("pre_merge", dict(GLIA_HMT_REBASE=200))])
def test_other_linkages_on_the_hub_image(ctx, name, kind, env):
    from glia_amd import hmt
    lab, _ = _image(name)
    ref = _oracle(name, kind)
    hits = width_classes(lab, ref[0], complete=kind != "pre_merge")
    assert hits[0] >= 20, "merges wider than 1408 entries"
    if kind == "pre_merge":
        assert 0 < len(ref[0]) < len(np.unique(lab)) - 2, "the condition stops the loop early"
    else:
        assert all(h >= 20 for h in hits), list(zip([c[0] for c in CLASSES], hits))
    before = hmt.Context.internal_errors()
    got = _pb_run(ctx, name, kind, **env)
    assert _same(got, ref), (kind, env)
    assert hmt.Context.internal_errors() == before == 0
