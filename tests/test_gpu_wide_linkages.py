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

Two more caps have images of their own (tests/_hub_cases.py; small instances of both are held to the oracle in
tests/test_loop_definition.py):
    the fragile comb (2202 regions)   one record, hub-Y, with a chain of 1100 fragile leaf entries of which half are dead when its edge
        pops.  A helper's last wave walks the chains of a chunk's (record, channel) pairs into ONE LDS work list of kFragCap = 4096
        entries: with four channels 4400 entries, two batches (the full list, the entry that opens the next batch, the accumulators
        carried over); with one channel a long chain inside one batch.  Under the stub scorer the loop's own workgroup walks the
        chain serially.  ysplit = 2: two records with chains of 550.
    the touching comb (16 606 regions, 410 merges)   `total` falls by one per merge from 16 607 to 16 198, across kJobMax = 16 384:
        the first 223 contractions are too large for a helper job and are scored by the loop's own workgroup, the others go to the
        helpers -- one run that changes the route; every contraction has more than 16 000 list entries and new records.
test_fragile_chains_and_job_sizes_are_reached proves these sizes from the replay.

The other linkages are compared with the oracle directly (0.5 s and 3 s of oracle time at 1801 regions).  Everything is Q8, every
comparison bit for bit -- but for comb32, the fragile comb with a float32 jitter, on which the loop is compared with itself under
every setting and with clf.predict of its own rows (the section "one association" below), bit for bit as well."""
import os
import tempfile

import numpy as np
import pytest

import _featdef
import _loopdef
import _rf
from _hub_cases import CLASSES, fragile_comb_image, fragile_comb_image_f32, hub_image, kMargin, thin_hub_image, touching_comb_image, width_classes

STUB = 11 + 4 * 3 + 7 + 1          # x0.b0.mean
kCap, kLdsCap4 = 96, 2252          # W.cap's limit; kWsBytes / (8 + 8 K) at K = 4
kFragCap, kHelpChunk, kJobMax = 4096, 8, 16384      # greedy_bc.hip, greedy_bc_state.hpp: work-list entries per batch; records per helper round; records per job
kCombN, kCombY = 1100, 2           # fragile comb: cells (chain entries of hub-Y), Y's label


def _narrow_hub(grid):
    """hub_image(None, grid) with the hub's own pixels pressed into [0.25, 0.75): on random Q8 values the extremes of a boundary of
    thousands of pixels are 0 and 255/256 from either side, so a contraction that took the neighbours' extremes for the hub's, or lost
    some, would go unnoticed; here the hub's side differs from every blob's"""
    lab, pb = hub_image(None, grid=grid)
    return lab, np.where(lab == 1, (np.floor(pb * 128) + 64) / 256, pb).astype(np.float32)


IMAGES = {"hub": lambda: hub_image(None), "hub4": lambda: hub_image(4), "hub36": lambda: hub_image(None, grid=36), "hub36n": lambda: _narrow_hub(36),
          "thin30": lambda: thin_hub_image(30), "thin30_4": lambda: thin_hub_image(30, 4),
          "comb": lambda: fragile_comb_image(kCombN), "comb32": lambda: fragile_comb_image_f32(kCombN), "comb2": lambda: fragile_comb_image(kCombN, ysplit=2),
          "tcomb": lambda: touching_comb_image(41, 10, 40, 39)}
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


def _pop_of(name, forest, y=kCombY):
    """(step, chain entries, alive ones) of the edge that merges Y away in the reference order"""
    key = ("pop", name, forest, y)
    if key not in _cpu:
        lab, pb = _image(name)
        _cpu[key] = _loopdef.chain_at_pop(lab, pb, _reference(name, forest)[0], y, leaves=_cpu["leaves", name])
    return _cpu[key]


@pytest.mark.parametrize("name,forest", [("comb", False), ("comb", True), ("comb2", True), ("tcomb", False), ("tcomb", True)])
def test_fragile_chains_and_job_sizes_are_reached(name, forest):
    """what the replay proves about the images of the two caps.  A chain's entries are the fragile pairs on one record, dead or alive
    (stats()["fragile"]): a helper's lane walks all of them, once per channel, and aliveness is decided from the list."""
    o, s, st, _ = _reference(name, forest)
    lab, _ = _image(name)
    which = "%s, %s" % (name, "stump forest" if forest else "stub")
    if name == "tcomb":
        total = st["len0"] + st["len1"]
        above, below = total > kJobMax, total <= kJobMax - kMargin
        print("%s: %d merges of %d regions, total %d .. %d: %d merges above kJobMax, %d at least kMargin below; fewest new records %d"
              % (which, len(o), len(np.unique(lab)), int(total.max()), int(total.min()), int(above.sum()), int(below.sum()), int(st["new_records"].min())))
        assert len(o) == 410 and above.sum() >= 100 and below.sum() >= 100
        assert above[:int(above.sum())].all() and below[-int(below.sum()):].all(), "one order, the large ones first"
        assert st["new_records"].min() > 16000 and st["new_edges"].max() <= 409
        return
    assert len(o) == len(np.unique(lab)) - 1
    K = 4
    two = st["fragile"] * K > kFragCap + kHelpChunk * 4        # the other records of the chunk add entries to the list too
    inside = (st["fragile"] > 256) & (st["fragile"] + kHelpChunk <= kFragCap)        # K = 1
    pops = [_pop_of(name, forest, y) for y in ((2, 3) if name == "comb2" else (kCombY,))]
    print("%s: largest fragile count on one record %d; %d merges with more than (kFragCap + 32) / 4 = 1032; hub-Y pops at %s, distinct saliencies %d"
          % (which, int(st["fragile"].max()), int(two.sum()),
             ", ".join("step %d with %d of %d entries alive" % (p[0], p[2], p[1]) for p in pops), len(np.unique(s))))
    if name == "comb":
        step, n, alive = pops[0]
        assert two.sum() >= 20 and inside.sum() >= 20
        assert n == kCombN > 1024 and n * K > kFragCap + kHelpChunk * 4
        assert n <= 4 * alive <= 3 * n, "a quarter to three quarters of the chain alive at the pop"
        assert two[step - 1], "the record that pops was scored with the long chain"
    else:
        assert all(p[1] == kCombN // 2 and 0 < p[2] < p[1] for p in pops)


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


def _stump_arrays(stumps):
    """forest arrays of one stump per (column, threshold, votes_on_le): it votes for the predicted label (-1) on x[column] <= threshold,
    or on x[column] > threshold.  [(STUB, t, True) for t in _stumps(pb)] is _stump_forest's."""
    n = len(stumps)
    forest = dict(xbestsplit=np.zeros((n, 3)), treemap=np.zeros((n, 3, 2), np.int32), nodestatus=np.full((n, 3), -1, np.int32),
                  nodeclass=np.zeros((n, 3), np.int32), bestvar=np.zeros((n, 3), np.int32), ndbigtree=np.full(n, 3, np.int32),
                  orig_labels=np.array([-1, 1], np.int32))
    for i, (col, thr, le) in enumerate(stumps):
        forest["xbestsplit"][i, 0], forest["treemap"][i, 0], forest["nodestatus"][i, 0], forest["bestvar"][i, 0] = thr, (2, 3), 1, col + 1
        forest["nodeclass"][i, 1:] = (1, 2) if le else (2, 1)
    return forest


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


HELPERS = [None, 5, 0]            # the default (one per compute unit left), a few, none: the loop's own workgroup walks trees and chains


def _forest_run(ctx, name, four, helpers, routes):
    """the stump forest on `name`: order and saliencies are the replay's, s == clf.predict(f), the popped rows are the rows of
    `routes` (attribute names of the map)"""
    from glia_amd import hmt
    lab, pb = _image(name)
    ref = _reference(name, forest=True)
    clf = _stump_forest(ctx, pb)
    before = hmt.Context.internal_errors()
    rm = _rm(ctx, name, four)
    with hmt.options(**({} if helpers is None else dict(GLIA_HMT_HELPERS=helpers))):
        o, s, f = rm.merge_order_bc(clf, want_feats=True)
    assert _loopdef.check(lab, pb, o, s, F=ref[3], explain=True, leaves=_cpu["leaves", name]) == (-1, "")
    assert _same((o, s), ref)
    assert (_bits(s) == _bits(clf.predict(f))).all()
    assert (_bits(s) == _bits(ref[3](f[:, STUB]))).all()
    assert len({_rows_are(f, o, getattr(rm, r), int(lab.max())) for r in routes}) == 1
    rm.close()
    clf.close()
    assert hmt.Context.internal_errors() == before == 0


def _stub_run_checked(ctx, name, four, routes, **env):
    from glia_amd import hmt
    lab, _ = _image(name)
    ref = _reference(name)
    before = hmt.Context.internal_errors()
    with hmt.options(**env):
        rm = _rm(ctx, name, four)
        o, s, f = rm.merge_order_bc(hmt.FeatureStubClassifier(ctx, STUB), want_feats=True)
    assert _check(name, o, s) == (-1, "")
    assert _same((o, s), ref)
    assert (_bits(1.0 - f[:, STUB]) == _bits(s)).all()
    assert len({_rows_are(f, o, getattr(rm, r), int(lab.max())) for r in routes}) == 1
    rm.close()
    assert hmt.Context.internal_errors() == before == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,helpers", [("comb", h) for h in HELPERS] + [("comb2", None)])
def test_stump_forest_on_a_fragile_chain_of_two_batches(ctx, name, helpers):
    """four channels: the 1100 entries of hub-Y are walked by four lanes into a list of 4096 -- the list fills, the wave goes round a
    second time with the accumulators carried over, and more than a third of the entries are dead when the edge pops (comb2: two
    chains of 550).  Of a helper's accumulators the saliency sees the count and the sum of one channel (the others:
    test_every_accumulator_of_a_chain_of_two_batches); the popped rows are the work of the loop's own workgroup, which walks the
    chain one lane per channel -- as it does for every record when there are no helpers."""
    step, n, alive = _pop_of(name, True)
    assert n * 4 > kFragCap + kHelpChunk * 4 or name == "comb2"
    assert 0 < alive < n
    _forest_run(ctx, name, True, helpers, ("bc_feat", "bc_feat_batch"))


def _mixed_forest(ctx, pb, rows, nrandom):
    """the 255 stumps on x0.b0.mean, which shape the order (the X_i first, hub-Y among the V_i), and `nrandom` trees of depth 7 over
    ALL columns of `rows`"""
    thr = _stumps(pb)
    rnd = _rf.random_forest(np.random.default_rng(63), nrandom, 7, rows)
    n, m = len(thr), rnd["xbestsplit"].shape[1]
    stumps = {k: np.zeros((n,) + v.shape[1:], v.dtype) for k, v in rnd.items() if k not in ("ndbigtree", "orig_labels")}
    stumps["xbestsplit"][:, 0] = thr
    stumps["treemap"][:, 0] = (2, 3)
    stumps["nodestatus"][:, 0], stumps["nodestatus"][:, 1:3] = 1, -1
    stumps["bestvar"][:, 0] = STUB + 1
    stumps["nodeclass"][:, 1], stumps["nodeclass"][:, 2] = 1, 2
    forest = {k: np.concatenate([v, rnd[k]]) for k, v in stumps.items()}
    forest["ndbigtree"] = np.concatenate([np.full(n, 3, np.int32), rnd["ndbigtree"]])
    forest["orig_labels"] = rnd["orig_labels"]
    assert m >= 3
    return _load(ctx, forest)


@pytest.mark.gpu
def test_every_accumulator_of_a_chain_of_two_batches(ctx):
    """The stump forest reads ONE column, the mean of one channel's sums; and the popped rows are no witness of a helper's work: the
    loop's own workgroup makes the row of the edge it pops, walking the chain itself.  So the helpers' histogram, threshold, extreme
    and square accumulators of the four channels are seen by nothing above.  Here 48 trees over all columns vote beside the stumps.
    No replay knows their votes; the witness is clf.predict() of the popped rows: the saliency hub-Y pops with is the helpers' vote
    on their vector, from a work list of two batches, the row is the loop's own serial walk of the same chain.  That hub-Y was
    scored on more than 1032 entries, and popped part dead, is read off the returned order.  (A run without helpers would be a
    witness of every re-scoring on the way to the pop, through the order, but takes 12 s: the serial walk is slow.)"""
    from glia_amd import hmt
    lab, pb = _image("comb")
    before = hmt.Context.internal_errors()
    rm = _rm(ctx, "comb", four=True)
    clf = _mixed_forest(ctx, pb, rm.bc_feat_batch(_reference("comb", forest=True)[0]), 48)
    o, s, f = rm.merge_order_bc(clf, want_feats=True)
    st = _loopdef.stats(lab, pb, order=o, leaves=_cpu["leaves", "comb"])
    step, n, alive = _loopdef.chain_at_pop(lab, pb, o, kCombY, leaves=_cpu["leaves", "comb"])
    two = st["fragile"] * 4 > kFragCap + kHelpChunk * 4
    print("mixed forest: hub-Y pops at step %d with %d of %d entries alive; %d merges with more than 1032 fragile entries on one record; "
          "distinct saliencies %d" % (step, alive, n, int(two.sum()), len(np.unique(s))))
    assert len(o) == 2 * kCombN + 1 and n * 4 > kFragCap + kHelpChunk * 4 and two[step - 1] and two.sum() >= 20
    assert 0 < alive < n
    assert (_bits(s) == _bits(clf.predict(f))).all()
    votes = s * (255 + 48) - 255 * _reference("comb", forest=True)[3](f[:, STUB])
    assert np.abs(votes - np.round(votes)).max() < 1e-9 and len(np.unique(np.round(votes))) > 8, "the random trees take part"
    _rows_are(f, o, rm.bc_feat_batch, int(lab.max()))
    rm.close()
    clf.close()
    assert hmt.Context.internal_errors() == before == 0


@pytest.mark.gpu
def test_stub_loop_on_a_fragile_chain(ctx):
    """the loop's own workgroup: one lane per (record, channel) walks the 1100 entries serially"""
    _stub_run_checked(ctx, "comb", True, ("bc_feat", "bc_feat_batch"))


@pytest.mark.gpu
@pytest.mark.parametrize("helpers", HELPERS + ["stub", "stub, smallest capacities"])
def test_fragile_chain_inside_one_batch(ctx, helpers):
    """one channel: 1100 entries of 4096.  The stub's serial walk takes a quarter of the four-channel one's time here, so this is where
    it runs once more with GLIA_HMT_MINCAP=1 (the arrays grow, and the kernel is launched again, while the chain is being built)"""
    if isinstance(helpers, str):
        _stub_run_checked(ctx, "comb", False, ("bc_feat", "bc_feat_batch"), **(dict(GLIA_HMT_MINCAP=1) if "smallest" in helpers else {}))
    else:
        _forest_run(ctx, "comb", False, helpers, ("bc_feat", "bc_feat_batch"))


@pytest.mark.gpu
@pytest.mark.parametrize("helpers", HELPERS)
def test_stump_forest_across_job_max(ctx, helpers):
    """the touching comb: 223 contractions of more than kJobMax list entries scored by the loop's own workgroup, then 187 helper jobs of
    16 000 rows (of which the table edges, at most 409, are scored) -- the job sequence, the vote slots and the rows start in the
    middle of a run"""
    st = _reference("tcomb", forest=True)[2]
    total = st["len0"] + st["len1"]
    assert (total > kJobMax).sum() >= 100 and (total <= kJobMax - kMargin).sum() >= 100
    _forest_run(ctx, "tcomb", False, helpers, ("bc_feat_batch",))


@pytest.mark.gpu
def test_stub_loop_on_the_touching_comb(ctx):
    """contractions of 16 000 list entries on the global mark arrays, 16 000 new records each"""
    _stub_run_checked(ctx, "tcomb", False, ("bc_feat_batch",))


# ---- one association of the fragile entries' sums, on a float32 image ---------------------------------------------------------------
# include/glia_hmt.h: "No setting changes a result."  On Q8 images every f64 sum is exact and no order of additions can show.  comb32
# is the fragile comb with a float32 jitter (_hub_cases.fragile_comb_image_f32): hub-Y pops on a chain of 1100 entries, half alive,
# whose squares do not add exactly.  The loop's own workgroup folds the alive entries one by one onto the mutual entries' sums; the
# rule ("One association") is that a helper does the same.  A vote is an integer, so a last-bit difference shows only if
# a split sits on it: four stumps are put AROUND the value the loop's own row holds for hub-Y's pop (_witness_stumps).
kBand = 64                         # ulps on either side of the value inside which a different association is seen
WITNESS_ENVS = [dict(), dict(GLIA_HMT_HELPERS=5), dict(GLIA_HMT_BC_NOCOMMON=1), dict(GLIA_HMT_BC_GENERIC=1), dict(GLIA_HMT_MINCAP=1)]


def _ulps(v, d):
    """the double d ulps above (below) the positive double v"""
    return float((np.array([v], np.float64).view(np.int64) + d).view(np.float64)[0])


def _witness_stumps(v, col, k=kBand):
    """four stumps on column col that vote 2 everywhere, and 3 within k ulps of v but not AT v: x <= pred(v), x > v - (k + 1) ulp,
    x > v, x <= v + k ulp.  Added to a forest F0 they make F1 = a monotone map of F0's votes (v0 -> (v0 + 2) / (n + 4)) for every
    record that is not within k ulps of v, ties kept."""
    assert v > 0.0
    return [(col, _ulps(v, -1), True), (col, _ulps(v, -(k + 1)), False), (col, v, False), (col, _ulps(v, k), True)]


def _comb32_folds(order):
    """From the image alone and the chain order _loopdef reports for hub-Y's pop in `order`: (step, alive entries, dead entries,
    sq folded serially, sq folded apart, sum folded serially, sum folded apart, pixels on the shared boundary).  An entry is the
    pair Y -> X_i, two pixels of column 5; its sq is p1 * p1 then an FMA of p2 * p2 -- both squares are exact in f64 (24 x 24 bits), so
    one rounding, the same in either order of the pixels.  The base is the record's mutual part: W -> Y, pixel (0, 4), and Y -> W,
    pixel (0, 5) (two terms: commutative); hub-Y has no other non-mutual entries.  Serially: ((base + e1) + e2) + ...;
    apart: base + (((+0.0 + e1) + e2) + ...)."""
    lab, pb = _image("comb32")
    step, pairs, alive = _loopdef.chain_entries_at_pop(lab, pb, order, kCombY, leaves=_cpu["leaves", "comb32"])
    p = pb.astype(np.float64)
    base_sq, base_sum = p[0, 4] * p[0, 4] + p[0, 5] * p[0, 5], p[0, 4] + p[0, 5]
    ser_sq, ser_sum, apart_sq, apart_sum = base_sq, base_sum, np.float64(0.0), np.float64(0.0)
    for (a, b), live in zip(pairs, alive):
        assert a == kCombY and b >= 3 and (b - 3) % 2 == 0, "a chain entry is a pair Y -> X_i"
        r = b - 2                                                    # X_i = 3 + 2 i lies in the rows 1 + 2 i and 2 + 2 i
        assert lab[r, 4] == b and lab[r, 5] == lab[r + 1, 5] == kCombY
        if live:
            e_sq, e_sum = p[r, 5] * p[r, 5] + p[r + 1, 5] * p[r + 1, 5], p[r, 5] + p[r + 1, 5]
            ser_sq, ser_sum, apart_sq, apart_sum = ser_sq + e_sq, ser_sum + e_sum, apart_sq + e_sq, apart_sum + e_sum
    n_alive = int(np.sum(alive))
    return step, n_alive, len(alive) - n_alive, float(ser_sq), float(base_sq + apart_sq), float(ser_sum), float(base_sum + apart_sum), 2 + 2 * n_alive


def _std_of(sq, total, n):
    """bc_features.hpp: mean = sum / n, stddev = sqrt(sq / n - mean * mean) (no contraction)"""
    mean = np.float64(total) / n
    return float(np.sqrt(np.float64(sq) / n - mean * mean))


def _assert_two_associations(order, where):
    """the condition on the INPUT under which the witness can see anything"""
    step, n_alive, n_dead, ser_sq, apart_sq, ser_sum, apart_sum, n = _comb32_folds(order)
    d = int(np.float64(_std_of(apart_sq, apart_sum, n)).view(np.int64) - np.float64(_std_of(ser_sq, ser_sum, n)).view(np.int64))
    print("comb32, %s: hub-Y pops at step %d with %d entries alive and %d dead; sq folded serially %r, apart %r; the standard "
          "deviations of the two are %d ulps apart" % (where, step, n_alive, n_dead, ser_sq, apart_sq, d))
    assert n_alive >= 64 and n_dead >= 1
    assert ser_sq != apart_sq, "both associations give the same sum of squares: the image is no witness"
    assert ser_sum == apart_sum, "the plain sums were expected exact (see test_comb32_has_two_associations)"
    return step, d


def test_comb32_has_two_associations():
    """No GPU: on the replayed order (the stump forest reads the mean alone, and comb32's plain sums along column 5 are exact) the
    sum of squares of hub-Y's alive entries differs between the two associations, by so little that the standard deviations stay
    within kBand ulps -- and do differ.  The plain SUM cannot be a witness on this image: the band of column 5 lies in [0.5, 0.75),
    whose float32 values are multiples of 2^-24, and 2202 of them add exactly in 53 bits whatever the jitter's seed; so only the
    column derived from sq, x0.b0.std, is witnessed."""
    step, d = _assert_two_associations(_reference("comb32", forest=True)[0], "replayed order")
    assert 0 < abs(d) <= kBand, "the two standard deviations must differ, and by no more than the band the stumps span"


@pytest.fixture(scope="module")
def wit(ctx):
    """one map object for the runs A, B and C: the RAG pass may differ from run to run in the last bit of an inexact sum"""
    w = dict(rm=_rm(ctx, "comb32"))
    yield w
    for k in ("F0", "F1"):
        if k in w:
            w[k].close()
    w["rm"].close()


def _run(w, clf, **env):
    from glia_amd import hmt
    with hmt.options(**env):
        return w["rm"].merge_order_bc(w[clf], want_feats=True)


def _wit_a(ctx, w):
    """run A: F0 = the 255 stumps on x0.b0.mean, no helpers -- every record and the popped rows by the loop's own workgroup"""
    if "A" not in w:
        _, pb = _image("comb32")
        w["stumps"] = [(STUB, t, True) for t in _stumps(pb)]
        w["F0"] = _load(ctx, _stump_arrays(w["stumps"]))
        w["A"] = _run(w, "F0", GLIA_HMT_HELPERS=0)
    return w["A"]


def _wit_proof(w, order):
    """the CPU-side conditions on run A's order, replayed once; returns the step at which hub-Y pops"""
    if "proof" not in w:
        w["proof"] = _assert_two_associations(order, "run A")[0]
    return w["proof"]


def _wit_b(ctx, w):
    """run B: F1 = F0 + the witness stumps around x0.b0.std of the row hub-Y popped with in run A, no helpers"""
    if "B" not in w:
        o, s, f = _wit_a(ctx, w)
        w["step"] = _wit_proof(w, o)
        w["F1"] = _load(ctx, _stump_arrays(w["stumps"] + _witness_stumps(float(f[w["step"], STUB + 1]), STUB + 1)))
        w["B"] = _run(w, "F1", GLIA_HMT_HELPERS=0)
    return w["B"]


@pytest.mark.gpu
def test_float32_comb_run_a(ctx, wit):
    """the CPU-side conditions on the order the device returned: at least 64 entries of hub-Y's chain alive and one dead at the pop,
    and the two associations of their squares differ"""
    from glia_amd import hmt
    before = hmt.Context.internal_errors()
    o, s, f = _wit_a(ctx, wit)
    lab, _ = _image("comb32")
    assert len(o) == len(np.unique(lab)) - 1 and _featdef.column_names(2, 3, [8], [], [8])[STUB + 1] == "x0.b0.std"
    assert (_bits(s) == _bits(wit["F0"].predict(f))).all()
    _wit_proof(wit, o)
    assert hmt.Context.internal_errors() == before == 0


@pytest.mark.gpu
def test_float32_comb_run_b(ctx, wit):
    """the witness stumps change nothing where every record goes one route: run A's order, hub-Y at the same step with the same row"""
    from glia_amd import hmt
    before = hmt.Context.internal_errors()
    (oa, sa, fa), (o, s, f) = _wit_a(ctx, wit), _wit_b(ctx, wit)
    step = wit["step"]
    assert o.shape == oa.shape and (o == oa).all(), "another record fell into the band: shrink kBand or move the seed"
    assert (_bits(s) == _bits(wit["F1"].predict(f))).all()
    assert kCombY in o[step, :2].tolist() and (_bits(f[step]) == _bits(fa[step])).all()
    assert round(s[step] * 259) == round(sa[step] * 255) + 2, "hub-Y pops AT the value: two of the four stumps vote"
    assert hmt.Context.internal_errors() == before == 0


@pytest.mark.gpu
@pytest.mark.parametrize("env", WITNESS_ENVS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default")
def test_float32_comb_under_every_setting(ctx, wit, env):
    """runs C: F1 under the default helpers, five helpers, the other two kernel instances and the smallest capacities -- (order,
    saliencies) byte-identical to run B's, saliencies = the forest's values of the returned rows.  The saliency hub-Y pops with is
    a helper's vote on ITS vector; the row is the loop's own."""
    from glia_amd import hmt
    before = hmt.Context.internal_errors()
    ob, sb, _ = _wit_b(ctx, wit)
    o, s, f = _run(wit, "F1", **env)
    step = wit["step"]
    print("comb32, %s: hub-Y pops at step %d with %r (run B: %r)" % (env, step, float(s[step]) if len(s) > step else None, float(sb[step])))
    assert _same((o, s), (ob, sb)), env
    assert (_bits(s) == _bits(wit["F1"].predict(f))).all(), env
    assert hmt.Context.internal_errors() == before == 0


@pytest.mark.gpu
def test_float32_comb_of_two_batches(ctx):
    """four channels, default helpers: the chain goes through two kFragCap batches and the fold is carried across them.  The serial
    walk without helpers takes 12 s here, so the value comes from a run with helpers: the popped row is the loop's own walk either
    way.  F0's run gives hub-Y's row; F1 has the witness stumps around x0.b0.std and x0.b3.std (both channels read comb32; the
    other two images are exact); its order is F0's and its saliencies are the forest's values of its rows."""
    from glia_amd import hmt
    lab, pb = _image("comb32")
    names = _featdef.column_names(2, 3, [8], [], [8, 8, 8, 4])
    cols = [names.index("x0.b0.std"), names.index("x0.b3.std")]
    before = hmt.Context.internal_errors()
    rm = _rm(ctx, "comb32", four=True)
    stumps = [(STUB, t, True) for t in _stumps(pb)]
    f0 = _load(ctx, _stump_arrays(stumps))
    oa, sa, fa = rm.merge_order_bc(f0, want_feats=True)
    step, pairs, alive = _loopdef.chain_entries_at_pop(lab, pb, oa, kCombY, leaves=_cpu["leaves", "comb32"])
    assert len(pairs) * 4 > kFragCap + kHelpChunk * 4 and sum(alive) >= 64 and not all(alive)
    f1 = _load(ctx, _stump_arrays(stumps + [t for c in cols for t in _witness_stumps(float(fa[step, c]), c)]))
    o, s, f = rm.merge_order_bc(f1, want_feats=True)
    assert o.shape == oa.shape and (o == oa).all()
    assert (_bits(f[step]) == _bits(fa[step])).all()
    assert (_bits(s) == _bits(f1.predict(f))).all()
    rm.close()
    f0.close()
    f1.close()
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
