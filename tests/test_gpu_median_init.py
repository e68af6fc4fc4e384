"""-m gpu: the median layout (GLIA_USE_MEDIAN_AS_FEATS) for the scores of the INITIAL edges -- sorted runs per leaf and per directed
pair, medians selected over the runs (glia_amd/csrc/median_init.hip), spliced into the vector on the device.

Expected rows.  The first merge of an order sees the initial map, so the row of an initial edge (x, y) is the oracle's bc_feat with
median_as_feats on an order in which (x, y) merges two LEAVES.  The oracle accepts the one-merge order [(x, y, key)] (checked on the
CPU: identical rows), but generates the features of every region of the map per call; the rows here come from orders that are MATCHINGS
of leaf pairs -- a merge of two other leaves changes none of the sets P(x), P(y), B(x), B(y), Sh(x, y) -- about twenty calls instead
of several hundred.  TBoundaryTable::init hands the pair over as (first, second) in the region map's iteration order; the area rule
then picks x1, so with equal areas that order decides: the orders below list each pair in the oracle's region_iter_order.
A score is read with FeatureStubClassifier(ctx, j): 1.0 - x[j].  The bit-exact claims hold up to the -0.0 / +0.0 order of the radix
sort, as for bc_feat (no image here holds a negative zero)."""
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 3          # thresholds of the default configuration


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    assert hmt.Context.internal_errors() == 0
    c.close()


def _records(a, b):
    """the initial records from the map's directed pairs (ascending (a, b)): one per unordered adjacent leaf pair, owned by the
    (a < b) entry when it exists, else by the lone (a > b) entry -- lexicographic among the mutual pairs, which are the table edges.
    Returns [(min, max, mutual)]."""
    have = set(zip(a.tolist(), b.tolist()))
    rec = []
    for x, y in zip(a.tolist(), b.tolist()):
        mutual = (y, x) in have
        if x < y or not mutual:
            rec.append((min(x, y), max(x, y), mutual))
    return rec


def _matchings(edges):
    """greedy edge colouring: lists of edge indices in which no leaf occurs twice"""
    used, out = {}, []
    for i, (x, y) in enumerate(edges):
        c = 0
        while c in used.get(x, ()) or c in used.get(y, ()):
            c += 1
        used.setdefault(x, set()).add(c); used.setdefault(y, set()).add(c)
        while len(out) <= c:
            out.append([])
        out[c].append(i)
    return out


def _layout(dim, n_r, n_rl, n_b, hist=(0, 0, 0)):
    """column indices of the full median-layout vector: diff_* per region image, sh_* per boundary image, reg_*[blk][img] and
    bnd_*[blk][img] for the blocks x1, x2, x1 + x2 (hist = histogram columns per region / label / boundary image)"""
    hr, hl, hbb = hist
    L = dict(diff_med=[], diff_mean=[], diff_std=[], sh_med=[], sh_mean=[], sh_std=[], sh_min=[],
             reg_med=[[], [], []], reg_mean=[[], [], []], reg_std=[[], [], []], bnd_med=[[], [], []], bnd_mean=[[], [], []], bnd_std=[[], [], []])
    pos = 11 + 4 * T
    for _ in range(n_r):
        L["diff_med"].append(pos + 3); L["diff_mean"].append(pos + 4); L["diff_std"].append(pos + 5); pos += 8
    pos += 3 * n_rl
    for _ in range(n_b):
        pos += hbb + 1
        L["sh_med"].append(pos); L["sh_mean"].append(pos + 1); L["sh_std"].append(pos + 2); L["sh_min"].append(pos + 3); pos += 5
    for blk in range(3):
        pos += 4 + dim + 2 * T
        for _ in range(n_r):
            pos += hr + 1
            L["reg_med"][blk].append(pos); L["reg_mean"][blk].append(pos + 1); L["reg_std"][blk].append(pos + 2); pos += 5
        pos += (hl + 1) * n_rl
        for _ in range(n_b):
            pos += hbb + 1
            L["bnd_med"][blk].append(pos); L["bnd_mean"][blk].append(pos + 1); L["bnd_std"][blk].append(pos + 2); pos += 5
    L["dim"] = pos
    L["median"] = L["diff_med"] + L["sh_med"] + sum(L["reg_med"], []) + sum(L["bnd_med"], [])
    L["loose"] = L["diff_mean"] + L["diff_std"] + L["sh_mean"] + L["sh_std"] + sum(L["reg_mean"] + L["reg_std"] + L["bnd_mean"] + L["bnd_std"], [])
    return L


class Case:
    """one volume: the device's records and, per configuration, the oracle's rows of its table edges (computed once, shared)"""

    def __init__(self, labels, pb, mask=None):
        import torch
        from oracle import pyoracle as O
        self.labels, self.pb, self.mask = labels, pb, mask
        self.d_lab = torch.from_numpy(labels.view(np.int32)).cuda()
        self.d_pb = torch.from_numpy(pb).cuda()
        self.d_mask = None if mask is None else torch.from_numpy(mask.view(np.int32)).cuda()
        rag = O.Rag(labels, mask=mask)
        a, b, _ = rag.pairs()
        self.pairs = (a, b)
        self.rec = _records(a, b)
        self.table = np.array([m for _, _, m in self.rec], bool)
        rank = {int(l): i for i, l in enumerate(rag.region_iter_order())}
        self.edges = [(x, y) if rank[x] < rank[y] else (y, x) for x, y, m in self.rec if m]      # (first, second) of every table edge
        self.key = int(rag.regions()[0].max()) + 1
        self._rows = {}

    def oracle_rows(self, name, **okw):
        from oracle import pyoracle as O
        if name not in self._rows:
            ocfg = O.make_cfg(self.pb, **okw)
            rows = None
            for m in _matchings(self.edges):
                order = np.array([[self.edges[i][0], self.edges[i][1], self.key + k] for k, i in enumerate(m)], np.uint32)
                f = O.Rag(self.labels, mask=self.mask).bc_feat(ocfg, order)
                if rows is None:
                    rows = np.empty((len(self.edges), f.shape[1]))
                rows[m] = f
            rows.setflags(write=False)
            self._rows[name] = rows
        return self._rows[name]

    def region_map(self, ctx, **dkw):
        from glia_amd import hmt
        return hmt.RegionMap(ctx, self.d_lab, pb=self.d_pb, mask=self.d_mask, cfg=hmt.make_config(self.d_pb, **dkw))

    def column(self, ctx, rm, j):
        """column j of every table edge's vector on the device; non-table records must carry no score"""
        from glia_amd import hmt
        s = rm.score_initial_edges_shard(hmt.FeatureStubClassifier(ctx, j), 0, 1)
        assert len(s) == len(self.rec) and (np.isfinite(s) == self.table).all()
        return s[self.table]


def _exact(case, ctx, rm, ref, cols):
    for j in cols:
        got = case.column(ctx, rm, j)
        bad = np.flatnonzero(got.view(np.uint64) != (1.0 - ref[:, j]).view(np.uint64))
        assert len(bad) == 0, "column %d differs at %d table edges, first (first, second) = %r: %r != %r" % (
            j, len(bad), case.edges[bad[0]], got[bad[0]], 1.0 - ref[bad[0], j])


def _close(case, ctx, rm, ref, cols):
    for j in cols:
        got = 1.0 - case.column(ctx, rm, j)
        assert np.allclose(got, ref[:, j], rtol=1e-12, atol=1e-13), "column %d: max |d| = %g" % (j, np.abs(got - ref[:, j]).max())


@pytest.fixture(scope="module")
def case_a():
    from oracle import pyoracle as O
    import torch
    labels, pb = O.synth((24, 30, 22), 5, 10)
    c = Case(labels, pb)
    c.raw = np.random.default_rng(11).random(labels.shape, dtype=np.float32)      # not quantised: (nearly) all values distinct
    c.d_raw = torch.from_numpy(c.raw).cuda()
    c.okw = dict(rb=[(pb, 8, 0.0, 1.0)], r=[(c.raw, 8, 0.0, 1.0)], b=[(c.raw, 8, 0.0, 1.0)])
    c.dkw = dict(rb=[(c.d_pb, 8, 0.0, 1.0)], r=[(c.d_raw, 8, 0.0, 1.0)], b=[(c.d_raw, 8, 0.0, 1.0)])
    return c


def test_synthetic_3d_every_median_column(ctx, case_a):
    """a: rb = pb (Q8, ties) + a non-quantised f32 image on the region and the boundary list"""
    from oracle import pyoracle as O
    c = case_a
    ref = c.oracle_rows("median", median_as_feats=True, **c.okw)
    L = _layout(3, 2, 0, 2)
    rm = c.region_map(ctx, use_median_features=True, **c.dkw)
    assert rm.feat_dim() == ref.shape[1] == L["dim"] == O.feat_dim(3, O.make_cfg(c.pb, **c.okw)) + 16
    assert len(c.edges) > 500
    _exact(c, ctx, rm, ref, L["median"])
    _close(c, ctx, rm, ref, [L["diff_mean"][1], L["diff_std"][1], L["sh_mean"][1], L["sh_std"][1], L["reg_mean"][2][1], L["reg_std"][2][1],
                             L["reg_mean"][0][0], L["reg_std"][1][1], L["bnd_mean"][2][1], L["bnd_std"][2][1], L["bnd_mean"][0][0], L["bnd_std"][1][1]])
    _exact(c, ctx, rm, ref, [0, L["sh_min"][1]])            # the splice moved nothing: boundary length, the shared boundary's minimum
    rm.close()


def test_synthetic_2d_non_mutual_entries_stay_in_boundary_sets(ctx):
    """b: in 2D the first-different-neighbour rule leaves directed pairs without a partner; they are part of B(u) (TRegion::merge)"""
    from oracle import pyoracle as O
    import torch
    labels, pb = O.synth((64, 64), 4, 16)
    c = Case(labels, pb)
    raw = (np.round(np.random.default_rng(5).random(labels.shape) * 255) / 256.0).astype(np.float32)
    d_raw = torch.from_numpy(raw).cuda()
    a, b = c.pairs
    have = set(zip(a.tolist(), b.tolist()))
    lone_src = {x for x, y in have if (y, x) not in have}
    assert lone_src and any(x in lone_src or y in lone_src for x, y in c.edges), "the case has non-mutual entries at leaves of table edges"
    ref = c.oracle_rows("split", median_as_feats=True, r=[(raw, 4, 0.0, 1.0)], b=[(pb, 8, 0.0, 1.0)], rl=[(raw, 4, 0.0, 1.0)])
    L = _layout(2, 1, 1, 1)
    assert ref.shape[1] == L["dim"]
    rm = c.region_map(ctx, use_median_features=True, r=[(d_raw, 4, 0.0, 1.0)], b=[(c.d_pb, 8, 0.0, 1.0)], rl=[(d_raw, 4, 0.0, 1.0)])
    _exact(c, ctx, rm, ref, L["median"])
    _close(c, ctx, rm, ref, [L["bnd_mean"][0][0], L["bnd_std"][2][0], L["reg_std"][2][0]])
    rm.close()


@pytest.mark.parametrize("transposed", [False, True])
def test_leaf_with_more_than_64_runs(ctx, transposed):
    """c: a strip next to 72 four-voxel regions, random Q8 values.  As 8 x 72 (rows 0-3 the strip, rows 4-7 one-column regions) the x
    neighbours come first in the neighbour rule, so the columns' entries point at each other and the strip's 72 one-voxel runs are
    all non-mutual: that image has a single table edge.  The transposed image (72 x 8: columns 0-3 the strip, columns 4-7 one-row
    regions) makes every (strip, row) pair mutual: 72 table edges whose B(strip) and B(strip + row) have 72 runs -- the run loop --
    beside 4-voxel sets and boundary runs of one and three voxels.  Both are checked."""
    lab = np.empty((8, 72), np.uint32)
    lab[:4] = 1
    lab[4:] = np.arange(2, 74, dtype=np.uint32)[None, :]
    pb = (np.round(np.random.default_rng(3).random((8, 72)) * 255) / 256.0).astype(np.float32)
    if transposed:
        lab, pb = np.ascontiguousarray(lab.T), np.ascontiguousarray(pb.T)
    c = Case(lab, pb)
    a, _ = c.pairs
    if transposed:
        assert (a == 1).sum() == 72 and sum(1 for x, y in c.edges if 1 in (x, y)) == 72
    else:
        assert (a == 1).sum() == 72 and len(c.edges) >= 1
    ref = c.oracle_rows("rb", median_as_feats=True, rb=[(pb, 8, 0.0, 1.0)])
    L = _layout(2, 1, 0, 1)
    rm = c.region_map(ctx, use_median_features=True, rb=[(c.d_pb, 8, 0.0, 1.0)])
    _exact(c, ctx, rm, ref, L["sh_med"] + [L["bnd_med"][k][0] for k in range(3)] + [L["reg_med"][2][0]])
    _close(c, ctx, rm, ref, [L["bnd_mean"][2][0], L["bnd_std"][2][0]])
    rm.close()


def test_simple_selection(ctx, case_a):
    """d: --simpf carries the shared boundary's median beside its mean (hmt/bc_feat.hxx:263-268)"""
    c = case_a
    ref = c.oracle_rows("simple", median_as_feats=True, use_simple=True, **c.okw)
    rm = c.region_map(ctx, use_median_features=True, use_simple_features=True, **c.dkw)
    assert rm.feat_dim() == ref.shape[1] == 5 + 2 * 2 + 4 * 2
    _exact(c, ctx, rm, ref, [5 + 1, 5 + 3, 0, 5 + 4 + 1])          # both medians; a shape column; a region-difference column the splice passes on
    _close(c, ctx, rm, ref, [5 + 0, 5 + 2, 5 + 4, 5 + 8])          # the means beside them, |d mean| of both region images
    rm.close()


def test_histogram_columns_and_mask(ctx, case_a):
    """d: use_histogram_features moves every block by its bins; masked-out voxels leave every value multiset"""
    from oracle import pyoracle as O
    a = case_a
    mask = (np.random.default_rng(5).random(a.labels.shape) > 0.15).astype(np.uint32)
    c = Case(a.labels, a.pb, mask=mask)
    ref = c.oracle_rows("hist", median_as_feats=True, hist_as_feats=True, **a.okw)
    L = _layout(3, 2, 0, 2, hist=(8, 0, 8))
    rm = c.region_map(ctx, use_median_features=True, use_histogram_features=True, **a.dkw)
    assert rm.feat_dim() == ref.shape[1] == L["dim"]
    _exact(c, ctx, rm, ref, L["median"] + [L["sh_min"][0], L["reg_med"][0][0] - 2])        # ... and a histogram column
    _close(c, ctx, rm, ref, [L["sh_std"][0], L["reg_mean"][1][1], L["bnd_std"][2][1]])
    rm.close()


FOREST_SEED = 7


def test_random_forest_on_the_median_layout(ctx, case_a):
    """d: a forest drawn on the oracle's median rows; votes / ntree must equal O.forest_predict of those rows for every table edge.
    A split within 1e-12 of a mean / stddev column's value could go either way: the seed was chosen on the CPU so that no
    threshold lies within 1e-9 of any loose-column value of the case, which is asserted."""
    from glia_amd import hmt
    from oracle import pyoracle as O
    import _rf
    c = case_a
    ref = c.oracle_rows("median", median_as_feats=True, **c.okw)
    forest = _rf.random_forest(np.random.default_rng(FOREST_SEED), 31, 6, ref)
    loose = set(_layout(3, 2, 0, 2)["loose"])
    used = 0
    for t in range(forest["bestvar"].shape[0]):
        for k in np.flatnonzero(forest["nodestatus"][t] == 1):
            var = int(forest["bestvar"][t, k]) - 1
            if var in loose:
                used += 1
                assert np.abs(ref[:, var] - forest["xbestsplit"][t, k]).min() > 1e-9
    assert used > 10, "the forest does split on mean / stddev columns"
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "model.bin")
        _rf.write_model(path, forest)
        clf = hmt.RandomForest(ctx, path, predict_label=-1)
    rm = c.region_map(ctx, use_median_features=True, **c.dkw)
    got = rm.score_initial_edges_shard(clf, 0, 1)
    assert (np.isfinite(got) == c.table).all()
    of = O.make_forest(forest, -1)
    want = np.array([O.forest_predict(of, row) for row in ref])
    assert len(set(want.tolist())) > 5 and (got[c.table] == want).all()
    rm.close()


def test_shards_and_batches(ctx, case_a):
    """e: three shards are disjoint and their maximum is the unsharded result; the same scores when the records go through the
    median stage in several batches; score_initial_edges counts the same edges as with the default layout"""
    from glia_amd import hmt
    c = case_a
    j = _layout(3, 2, 0, 2)["bnd_med"][2][1]
    clf = hmt.FeatureStubClassifier(ctx, j)
    rm = c.region_map(ctx, use_median_features=True, **c.dkw)
    full = rm.score_initial_edges_shard(clf, 0, 1)
    parts = [rm.score_initial_edges_shard(clf, r, 3) for r in range(3)]
    assert all(len(p) == len(full) for p in parts) and (np.maximum.reduce(parts) == full).all()
    fin = [np.isfinite(p) for p in parts]
    assert not (fin[0] & fin[1]).any() and not (fin[1] & fin[2]).any() and not (fin[0] & fin[2]).any()
    assert np.isfinite(full).sum() == sum(f.sum() for f in fin) == c.table.sum()
    with hmt.options(GLIA_HMT_MEDIAN_BATCH=100):
        assert (rm.score_initial_edges_shard(clf, 0, 1) == full).all()
        assert (rm.score_initial_edges_shard(clf, 1, 3) == parts[1]).all()
    n_med, _ = rm.score_initial_edges(clf)
    rm_def = c.region_map(ctx, **c.dkw)
    n_def, _ = rm_def.score_initial_edges(hmt.FeatureStubClassifier(ctx, 0))
    assert n_med == n_def == c.table.sum()
    rm.close(); rm_def.close()


def test_same_medians_as_the_sort_based_route(ctx, case_a):
    """f: for 32 table edges the median columns equal those of bc_feat on the device (median_feats.hip gathers and sorts each set)"""
    c = case_a
    L = _layout(3, 2, 0, 2)
    rm = c.region_map(ctx, use_median_features=True, **c.dkw)
    idx = np.linspace(0, len(c.edges) - 1, 32).astype(int)
    rows = np.empty((32, L["dim"]))
    sub = [c.edges[i] for i in idx]
    for m in _matchings(sub):
        rows[m] = rm.bc_feat(np.array([[sub[i][0], sub[i][1], c.key + k] for k, i in enumerate(m)], np.uint32))
    for j in L["median"]:
        got = c.column(ctx, rm, j)[idx]
        assert (got.view(np.uint64) == (1.0 - rows[:, j]).view(np.uint64)).all(), j
    rm.close()


def test_loop_still_refuses_and_default_layout_unchanged(ctx, case_a):
    """g: merge_order_bc keeps its refusal; a map with the default layout scores as before -- the oracle's default rows, bit for bit
    on the Q8 image"""
    from glia_amd import hmt
    c = case_a
    rm = c.region_map(ctx, use_median_features=True, rb=[(c.d_pb, 8, 0.0, 1.0)])
    with pytest.raises(hmt.HmtError, match="given merge order only"):
        rm.merge_order_bc(hmt.FeatureStubClassifier(ctx, 5))
    rm.close()
    ref = c.oracle_rows("default", rb=[(c.pb, 8, 0.0, 1.0)])
    rm = c.region_map(ctx, rb=[(c.d_pb, 8, 0.0, 1.0)])
    assert rm.feat_dim() == ref.shape[1] == 104
    _exact(c, ctx, rm, ref, [0, 31, 11 + 4 * T + 4, 103])
    rm.close()
