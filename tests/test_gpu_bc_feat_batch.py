"""-m gpu: the batch route to the feature rows of a given merge order (glia_hmt_bc_feat_batch, glia_amd/csrc/bc_feat_batch.hip)
against three witnesses, all through the C ABI:

  the definitions   tests/_featdef.py                 rtol 1e-12, atol 1e-14 (standard deviations left out on edge-value images)
  the oracle        FC.oracle_rows                    bit for bit where the case is Q8, the loose columns of
                                                      test_gpu_feat_definitions.py otherwise
  the replay        rm.bc_feat on the SAME map object byte for byte where the case is Q8 (every sum is exact, so no association of the
                                                      sums can show); otherwise bit for bit outside the mean / std columns, 1e-12 inside

The same map matters: two builds of a map differ in the last bits of inexact sums of squares (the accumulation pass adds with f64
atomics), which is the pass and not the route.  The comparison helpers restate those of test_gpu_feat_definitions.py.
"""
import numpy as np
import pytest

import _feat_cases as FC
import _featdef as FD

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-12, 1e-14


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    c.close()
    assert hmt.Context.internal_errors() == 0


def _first(bad, cols, got, want):
    i, j = np.argwhere(bad)[0]
    return "%d cells differ, first at row %d column %d (%s): %r vs %r" % (int(bad.sum()), i, j, cols[j], got[i, j], want[i, j])


def _assert_close(got, want, cols, skip, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~np.isclose(got, want, rtol=RTOL, atol=ATOL)
    bad[:, skip] = False
    assert not bad.any(), what + ": " + _first(bad, cols, got, want)


def _assert_bits(got, want, cols, loose, what):
    """bit for bit outside `loose`"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint64) != want.view(np.uint64)
    bad[:, loose] = False
    assert not bad.any(), what + " (bits): " + _first(bad, cols, got, want)


def _compare(c, got, definition, oracle, what):
    cols = c.columns()
    none = np.zeros(len(cols), bool)
    std = c.std_mask() if c.edge else none
    _assert_close(got, definition, cols, std, what + " vs definition")
    if oracle is None:
        return
    loose = c.order_dependent_mask()
    if not c.q8:
        loose = loose | np.array([n.endswith(".mean") or n.endswith(".std") for n in cols])
    _assert_bits(got, oracle, cols, loose, what + " vs oracle")
    _assert_close(got, oracle, cols, std, what + " vs oracle")


def _compare_routes(c, batch, replay, what):
    if c.q8:
        assert batch.shape == replay.shape and batch.tobytes() == replay.tobytes(), what + ": batch and replay differ on a Q8 case"
        return
    cols = c.columns()
    loose = np.array([n.endswith(".mean") or n.endswith(".std") for n in cols])
    _assert_bits(batch, replay, cols, loose, what + " vs replay")
    _assert_close(batch, replay, cols, c.std_mask() if c.edge else np.zeros(len(cols), bool), what + " vs replay")


def _batch_rows(c, rm):
    if c.saliency is not None:
        return rm.bc_feat_batch(c.order, saliencies=c.order_sal, init_sal=c.saliency[0], sal_bias=c.saliency[1])
    return rm.bc_feat_batch(c.order)


# ---- 1. every case of _feat_cases ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.NAMES)
def test_batch_rows_of_every_case(ctx, name):
    from glia_amd import hmt
    c = FC.case(name)
    rm = c.device_map(ctx)
    got = _batch_rows(c, rm)
    assert rm.last_bc_feat_timing()["route"] == "batch"
    replay = c.device_rows(rm)
    assert rm.last_bc_feat_timing()["route"] == "replay"
    rm.close()
    assert got.shape == (len(c.order), c.feat_dim())
    _compare(c, got, FC.definition_rows(name), FC.oracle_rows(name), name)
    _compare_routes(c, got, replay, name)
    assert hmt.Context.internal_errors() == 0


# ---- 2. / 3. tree shapes and cancellations the cases above do not make ------------------------------------------------------------
class _Custom(FC.Case):
    """a Case on a geometry of this file (FC.geometry knows its own names only)"""

    def __init__(self, name, labels, order, pb):
        self.name, self.geom = name, name
        self.labels, self.mask, self.order, self.order_sal = labels, None, np.ascontiguousarray(order, np.uint32), None
        self.images, self.pb = {"pb": pb}, "pb"
        self.lists = dict(rb=[("pb", 8, 0.0, 1.0)])
        self.thr = FC.DEFAULT_THR
        self.edge, self.q8, self.saliency = False, True, None
        self.flags = dict(norm_area=1.0, norm_len=1.0, use_log=False, use_simple=False, hist_as_feats=False, median_as_feats=False)
        self.dim = labels.ndim

    def definition_rows(self):
        g = FD.Geometry(self.labels, None, self.order)
        return FD.feature_rows(g, self.images["pb"], thresholds=self.thr, **self._lists(self.images), **self.flags)


N_PLATES = 100


def _plates():
    """100 plates of 4 x 4 x 2 voxels stacked along z, labels 1 .. 100 from z = 0; Q8 pb"""
    lab = np.repeat(np.arange(1, N_PLATES + 1, dtype=np.uint32), 2)[:, None, None] * np.ones((1, 4, 4), np.uint32)
    pb = (np.random.default_rng(77).integers(0, 256, lab.shape) / 256.0).astype(np.float32)
    return np.ascontiguousarray(lab), pb


def _chain(leaves, first_key):
    """leaves[0] + leaves[1] -> first_key, that + leaves[2] -> first_key + 1, ...; returns (merges, key of the last region)"""
    out, top, key = [], leaves[0], first_key
    for l in leaves[1:]:
        out.append([top, l, key])
        top, key = key, key + 1
    return out, top


def _plate_orders():
    n = N_PLATES
    up = list(range(1, n + 1))
    orders = {"chain_from_bottom": _chain(up, n + 1)[0], "chain_from_top": _chain(up[::-1], n + 1)[0]}
    rounds, roots, key = [], up, n + 1
    while len(roots) > 1:                                     # neighbours in z pair up; 100 is no power of two: odd rounds carry one over
        nxt = []
        for i in range(0, len(roots) - 1, 2):
            rounds.append([roots[i], roots[i + 1], key]); nxt.append(key); key += 1
        if len(roots) & 1:
            nxt.append(roots[-1])
        roots = nxt
    orders["pairwise_rounds"] = rounds
    orders["first_37_of_the_chain"] = orders["chain_from_bottom"][:37]
    lo, lo_top = _chain(up[:50], n + 1)
    hi, hi_top = _chain(up[:49:-1], n + 1 + len(lo))
    orders["two_chains_joined_last"] = lo + hi + [[lo_top, hi_top, n + 1 + len(lo) + len(hi)]]
    return orders


PLATE_ORDERS = _plate_orders()


@pytest.mark.parametrize("name", list(PLATE_ORDERS))
def test_tree_shapes_on_stacked_plates(ctx, name):
    from glia_amd import hmt
    lab, pb = _plates()
    c = _Custom("plates100/" + name, lab, PLATE_ORDERS[name], pb)
    assert len(c.order) == {"first_37_of_the_chain": 37}.get(name, N_PLATES - 1)
    rm = c.device_map(ctx)
    got = rm.bc_feat_batch(c.order)
    t = rm.last_bc_feat_timing()
    replay = rm.bc_feat(c.order)
    rm.close()
    assert t["route"] == "batch" and t["launches"] > 0 and t["path_updates"] > 0
    if name.startswith("chain_from"):
        assert t["height"] == N_PLATES - 1
    if name == "pairwise_rounds":
        assert t["height"] == 7                               # ceil(log2(100))
    assert got.shape == replay.shape and got.tobytes() == replay.tobytes(), name + ": batch and replay differ"
    _compare(c, got, c.definition_rows(), None, name)
    assert hmt.Context.internal_errors() == 0


def _shells():
    """a 4^3 box (label 3) inside an 8^3 box (2) inside the 12^3 volume (1).  Q8 pb: the voxels of the inner interface -- the surface
    of 3 and the voxels of 2 that touch it -- hold 0 and 255/256 in turn, every other voxel lies in [64/256, 192/256)."""
    lab = np.ones((12, 12, 12), np.uint32)
    lab[2:10, 2:10, 2:10] = 2
    lab[4:8, 4:8, 4:8] = 3
    pb = (np.random.default_rng(5).integers(64, 192, lab.shape) / 256.0).astype(np.float32)
    near3 = np.zeros(lab.shape, bool)
    near3[3:9, 3:9, 3:9] = True
    near3[5:7, 5:7, 5:7] = False                              # the core of 3 has no neighbour in 2
    z, y, x = np.indices(lab.shape)
    pb[near3] = np.where((z + y + x)[near3] % 2 == 0, 0.0, 255.0 / 256.0).astype(np.float32)
    return lab, pb


@pytest.mark.parametrize("name,order", [("inner_first", [[2, 3, 4], [4, 1, 5]]), ("outer_first", [[1, 2, 4], [4, 3, 5]])])
def test_extrema_leave_with_their_entries(ctx, name, order):
    """the global minimum and maximum of the boundary image lie on the interface of 2 and 3: once that interface is inside a
    region, the region's boundary min / max come from the outer interface alone"""
    from glia_amd import hmt
    lab, pb = _shells()
    g = FD.Geometry(lab, None, order)
    inner = np.concatenate([g.leaf_bnd[(2, 3)], g.leaf_bnd[(3, 2)]])
    outer = np.concatenate([g.leaf_bnd[(1, 2)], g.leaf_bnd[(2, 1)]])
    flat = pb.ravel()
    assert flat[inner].min() == flat.min() == 0.0 and flat[inner].max() == flat.max() == np.float32(255.0 / 256.0)
    assert flat[outer].min() >= 0.25 and flat[outer].max() < 0.75
    c = _Custom("shells/" + name, lab, order, pb)
    rm = c.device_map(ctx)
    got = rm.bc_feat_batch(c.order)
    replay = rm.bc_feat(c.order)
    rm.close()
    cols = c.columns()
    if name == "inner_first":                                 # B(2 + 3) = the entries 2 -> 1 only
        vals = flat[g.leaf_bnd[(2, 1)]]
        assert got[0, cols.index("x3.b0.min")] == vals.min() and got[0, cols.index("x3.b0.max")] == vals.max()
        assert got[0, cols.index("x0.b0.min")] == 0.0        # ... and the shared boundary of that merge is the inner interface
    assert got.tobytes() == replay.tobytes(), name + ": batch and replay differ"
    _compare(c, got, c.definition_rows(), None, name)
    assert hmt.Context.internal_errors() == 0


# ---- 4. directed-only adjacencies: target leaf dead / alive at the join -----------------------------------------------------------
def _directed_only(pairs, order):
    """[(a, b, alive)] for every entry (a, b) without (b, a) whose leaves a merge of `order` joins; alive: at that merge b still owns
    a non-mutual entry or a mutual partner outside its side (TRegion::boundaryWith, type/region.hxx:42-51)"""
    pairs = set(pairs)
    out_of = {}
    for a, b in pairs:
        out_of.setdefault(a, []).append(b)
    under, res = {}, []
    for x0, x1, x2 in order:
        s0, s1 = under.get(x0, {x0}), under.get(x1, {x1})
        for a, b in pairs:
            if (b, a) in pairs:
                continue
            for sa, sb in ((s0, s1), (s1, s0)):
                if a in sa and b in sb:
                    res.append((a, b, any((t, b) not in pairs or t not in sb for t in out_of.get(b, []))))
        under[x2] = s0 | s1
    return res


def test_cases_hold_dead_and_alive_directed_only_targets(ctx):
    from glia_amd import hmt
    seen = {True: 0, False: 0}
    for name in ("geom/masked", "geom/synth2d", "geom/plates"):
        c = FC.case(name)
        rm = c.device_map(ctx)
        par = rm.pairs()
        status = _directed_only(zip(par["a"].tolist(), par["b"].tolist()), [tuple(int(v) for v in m) for m in c.order])
        for _, _, alive in status:
            seen[alive] += 1
        got = _batch_rows(c, rm)
        replay = c.device_rows(rm)
        rm.close()
        assert len(status) > 0, name
        _compare(c, got, FC.definition_rows(name), FC.oracle_rows(name), name)
        _compare_routes(c, got, replay, name)
    assert seen[True] > 0 and seen[False] > 0, seen
    assert hmt.Context.internal_errors() == 0


# ---- 5. both routes through the option ------------------------------------------------------------------------------------------------
def test_option_reroutes_the_existing_entry_points(ctx):
    from glia_amd import hmt
    c = FC.case("layout/saliency")
    rm = c.device_map(ctx)
    batch = _batch_rows(c, rm)
    with hmt.options(GLIA_HMT_BCFEAT="batch"):
        via_option = c.device_rows(rm)
        assert rm.last_bc_feat_timing()["route"] == "batch"
        plain = rm.bc_feat(c.order)
        assert rm.last_bc_feat_timing()["route"] == "batch"
        assert plain.tobytes() == rm.bc_feat_batch(c.order).tobytes()
    assert via_option.tobytes() == batch.tobytes()
    c.device_rows(rm)
    assert rm.last_bc_feat_timing()["route"] == "replay"
    with hmt.options(GLIA_HMT_BCFEAT="replay"):
        rm.bc_feat(c.order)
        assert rm.last_bc_feat_timing()["route"] == "replay"
    with hmt.options(GLIA_HMT_BCFEAT="both"):
        with pytest.raises(hmt.HmtError) as e:
            rm.bc_feat(c.order)
        assert e.value.code == hmt.ERR_ARG and "GLIA_HMT_BCFEAT" in str(e.value)
    rm.close()
    assert hmt.Context.internal_errors() == 0


# ---- 6. determinism -----------------------------------------------------------------------------------------------------------------------
def test_two_calls_return_identical_bytes(ctx):
    c = FC.case("values/gaussian")                                # float32 values, no sum exact
    assert not c.q8
    rm = c.device_map(ctx)
    a = rm.bc_feat_batch(c.order)
    b = rm.bc_feat_batch(c.order)
    rm.close()
    assert a.tobytes() == b.tobytes()


# ---- 7. one workload-shaped check --------------------------------------------------------------------------------------------------------
def test_workload_shaped_order(ctx):
    from glia_amd import hmt
    labels, pb = ctx.synth((128,) * 3, 8, 64)
    rm0 = hmt.RegionMap(ctx, labels, pb=pb, only_contour=True)
    order, _ = rm0.merge_order_pb(type=2)
    rm0.close()
    rm = hmt.RegionMap(ctx, labels, pb=pb, cfg=hmt.make_config(pb, rb=[(pb, 8, 0.0, 1.0)]))
    got = rm.bc_feat_batch(order)
    t = rm.last_bc_feat_timing()
    replay = rm.bc_feat(order)
    rm.close()
    assert got.shape == (4095, 104)
    assert t["route"] == "batch" and t["height"] > 64, t        # several lifting levels
    assert got.tobytes() == replay.tobytes()
    assert hmt.Context.internal_errors() == 0


# ---- 8. argument errors equal the replay's ----------------------------------------------------------------------------------------------
def test_argument_errors_equal_the_replays(ctx):
    import torch
    from glia_amd import hmt
    c = FC.case("geom/plates")
    rm = c.device_map(ctx)
    keys = sorted(set(np.unique(c.labels).tolist()))
    fresh = max(int(c.order.max()), max(keys)) + 1
    bad_orders = {
        "unknown key": [[keys[0], fresh + 7, fresh]],
        "key merged twice": [[keys[0], keys[1], fresh], [keys[0], keys[2], fresh + 1]],
        "reused key": [[keys[0], keys[1], keys[2]]],
        "more merges than regions": [[keys[0], keys[1], fresh + i] for i in range(len(keys))],
    }
    for what, order in bad_orders.items():
        order = np.array(order, np.uint32)
        errs = []
        for call in (rm.bc_feat, rm.bc_feat_batch):
            with pytest.raises(hmt.HmtError) as e:
                call(order)
            errs.append((e.value.code, str(e.value)))
        assert errs[0][0] == hmt.ERR_ARG and errs[0] == errs[1], (what, errs)
    rm.close()
    d_lab = torch.from_numpy(np.array(c.labels).view(np.int32)).cuda()
    d_pb = torch.from_numpy(np.array(c.images["pb"])).cuda()
    # a full vector longer than the kernels' limit (three 16-bin images with histogram columns: 524 columns before the selection)
    big = hmt.make_config(d_pb, use_histogram_features=True, use_simple_features=True,
                          rb=[(d_pb, 16, 0.0, 1.0), (d_pb, 16, 0.0, 0.5), (d_pb, 16, 0.0, 2.0)])
    rm = hmt.RegionMap(ctx, d_lab, pb=d_pb, cfg=big)
    errs = []
    for call in (rm.bc_feat, rm.bc_feat_batch):
        with pytest.raises(hmt.HmtError) as e:
            call(c.order)
        errs.append((e.value.code, str(e.value)))
    rm.close()
    assert errs[0][0] == hmt.ERR_ARG and "too long" in errs[0][1] and errs[0] == errs[1], errs
    # a map without region points, and one without a configuration (no row width: asked of the C entry points themselves)
    import ctypes as C
    order = np.ascontiguousarray(c.order, np.uint32)
    room = np.zeros(len(order) * 1024, np.float64)
    for kw in (dict(only_contour=True, cfg=hmt.make_config(d_pb, rb=[(d_pb, 8, 0.0, 1.0)])), dict()):
        rm = hmt.RegionMap(ctx, d_lab, pb=d_pb, **kw)
        errs = []
        for fn in (hmt.lib().glia_hmt_bc_feat_saliency, hmt.lib().glia_hmt_bc_feat_batch):
            rc = fn(ctx.h, rm.h, order.ctypes.data_as(C.c_void_p), C.c_int64(len(order)), None, C.c_double(1.0), C.c_double(1.0),
                    room.ctypes.data_as(C.c_void_p))
            errs.append((rc, hmt.lib().glia_hmt_last_error().decode()))
        rm.close()
        assert errs[0][0] == hmt.ERR_ARG and errs[0] == errs[1], (list(kw), errs)
    assert hmt.Context.internal_errors() == 0
