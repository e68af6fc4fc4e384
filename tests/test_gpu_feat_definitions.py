"""-m gpu: the device's feature rows (bc_feat, merge_order_bc, the median layout) and its histogram / threshold counters
against the reference's definitions (tests/_featdef.py) AND the oracle, over every case of tests/_feat_cases.py: 1-16 bins on
dyadic and non-dyadic intervals, lo > 0, 0-4 thresholds sorted, unsorted and repeated, float32 values next to every bound.

  device vs definition: rtol 1e-12, atol 1e-14, always (the definition sums with math.fsum and calls Python's log2)
  device vs oracle:     bit for bit where every image is Q8; on the edge-value images bit for bit outside the mean / standard-
                        deviation columns, the means to 1e-12, the standard deviations left out (Case.std_mask: cancellation
                        of sums of squares that are not exact in double); median layout: mean / stddev columns to 1e-12
                        (Case.order_dependent_mask), every other column bit for bit
"""
import numpy as np
import pytest

import _feat_cases as FC
import _featdef as FD

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-12, 1e-14
TIERS = ({}, {"GLIA_HMT_BC_NOCOMMON": "1"}, {"GLIA_HMT_BC_GENERIC": "1"})


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
    """bit for bit outside `loose`, rtol 1e-12 inside"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint64) != want.view(np.uint64)
    bad[:, loose] = False
    assert not bad.any(), what + " (bits): " + _first(bad, cols, got, want)


def _compare(c, got, definition, oracle, what):
    cols = c.columns()
    none = np.zeros(len(cols), bool)
    std = c.std_mask() if c.edge else none
    _assert_close(got, definition, cols, std, what + " vs definition")
    loose = c.order_dependent_mask()
    if not c.q8:
        loose = loose | np.array([n.endswith(".mean") or n.endswith(".std") for n in cols])
    _assert_bits(got, oracle, cols, loose, what + " vs oracle")
    _assert_close(got, oracle, cols, std, what + " vs oracle")


@pytest.mark.parametrize("name", FC.NAMES)
def test_bc_feat_rows(ctx, name):
    from glia_amd import hmt
    c = FC.case(name)
    rm = c.device_map(ctx)
    got = c.device_rows(rm)
    assert got.shape == (len(c.order), c.feat_dim())            # D_f: the formula of bc_feat.hxx's dim()
    if c.saliency is None:
        assert rm.feat_dim() == c.feat_dim()
    rm.close()
    _compare(c, got, FC.definition_rows(name), FC.oracle_rows(name), name)
    assert hmt.Context.internal_errors() == 0


@pytest.mark.parametrize("name", FC.LOOP_NAMES)
def test_merge_loop_rows(ctx, name):
    """the rows the classifier merge loop records for the order it chooses itself"""
    from glia_amd import hmt
    c = FC.case(name)
    cols = c.columns()
    stub = cols.index("x0.b0.mean")
    rm = c.device_map(ctx)
    order, sal, feats = rm.merge_order_bc(hmt.FeatureStubClassifier(ctx, stub), want_feats=True)
    rm.close()
    o_ref, s_ref, f_ref = c.oracle_rag().merge_order_bc(c.oracle_cfg(), None, stub_index=stub, want_feats=True)
    assert order.shape == o_ref.shape and (order == o_ref).all() and (sal == s_ref).all()
    _compare(c, feats, c.definition_rows(order=o_ref, order_key=name + "/loop"), f_ref, name)
    assert hmt.Context.internal_errors() == 0


@pytest.mark.parametrize("name", FC.SPEC_AND_THR_NAMES)
def test_loop_instances_agree_on_every_bin_and_threshold_count(ctx, name):
    """greedy_bc.hip's three tiers of instances (common configuration / libm fixed / everything at run time): identical rows for
    a given order and out of the loop, on every histogram spec and threshold list"""
    from glia_amd import hmt
    c = FC.case(name)
    stub = c.columns().index("x0.b0.mean")
    # ONE map for the three tiers (the switches are read per call): the accumulation pass adds a region's sums with double
    # atomics, so two builds of the same map differ in the last bits of a sum of squares that is not exact (edge-value images)
    # and in the standard deviation that cancels it -- that is the pass, not the tier
    rm = c.device_map(ctx)
    results = []
    for env in TIERS:
        with hmt.options(**env):
            results.append((c.device_rows(rm),) + rm.merge_order_bc(hmt.FeatureStubClassifier(ctx, stub), want_feats=True))
    rm.close()
    for env, r in zip(TIERS[1:], results[1:]):
        for a, b in zip(results[0], r):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), env
    _assert_close(results[0][0], FC.definition_rows(name), c.columns(), c.std_mask() if c.edge else np.zeros(0, int), name)
    assert hmt.Context.internal_errors() == 0


@pytest.mark.parametrize("name", FC.SPEC_AND_THR_NAMES + ["geom/masked", "geom/plates", "values/constant", "values/gaussian"])
def test_histogram_and_threshold_counters(ctx, name):
    """the accumulation pass's counters of every region and directed pair, counted directly over the definition's voxel sets"""
    from glia_amd import hmt
    c = FC.case(name)
    g = FC.definition_geometry(c.geom)
    _, bins, lo, hi = c.lists["rb"][0]
    img = c.images[c.pb].ravel()
    rm = c.device_map(ctx)
    reg, par = rm.regions(), rm.pairs()
    rm.close()
    assert sorted(reg["label"].tolist()) == sorted(g.leaf_pts)
    for i, l in enumerate(reg["label"].tolist()):
        assert reg["count"][i] == len(g.leaf_pts[l])
        assert reg["hist"][i].tolist() == FD.histc(img[g.leaf_pts[l]], bins, lo, hi), (name, l)
    keys = list(zip(par["a"].tolist(), par["b"].tolist()))
    assert sorted(keys) == sorted(g.leaf_bnd)
    for i, k in enumerate(keys):
        vals = img[g.leaf_bnd[k]]
        assert par["count"][i] == len(vals)
        assert par["hist"][i].tolist() == FD.histc(vals, bins, lo, hi), (name, k)
        for j, t in enumerate(c.thr):
            assert par["thr"][i, j] == sum(1 for v in vals if float(v) >= t), (name, k, t)
    assert hmt.Context.internal_errors() == 0


def test_specs_outside_the_abi_are_refused(ctx):
    """what the C ABI does not serve (include/glia_hmt.h: 1..16 bins, lo < hi, 0..4 thresholds) comes back as GLIA_HMT_ERR_ARG with
    a message, never as a row"""
    import torch
    from glia_amd import hmt
    c = FC.case("geom/boxes")
    d_lab = torch.from_numpy(np.array(c.labels).view(np.int32)).cuda()
    d_pb = torch.from_numpy(np.array(c.images["pb"])).cuda()
    for bins, lo, hi in [(0, 0.0, 1.0), (17, 0.0, 1.0), (-1, 0.0, 1.0), (8, 1.0, 1.0), (8, 1.0, 0.0), (8, float("nan"), 1.0), (8, 0.0, float("nan"))]:
        with pytest.raises(hmt.HmtError) as e:
            hmt.RegionMap(ctx, d_lab, pb=d_pb, cfg=hmt.make_config(d_pb, rb=[(d_pb, bins, lo, hi)]))
        assert e.value.code == hmt.ERR_ARG and "bins" in str(e.value), (bins, lo, hi)
    for n in (5, -1):
        cfg = hmt.make_config(d_pb, rb=[(d_pb, 8, 0.0, 1.0)], thresholds=(0.125, 0.25, 0.5, 0.75))
        cfg.n_thresholds = n
        with pytest.raises(hmt.HmtError) as e:
            hmt.RegionMap(ctx, d_lab, pb=d_pb, cfg=cfg)
        assert e.value.code == hmt.ERR_ARG and "thresholds" in str(e.value), n
    assert hmt.Context.internal_errors() == 0
