"""No GPU: the oracle's feature rows (oracle/hmt_oracle.cc: orc_bc_feat_sal, orc_merge_order_bc) against the reference's
definitions restated in tests/_featdef.py, over every case of tests/_feat_cases.py.

Tolerance rtol 1e-12, atol 1e-14: the project's number for sums taken in another order (the oracle adds in list order, the
definition with math.fsum; Python's math.log2 is not the host's std::log2 bit for bit either).  On the edge-value images alone
the standard-deviation columns and their differences are left out (Case.std_mask): sum of squares / n - mean^2 cancels there
and what is left is summation order; the Q8 cases cover those columns.  Nothing else is left out.
"""
import numpy as np
import pytest

import _feat_cases as FC
import _featdef as FD

RTOL, ATOL = 1e-12, 1e-14


def _assert_rows(got, want, cols, skip=None, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~np.isclose(got, want, rtol=RTOL, atol=ATOL)
    if skip is not None:
        bad[:, skip] = False
    if bad.any():
        i, j = np.argwhere(bad)[0]
        raise AssertionError("%s: %d cells differ, first at row %d column %d (%s): %r vs %r" %
                             (what, int(bad.sum()), i, j, cols[j], got[i, j], want[i, j]))


def test_names_are_complete():
    for n in FC.NAMES:
        FC.case(n)
    assert len(set(FC.NAMES)) == len(FC.NAMES)


@pytest.mark.parametrize("name", FC.NAMES)
def test_oracle_rows_match_the_definitions(name):
    from oracle import pyoracle as O
    c = FC.case(name)
    want = FC.definition_rows(name)
    got = FC.oracle_rows(name)
    cols = c.columns()
    # D_f: the formula of the classes' dim() members, the oracle's orc_feat_dim, and both row lengths
    extra = 5 if c.saliency is not None and not c.flags["use_simple"] else 0
    assert len(cols) == c.feat_dim() == want.shape[1] == O.feat_dim(c.dim, c.oracle_cfg()) + extra
    assert len(want) == len(c.order) > 0
    _assert_rows(got, want, cols, skip=c.std_mask() if c.edge else None, what=name)


def test_boxes_closed_form():
    """the hand-derived literals of _feat_cases.py against the definition and the oracle"""
    c = FC.case("geom/boxes")
    cols = c.columns()
    for rows in (FC.definition_rows("geom/boxes"), FC.oracle_rows("geom/boxes")):
        assert rows.shape == (1, 104)
        for k, v in FC.BOXES_LITERALS.items():
            assert rows[0, cols.index(k)] == pytest.approx(v, rel=1e-15, abs=0), k


def test_equal_areas_do_not_swap():
    """main_bc_feat.cxx:86 swaps on strictly greater area: with equal areas x1 is the order's x0, so the two label orders give
    rows with x1 and x2 exchanged"""
    a, b = FC.definition_rows("geom/equal_ab"), FC.definition_rows("geom/equal_ba")
    cols = FC.case("geom/equal_ab").columns()
    x1 = [i for i, n in enumerate(cols) if n.startswith("x1.")]
    x2 = [i for i, n in enumerate(cols) if n.startswith("x2.")]
    assert (a[:, x1] == b[:, x2]).all() and (a[:, x2] == b[:, x1]).all()
    assert not (a[:, x1] == a[:, x2]).all()
    assert a[0, cols.index("x1.area")] == a[0, cols.index("x2.area")] == 48.0


def test_geometry_cases_reach_their_rules():
    """each geometry really has what it was built for"""
    g = FC.definition_geometry("plates")
    assert any((b, a) not in g.leaf_bnd for (a, b) in g.leaf_bnd), "a pair that exists in one direction only"
    assert any(len(p) == 1 for p in g.leaf_pts.values()), "a one-voxel region"
    rows, cols = FC.definition_rows("geom/plates"), FC.case("geom/plates").columns()
    assert (rows[:, [cols.index("x1.bbox%d" % i) for i in range(3)]] == 0).any(), "a bounding-box extent of 0"
    last = g.order[-1][2]
    assert len(g.lists[last][0]) == g.labels.size, "the last region is the whole volume"
    left = set(g.regions[last].bnd)
    assert left and all((b, a) not in g.leaf_bnd for (a, b) in left), "only the pairs without a reverse stay inside it (region.hxx:70-73)"
    g = FC.definition_geometry("not_adjacent")
    assert len(FD.get_boundary(g.regions[1], g.regions[3])) == 0
    assert FC.definition_rows("geom/not_adjacent")[0, FC.case("geom/not_adjacent").columns().index("x0.blen")] == 0.0
    m = FC.case("geom/masked")
    assert 0.1 < 1.0 - m.mask.mean() < 0.35 and sum(len(p) for p in FC.definition_geometry("masked").leaf_pts.values()) == int(m.mask.sum())


@pytest.mark.parametrize("name", [n for n in FC.NAMES if n.startswith("thr/") and n.endswith("/q8")] + ["spec/b16/q8", "spec/b16_labels/q8", "spec/b16_01_09/q8", "spec/b6_05_75/q8"])
def test_q8_values_hit_thresholds_and_bounds(name):
    """the Q8 images are arranged so that values sit exactly ON thresholds and dyadic bin bounds -- on boundary voxels too"""
    c = FC.case(name)
    img = c.images[c.pb]
    g = FC.definition_geometry(c.geom)
    bvox = np.unique(np.concatenate([np.asarray(v) for v in g.leaf_bnd.values()]))
    if name.startswith("thr/"):
        for t in set(c.thr) - {0.8, 0.2}:                          # 0.2 and 0.8 are no Q8 values
            assert (img.ravel()[bvox] == np.float32(t)).sum() > 0, t
    else:
        _, bins, lo, hi = c.lists["rb"][0]
        inner = [b for b in FD.hist_bounds(bins, lo, hi) if lo < b < hi]
        assert sum(int((img == np.float32(b)).sum()) for b in inner) > 0


@pytest.mark.parametrize("name", [n for n in FC.NAMES if n.endswith("/edge")])
def test_edge_images_hold_every_edge_value(name):
    c = FC.case(name)
    _, bins, lo, hi = c.lists["rb"][0]
    vals = FC.edge_values((bins, lo, hi), c.thr)
    assert set(np.unique(c.images[c.pb]).tolist()) == set(vals.tolist())
    # the accumulated bounds differ from (i + 1) * interval for the non-dyadic specs -- that is what these images are for
    if bins in (7, 10, 13):
        interval = (hi - lo) / bins
        assert any(b != (i + 1) * interval for i, b in enumerate(FD.hist_bounds(bins, lo, hi)))


@pytest.mark.parametrize("name", FC.LOOP_NAMES)
def test_oracle_merge_loop_rows_match_the_definitions(name):
    """rows the classifier merge loop records (orc_merge_order_bc, want_feats) for the order it chooses itself"""
    c = FC.case(name)
    cols = c.columns()
    stub = cols.index("x0.b0.mean")
    order, sal, feats = c.oracle_rag().merge_order_bc(c.oracle_cfg(), None, stub_index=stub, want_feats=True)
    assert len(order) > 0
    want = c.definition_rows(order=order, order_key=name + "/loop")
    _assert_rows(feats, want, cols, what=name)


@pytest.mark.parametrize("name,value", [("spec/b16_01_09/q8", 0.75), ("spec/b6_05_75/q8", 7.0)])
def test_accumulated_bounds_are_observable(name, value):
    """bounds[i] = bounds[i-1] + interval (util/image_stats.hxx:20-22) is not (i + 1) * interval: at these two specs an image
    value lies between the two, so a histogram built on products differs -- the cases are there to notice that"""
    c = FC.case(name)
    _, bins, lo, hi = c.lists["rb"][0]
    img = c.images[c.pb]
    assert (img == np.float32(value)).sum() > 0
    acc = FD.hist_bounds(bins, lo, hi)
    prod = [(i + 1) * ((hi - lo) / bins) for i in range(bins)]
    assert any(p <= value < a for a, p in zip(acc, prod))
    h_acc = FD.histc(img.ravel(), bins, lo, hi)
    first_below = lambda v, bounds: next((i for i, b in enumerate(bounds) if v < b), None)
    assert first_below(value, acc) != first_below(value, prod)
    assert h_acc[first_below(value, acc)] > 0
