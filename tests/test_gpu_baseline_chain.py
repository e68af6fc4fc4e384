"""-m gpu: the baseline chain of the pb-mean window queue (glia_amd/csrc/greedy_baseline.hpp, WinBaseline): the collection pass that takes
seq and saliency key from the list entries, its two lane-group widths, the sorts on compact arrays, the per-cell segments, and the
threshold that starts at the top occupied cell.

Every run is compared bit for bit with the tournament-tree kernel (GLIA_HMT_PB_WINDOW=0), which has no baseline, and runs with
GLIA_HMT_BASELINE_AUDIT=1: one checking kernel behind every baseline (entry keys against the records, the sorted order, the
segments and counts, nothing above the starting threshold); a mismatch ends the call with GLIA_HMT_ERR_INTERNAL.

There is no test that corrupts a key to see the audit stop a call: such a call counts in glia_hmt_internal_errors(), which the
session's closing check (tests/conftest.py) wants at 0, and nothing resets the counter."""
import numpy as np
import pytest

from _pb_cases import AUDIT, HUB_L, _case, _order, _same

pytestmark = pytest.mark.gpu

SETS = [dict(), dict(GLIA_HMT_REBASE=200), dict(GLIA_HMT_HORIZON=0.25, GLIA_HMT_REBASE=5000), dict(GLIA_HMT_HORIZON=0),
        dict(GLIA_HMT_WINCAP=64, GLIA_HMT_REBASE=400), dict(GLIA_HMT_MINCAP=1, GLIA_HMT_REBASE=300)]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    c.close()


def test_the_large_volume_places_a_horizon_and_the_small_one_does_not(ctx):
    assert _case(ctx, "large")[2][2] > 6000 and len(_case(ctx, "large")[2][0]) > 3000
    assert 0 < _case(ctx, "small")[2][2] < 4096


@pytest.mark.parametrize("env", SETS)
def test_orders_under_frequent_baselines(ctx, env):
    from glia_amd import hmt
    d_lab, d_pb, tree = _case(ctx, "large")
    before = hmt.Context.internal_errors()
    got = _order(ctx, d_lab, d_pb, **env, **AUDIT)
    assert _same(got, tree), env
    assert hmt.Context.internal_errors() == before


def test_orders_without_a_horizon(ctx):
    from glia_amd import hmt
    d_lab, d_pb, tree = _case(ctx, "small")
    before = hmt.Context.internal_errors()
    assert _same(_order(ctx, d_lab, d_pb, GLIA_HMT_REBASE=100, **AUDIT), tree)
    assert hmt.Context.internal_errors() == before


def test_the_record_scan_feeds_the_same_chain(ctx):
    """the one-at-a-time window kernel collects from the edge records (win_collect_kernel) and takes its saliency keys from them"""
    from glia_amd import hmt
    d_lab, d_pb, tree = _case(ctx, "large")
    before = hmt.Context.internal_errors()
    assert _same(_order(ctx, d_lab, d_pb, GLIA_HMT_PB_BATCH=0, GLIA_HMT_REBASE=200, **AUDIT), tree)
    assert hmt.Context.internal_errors() == before


@pytest.mark.parametrize("env", [dict(GLIA_HMT_FORCE_TREE=1500), dict(GLIA_HMT_FORCE_TREE=700, GLIA_HMT_REBASE=400)])
def test_hand_over_collects_from_the_lists(ctx, env):
    """ST_NEED_TREE: the collection pass lists the live edges (and rebuilds their records) for the tree kernel"""
    from glia_amd import hmt
    d_lab, d_pb, tree = _case(ctx, "large")
    before = hmt.Context.internal_errors()
    assert _same(_order(ctx, d_lab, d_pb, **env, **AUDIT), tree), env
    assert hmt.Context.internal_errors() == before


@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("L", HUB_L)
def test_list_lengths_around_the_group_widths(ctx, L, lanes):
    """a list of exactly L entries, walked by groups of 16 and of 64 lanes; a baseline every 4 created edges, so that many fall
    while the hub is alive"""
    from glia_amd import hmt
    d_lab, d_pb, tree = _case(ctx, L)
    assert len(tree[0]) == L
    if L > 1:
        assert len(np.unique(tree[1])) == L           # distinct means
    before = hmt.Context.internal_errors()
    got = _order(ctx, d_lab, d_pb, GLIA_HMT_REBASE=3, GLIA_HMT_COLLECT_LANES=lanes, **AUDIT)
    assert _same(got, tree), (L, lanes)
    assert hmt.Context.internal_errors() == before


@pytest.mark.parametrize("name", ["constant", "two-valued"])
def test_degenerate_saliency_ranges(ctx, name):
    """one cell holds everything (constant pb), or nearly so: the order must match whether the window queue finishes or hands
    over to the tree kernel"""
    from glia_amd import hmt
    d_lab, d_pb, tree = _case(ctx, name)
    if name == "constant":
        assert len(np.unique(tree[1])) == 1
    before = hmt.Context.internal_errors()
    assert _same(_order(ctx, d_lab, d_pb, GLIA_HMT_REBASE=100, **AUDIT), tree)
    assert hmt.Context.internal_errors() == before
