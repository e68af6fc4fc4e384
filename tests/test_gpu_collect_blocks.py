"""-m gpu: the block-counted collection pass of the pb-mean window queue's baselines (glia_amd/csrc/greedy_baseline.hpp,
win_collect_lists_kernel) and the shorter interval at the end of a run (GLIA_HMT_REBASE_END).

The pass runs twice over the lists -- it counts, a scan turns the counts into ranges, it writes -- and shares no counter.  A block
of the 16-lane pass holds sixteen regions.  Their short lists (at most 32 entries) are counted by the block and written into the
block's range; the long lists among them are walked by their wave behind the block's barrier, into the wave's range.  A dead region,
a region past the last one and a long list count as nothing in front of the barrier.  The cases below put every one of these into a block
together with lists that do count, at many values of the region count: small GLIA_HMT_REBASE values give a run tens of baselines.

Every run is compared byte for byte (order and saliencies) with the tournament-tree kernel (GLIA_HMT_PB_WINDOW=0), which has no
baseline, and runs with GLIA_HMT_BASELINE_AUDIT=1: a checking kernel behind every baseline (collected keys against the records,
the sorted order -- which the key sort now reaches without looking at the bits all keys share -- the segments and the counts).
No test provokes an error."""
import re

import numpy as np
import pytest

from _pb_cases import AUDIT, HUB_L, _case, _order, _same

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    c.close()


def _check(ctx, name, **env):
    from glia_amd import hmt
    d_lab, d_pb, tree = _case(ctx, name)
    before = hmt.Context.internal_errors()
    got = _order(ctx, d_lab, d_pb, **env, **AUDIT)
    assert _same(got, tree), (name, env)
    assert hmt.Context.internal_errors() == before
    return tree


@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("L", HUB_L)
def test_short_and_long_lists_share_a_block(ctx, L, lanes):
    """a hub of exactly L neighbours among lists of one entry.  With a baseline every 3 created edges the hub's list passes every
    length from L down, across the 32 | 33 boundary between the block's count and the wave's walk; every 200, the larger hubs
    still see tens of baselines"""
    for rebase in (3, 200):
        tree = _check(ctx, L, GLIA_HMT_REBASE=rebase, GLIA_HMT_COLLECT_LANES=lanes)
    assert len(tree[0]) == L
    if L > 1:
        assert len(np.unique(tree[1])) == L           # distinct means


@pytest.mark.parametrize("rebase", [25, 200, 400])
def test_blocks_that_contribute_nothing(ctx, rebase):
    """64 regions, four blocks at the start, run to the end: the late baselines see blocks whose sixteen regions are all dead, and
    a last block cut by the region count (64 + merges).  The volume creates a few hundred edges: an interval of 25 gives it the
    tens of baselines that 200 and 400 give the larger ones"""
    tree = _check(ctx, "small", GLIA_HMT_REBASE=rebase, GLIA_HMT_COLLECT_LANES=16)
    assert len(tree[0]) > 48                          # more merges than three blocks hold regions: whole blocks die


@pytest.mark.parametrize("end", [1, 64])
@pytest.mark.parametrize("env", [dict(GLIA_HMT_REBASE=300), dict(GLIA_HMT_HORIZON=0.25, GLIA_HMT_REBASE=5000)])
def test_more_than_4096_live_edges(ctx, capfd, env, end):
    """horizons are placed and the first baseline returns exactly as many items as there is room for.  The trace shows the interval
    of every launch: the usual one wherever a horizon stands, and nothing else at factor 1"""
    capfd.readouterr()
    tree = _check(ctx, "large", GLIA_HMT_TRACE=1, GLIA_HMT_REBASE_END=end, **env)
    err = capfd.readouterr().err
    launches = [(int(h), int(i)) for h, i in re.findall(r"merge loop launch ended:.*horizon (\d+), interval (\d+)", err)]
    print("%s end %d: %d launches, %d with a horizon, %d with a shorter interval" % (
        env, end, len(launches), sum(h > 0 for h, _ in launches), sum(i != env["GLIA_HMT_REBASE"] for _, i in launches)))
    assert len(tree[0]) > 3000 and len(launches) > 1
    assert any(h > 0 for h, _ in launches)
    if end > 1:                                       # the run ends below 4096 live edges, where no horizon is placed
        assert launches[-1] == (0, env["GLIA_HMT_REBASE"] // end), launches[-3:]
    for h, i in launches:
        assert i in (env["GLIA_HMT_REBASE"], max(1, env["GLIA_HMT_REBASE"] // end)), launches
        if h > 0 or end == 1:
            assert i == env["GLIA_HMT_REBASE"], launches


@pytest.mark.parametrize("name", ["constant", "two-valued"])
def test_scale_zero_and_massive_ties(ctx, name):
    """every item in cell 0 and no key bit that differs (constant pb), or two values"""
    for rebase in (25, 200):
        tree = _check(ctx, name, GLIA_HMT_REBASE=rebase)
    if name == "constant":
        assert len(np.unique(tree[1])) == 1
