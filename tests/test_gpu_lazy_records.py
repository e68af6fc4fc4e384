"""-m gpu: the batch kernel writes no edge record for an edge it creates below the horizon; the baseline's collection pass walks the
lists of the live regions and rebuilds the records of the survivors from their list entries (glia_amd/csrc/edge_record.hpp).

Every case compares orders and saliencies byte for byte with the tournament-tree kernel (GLIA_HMT_PB_WINDOW=0), which runs none of
that code, and reads from the GLIA_HMT_TRACE lines (captured at file-descriptor level: the library writes them to fd 2) that records
WERE rebuilt -- no case passes without running the new path.  Volumes: the 128^3 synthetic volume of test_gpu_queue.py in both pb
variants, a volume with four pb levels (massive exact ties: the rebuilt seq, cat bits included, decides the order), and a hub image
whose background region starts with 10 368 list entries (contractions on the global mark arrays, win_complete_r2 on lazy edges)."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SETTINGS = [dict(GLIA_HMT_REBASE=2000), dict(GLIA_HMT_HORIZON=0.05, GLIA_HMT_REBASE=1000), dict(GLIA_HMT_HORIZON=8, GLIA_HMT_REBASE=20000),
            dict(GLIA_HMT_MINCAP=1, GLIA_HMT_REBASE=2000)]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    c.close()


def _order(ctx, d_lab, d_pb, **env):
    from glia_amd import hmt
    with hmt.options(**env):
        rm = hmt.RegionMap(ctx, d_lab, pb=d_pb, only_contour=True)
        o, s = rm.merge_order_pb(type=2)
        rm.close()
    return o, s


def _traced(ctx, capfd, d_lab, d_pb, **env):
    """the order under env, and the records its baselines rebuilt (sum over the trace lines of the launches)"""
    capfd.readouterr()
    o, s = _order(ctx, d_lab, d_pb, GLIA_HMT_TRACE=1, **env)
    err = capfd.readouterr().err
    counts = [int(m) for m in re.findall(r"merge loop launch ended:.*records rebuilt (\d+)", err)]
    assert counts, "no trace line: " + err[-400:]
    return o, s, sum(counts), len(counts)


_cache = {}


def _synth_case(ctx, shape, S, variant, levels):
    """volume and the tree kernel's order, computed once per module"""
    key = (shape, S, variant, levels)
    if key not in _cache:
        import torch
        labels, pb = ctx.synth(shape, S, 4 * S, variant=variant)
        if levels:
            pb = torch.floor(pb * levels) / levels
        pb = pb.contiguous()
        _cache[key] = (labels, pb, _order(ctx, labels, pb, GLIA_HMT_PB_WINDOW=0))
    return _cache[key]


def _hub_case(ctx, levels):
    """432 x 432, background = label 1, a 72 x 72 grid of 6 x 6 cells each holding a 3 x 4 blob split into two 3 x 2 labels: 10 369
    regions, 15 552 initial edges, and the background starts with 10 368 list entries.  pb: seeded random Q8 values (floored to
    `levels` levels if given)."""
    key = ("hub", levels)
    if key not in _cache:
        import torch
        lab = np.ones((432, 432), np.uint32)
        nxt = 2
        for cy in range(72):
            for cx in range(72):
                y, x = 6 * cy + 1, 6 * cx + 1
                lab[y:y + 3, x:x + 2] = nxt
                lab[y:y + 3, x + 2:x + 4] = nxt + 1
                nxt += 2
        assert nxt - 1 == 10369
        pb = np.random.default_rng(20250921).integers(0, 256, lab.shape).astype(np.float32) / np.float32(256)
        if levels:
            pb = np.floor(pb * levels).astype(np.float32) / np.float32(levels)
        d_lab, d_pb = torch.from_numpy(lab.view(np.int32)).cuda(), torch.from_numpy(pb).cuda()
        _cache[key] = (d_lab, d_pb, _order(ctx, d_lab, d_pb, GLIA_HMT_PB_WINDOW=0))
    return _cache[key]


def _same(got, tree):
    return got[0].shape == tree[0].shape and (got[0] == tree[0]).all() and (got[1] == tree[1]).all()


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("env", SETTINGS)
def test_lazy_records_on_the_synthetic_volume(ctx, capfd, variant, env):
    d_lab, d_pb, tree = _synth_case(ctx, (128, 128, 128), 8, variant, None)
    assert len(tree[0]) == 4095
    o, s, rebuilt, launches = _traced(ctx, capfd, d_lab, d_pb, **env)
    print("variant %d %s: %d launches, %d records rebuilt" % (variant, env, launches, rebuilt))
    assert _same((o, s), tree)
    assert rebuilt > 0


@pytest.mark.parametrize("env", SETTINGS)
def test_lazy_records_under_massive_ties(ctx, capfd, env):
    """four pb levels: most saliencies are shared by many edges, so the seq -- for a rebuilt record: merge number, cat bits and
    neighbour put together again -- decides the order"""
    d_lab, d_pb, tree = _synth_case(ctx, (96, 80, 64), 6, 0, 4)
    # fewer than half as many distinct saliencies as merges: on average a saliency is shared by more than two pops, so the seq
    # decides most of the order (a property of the input, taken from the tree kernel's order)
    assert len(tree[0]) > 500 and len(np.unique(tree[1])) * 2 < len(tree[0])
    o, s, rebuilt, launches = _traced(ctx, capfd, d_lab, d_pb, **env)
    print("ties %s: %d launches, %d records rebuilt, %d distinct saliencies in %d merges" % (env, launches, rebuilt, len(np.unique(tree[1])), len(tree[0])))
    assert _same((o, s), tree)
    assert rebuilt > 0


@pytest.mark.parametrize("levels", [None, 4])
@pytest.mark.parametrize("env", [dict(), dict(GLIA_HMT_REBASE=300), dict(GLIA_HMT_FORCE_TREE=200), dict(GLIA_HMT_FORCE_TREE=200, GLIA_HMT_REBASE=300)])
def test_lazy_records_on_the_hub_image(ctx, capfd, levels, env):
    """contractions of more than kMarkMax (1408) list entries while the horizon is on: r2's list length is completed afterwards
    (win_complete_r2), which must leave the unwritten records of lazy edges alone; with GLIA_HMT_FORCE_TREE the tournament-tree
    kernel takes over with lazy edges outstanding (the hand-over rebuilds them first)"""
    d_lab, d_pb, tree = _hub_case(ctx, levels)
    assert len(tree[0]) == 10368
    o, s, rebuilt, launches = _traced(ctx, capfd, d_lab, d_pb, **env)
    print("hub levels %s %s: %d launches, %d records rebuilt, %d distinct saliencies" % (levels, env, launches, rebuilt, len(np.unique(tree[1]))))
    assert _same((o, s), tree)
    assert rebuilt > 0


@pytest.mark.parametrize("variant", [0, 1])
def test_no_horizon_no_rebuild(ctx, capfd, variant):
    """GLIA_HMT_HORIZON=0: every record is written when its edge is created, nothing is rebuilt, the order is the same"""
    d_lab, d_pb, tree = _synth_case(ctx, (128, 128, 128), 8, variant, None)
    for env in (dict(GLIA_HMT_HORIZON=0), dict(GLIA_HMT_HORIZON=0, GLIA_HMT_REBASE=2000)):
        o, s, rebuilt, launches = _traced(ctx, capfd, d_lab, d_pb, **env)
        assert _same((o, s), tree), env
        assert rebuilt == 0, env
    assert launches > 1
