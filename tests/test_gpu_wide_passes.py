"""-m gpu: contractions of every width class of the batch kernel (glia_amd/csrc/greedy_batch.hpp) in ONE run, under the settings that
make every pass push, spill, evict, or leave the kernel with list links still pending.

The input is a hub image: 180 x 180, background = label 1, a 30 x 30 grid of 6 x 6 cells each holding a 3 x 4 blob split into two
3 x 2 labels -- 1801 regions, and the background starts with 1800 list entries.  As the hub absorbs blobs its list shrinks, so its
contractions cross the classes the kernel treats differently:
    more than 1408 entries   the whole workgroup, neighbour matching on the global mark arrays
    1025 .. 1408             the whole workgroup on the LDS table, three entries per lane
    513 .. 1024              two entries per lane
    193 .. 512               one
    129 .. 192, 65 .. 128    one wave (a batch member), three / two entries per lane
That they are crossed is not assumed: the tree kernel's order is replayed on the CPU with neighbour sets and list lengths, and every
class has to be hit by at least 20 merges (test_every_width_class_is_hit).  A class is counted from both sides: the live neighbours
of the two regions are a LOWER bound of the entries the contraction reads, the list lengths by the kernel's rule (a list is created
with one entry per distinct neighbour and never changes its length: an entry is reused in place or becomes a tombstone) the count
itself; a merge counts for a class only if the lower bound is inside it and the length is at least kMargin below its upper edge.

Every setting is compared byte for byte with the tournament-tree kernel (GLIA_HMT_PB_WINDOW=0), which shares no queue code with the
batch kernel, and with the one-at-a-time window kernel (GLIA_HMT_PB_BATCH=0)."""
import numpy as np
import pytest

from _hub_cases import CLASSES, hub_image, kGrid, kMargin, kRegions, width_classes      # noqa: F401 (kGrid, kMargin: part of the case)

pytestmark = pytest.mark.gpu

SETTINGS = [dict(), dict(GLIA_HMT_HORIZON=0), dict(GLIA_HMT_WINCAP=32), dict(GLIA_HMT_WINCAP=16, GLIA_HMT_REBASE=300), dict(GLIA_HMT_REBASE=100),
            dict(GLIA_HMT_FORCE_TREE=200)]


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


_cache = {}


def _hub_case(ctx, levels):
    """the image on the device, the tree kernel's order and the one-at-a-time window kernel's, computed once per module"""
    if levels not in _cache:
        import torch
        lab, pb = hub_image(levels)
        d_lab, d_pb = torch.from_numpy(lab.view(np.int32)).cuda(), torch.from_numpy(pb).cuda()
        _cache[levels] = (lab, d_lab, d_pb, _order(ctx, d_lab, d_pb, GLIA_HMT_PB_WINDOW=0), _order(ctx, d_lab, d_pb, GLIA_HMT_PB_BATCH=0))
    return _cache[levels]


def _same(got, ref):
    return got[0].shape == ref[0].shape and (got[0] == ref[0]).all() and (got[1] == ref[1]).all()


@pytest.mark.parametrize("levels", [None, 4])
def test_every_width_class_is_hit(ctx, levels):
    lab, _, _, tree, _ = _hub_case(ctx, levels)
    assert len(tree[0]) == kRegions - 1
    hits = width_classes(lab, tree[0])
    print("levels %s: %s" % (levels, ", ".join("%s %d" % (c[0], h) for c, h in zip(CLASSES, hits))))
    for (name, _, _), h in zip(CLASSES, hits):
        assert h >= 20, (name, h)
    if levels:      # exact ties: fewer than half as many distinct saliencies as merges, so the seq decides most of the order
        assert len(np.unique(tree[1])) * 2 < len(tree[0])


@pytest.mark.parametrize("levels", [None, 4])
@pytest.mark.parametrize("env", SETTINGS)
def test_wide_passes_on_the_hub_image(ctx, levels, env):
    from glia_amd import hmt
    _, d_lab, d_pb, tree, seq = _hub_case(ctx, levels)
    before = hmt.Context.internal_errors()
    got = _order(ctx, d_lab, d_pb, **env)
    assert _same(got, tree), ("against the tree kernel", env)
    assert _same(got, seq), ("against the one-at-a-time window kernel", env)
    assert hmt.Context.internal_errors() == before == 0
