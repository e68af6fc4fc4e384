"""-m gpu: the batch kernel's window scan reads only the blocks of 512 slots below the window's fill, and finds every wave's best
and second-best item in one reduction (exact saliency ties go by seq).  With window capacities on and around every block
boundary the fill crosses them all the time; the batch kernel's merge order must stay byte-identical to that of the
tournament-tree kernel (GLIA_HMT_PB_WINDOW=0), on volumes with massive exact ties and on one without."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAPS = [511, 512, 513, 1023, 1024, 1025, 1536]


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


def _synth(ctx, shape, S, variant, levels):
    import torch
    labels, pb = ctx.synth(shape, S, 4 * S, variant=variant)
    if levels:
        pb = torch.floor(pb * levels) / levels            # few distinct boundary values: massive exact ties
    return labels, pb.contiguous()


def _constant(ctx):
    import torch
    from oracle import pyoracle as O
    labels, _ = O.synth((48, 48, 48), 4, 8)
    pb = np.full(labels.shape, 0.25, np.float32)          # every saliency equal: the order is the tie rule alone
    return torch.from_numpy(labels.view(np.int32)).cuda(), torch.from_numpy(pb).cuda()


VOLUMES = {
    "levels4": lambda ctx: _synth(ctx, (96, 80, 64), 6, 0, 4),
    "constant": _constant,
    "no_ties": lambda ctx: _synth(ctx, (128, 128, 128), 8, 1, None),
}


@pytest.fixture(scope="module")
def trees(ctx):
    cache = {}

    def get(name):
        if name not in cache:
            d_lab, d_pb = VOLUMES[name](ctx)
            cache[name] = (d_lab, d_pb, _order(ctx, d_lab, d_pb, GLIA_HMT_PB_WINDOW=0))
        return cache[name]
    return get


@pytest.mark.parametrize("volume", list(VOLUMES))
@pytest.mark.parametrize("cap", CAPS)
def test_batch_equals_tree_around_block_boundaries(trees, ctx, volume, cap):
    d_lab, d_pb, tree = trees(volume)
    assert len(tree[0]) > 500
    o, s = _order(ctx, d_lab, d_pb, GLIA_HMT_WINCAP=cap)
    assert o.shape == tree[0].shape and (o == tree[0]).all() and (s == tree[1]).all()
