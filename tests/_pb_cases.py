"""The shared cases of test_gpu_baseline_chain.py and test_gpu_collect_blocks.py: volumes whose pb-mean merge order exercises the
baseline chain of the window queue (glia_amd/csrc/greedy_baseline.hpp), each with the order of the tournament-tree kernel
(GLIA_HMT_PB_WINDOW=0), which has no baseline."""
import numpy as np

AUDIT = dict(GLIA_HMT_BASELINE_AUDIT=1)
# 32 | 33: the longest list a group of 16 lanes walks (and the block counts), the shortest it leaves to its wave
HUB_L = [1, 15, 16, 17, 32, 33, 63, 64, 65, 130]


def _order(ctx, d_lab, d_pb, **env):
    from glia_amd import hmt
    with hmt.options(**env):
        rm = hmt.RegionMap(ctx, d_lab, pb=d_pb, only_contour=True)
        o, s = rm.merge_order_pb(type=2)
        n_edges = rm.num_pairs // 2               # directed pairs / 2: at least the initial edges (a table edge needs both directions)
        rm.close()
    return o, s, n_edges


def _same(got, ref):
    return got[0].shape == ref[0].shape and (got[0] == ref[0]).all() and (got[1] == ref[1]).all()


def hub_image(L):
    """A hub with exactly L neighbours: L columns, one voxel wide and three high (labels 1 .. L), stand two voxels apart in a hub
    (label L + 1) that fills the rest -- a plane under the columns and the gaps between them.  A voxel belongs to the boundary with
    its first differing neighbour (x - 1 first), and a table edge needs both directions: a column's voxels see the hub on their
    left, the hub's voxels right of a column see the column, columns never touch.  So the L edges all end at the hub: the columns
    have lists of one entry, every merge re-creates the hub's remaining edges (a list of L - 1, L - 2, ... entries), the newest region
    holds them all, and all of them share a block of the collection pass as long as there are at most 16 regions.  pb is seeded
    random Q16: the boundary means are distinct."""
    lab = np.full((5, 2 * L + 1), L + 1, np.uint32)
    lab[:3, 1::2] = np.arange(1, L + 1, dtype=np.uint32)[None, :]
    pb = np.random.default_rng(20261020 + L).integers(0, 1 << 16, lab.shape).astype(np.float32) / np.float32(1 << 16)
    return lab, pb


_cache = {}


def _case(ctx, name):
    """a volume on the device and the tree kernel's order, computed once per context (a test module's)"""
    if (ctx, name) not in _cache:
        import torch
        if name == "large":                       # ~4 k regions, more than 4096 live edges: horizons are placed, the first baseline fills the cap
            d_lab, d_pb = ctx.synth((64, 64, 64), 4, 32)
        elif name == "small":                     # fewer than 4096 edges: no horizon is placed
            d_lab, d_pb = ctx.synth((32, 32, 32), 8, 32)
        elif name == "constant":                  # smax == smin: scale 0, every item in cell 0, every key the same
            d_lab, _ = ctx.synth((32, 32, 32), 8, 32)
            d_pb = torch.full((32, 32, 32), 0.5, dtype=torch.float32, device=d_lab.device)
        elif name == "two-valued":
            d_lab, pb = ctx.synth((32, 32, 32), 8, 32)
            d_pb = (torch.floor(pb * 2) / 2).contiguous()
        else:
            lab, pb = hub_image(name)
            d_lab, d_pb = torch.from_numpy(lab.view(np.int32)).cuda(), torch.from_numpy(pb).cuda()
        _cache[(ctx, name)] = (d_lab, d_pb, _order(ctx, d_lab, d_pb, GLIA_HMT_PB_WINDOW=0))
    return _cache[(ctx, name)]
