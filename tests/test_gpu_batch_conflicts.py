"""-m gpu: the batch kernel's conflict test between the members of a round (glia_amd/csrc/greedy_batch.hpp, rule (b) of its header).

A round commits member j only if its two regions are neither an earlier member's regions nor neighbours of them.  The cheap filter
for that is a 2048-bit map per member, indexed by region id mod 2048; a pair the filter flags is then decided exactly, by the earlier
member's wave, from the list entries it holds in registers.  The cases below are the smallest at which that decision can go wrong:

    ties, q8        4096 regions: ids i and i + 2048 exist, so the filter flags pairs that share nothing (few levels: massive ties)
    created         6144 regions: the ids of created regions (R0 + k) share residues with initial ones from the first merge on
    constant        every saliency ties: the top of the queue is chains of adjacent edges, the flagged pairs are true conflicts
    chain           4100 slabs in a row whose three best edges are (10, 11), (2058, 2059) and (11, 12): the second collides with the
                    first in the filter and shares nothing with it, the third shares region 11 with the first
    hub10, hub30    hub images: members near the 192-entry limit, whose maps are dense (nearly every pair is flagged), and wide
                    contractions at rank > 0

Every case runs under the default window, under a tiny one and under a small one with frequent re-baselines (longer prefixes fill the
window faster: compaction and spill), and is compared byte for byte with the tournament-tree kernel (GLIA_HMT_PB_WINDOW=0), the
one-at-a-time window kernel (GLIA_HMT_PB_BATCH=0) and the CPU oracle.  The tests cannot see batching itself (the profiling build's
counters do); a wrong decision shows as a different order."""
import numpy as np
import pytest

from _hub_cases import hub_image

pytestmark = pytest.mark.gpu

CASES = ["ties", "q8", "created", "constant", "chain", "hub10", "hub10-ties", "hub30", "hub30-ties"]
SETTINGS = [dict(), dict(GLIA_HMT_WINCAP=32), dict(GLIA_HMT_WINCAP=64, GLIA_HMT_REBASE=300)]
kChain = 4100
kChainBest = [(10, 11), (2058, 2059), (11, 12)]


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


def chain_image():
    """labels (uint32) and pb (float32) of the chain: 2 x 2 kChain pixels, slab L (1 .. kChain) holds columns 2 L - 2 and 2 L - 1.  A
    pixel belongs to the boundary with its first differing neighbour (x - 1 first): a slab's left column to the slab on its left, its
    right column to the one on its right, so edge (L, L + 1) is the mean of columns 2 L - 1 and 2 L.  Those are 0, 1 / 256 and 2 / 256
    for the three edges of kChainBest, in that order, and seeded random Q8 in [0.5, 1) everywhere else."""
    lab = np.repeat(np.arange(1, kChain + 1, dtype=np.uint32), 2)[None, :].repeat(2, axis=0)
    pb = np.random.default_rng(20261021).integers(128, 256, lab.shape).astype(np.float32) / np.float32(256)
    for rank, (a, _) in enumerate(kChainBest):
        pb[:, 2 * a - 1:2 * a + 1] = np.float32(rank) / np.float32(256)
    return np.ascontiguousarray(lab), pb


_cache = {}


def _case(ctx, name):
    """the image on the device and the orders of the tree kernel, the one-at-a-time window kernel and the oracle, once per module"""
    if name not in _cache:
        import torch
        from oracle import pyoracle as O
        if name in ("ties", "q8", "constant", "created"):
            d_lab, d_pb = ctx.synth((96, 64, 64) if name == "created" else (64, 64, 64), 4, 16)
            if name == "ties":
                d_pb = (torch.floor(d_pb * 4) / 4).contiguous()
            if name == "constant":
                d_pb = torch.full_like(d_pb, 0.25)
            lab, pb = d_lab.cpu().numpy().view(np.uint32), d_pb.cpu().numpy()
        else:
            lab, pb = chain_image() if name == "chain" else hub_image(4 if name.endswith("-ties") else None, grid=int(name[3:5]))
            d_lab, d_pb = torch.from_numpy(lab.view(np.int32)).cuda(), torch.from_numpy(pb).cuda()
        _cache[name] = (lab, d_lab, d_pb, _order(ctx, d_lab, d_pb, GLIA_HMT_PB_WINDOW=0), _order(ctx, d_lab, d_pb, GLIA_HMT_PB_BATCH=0),
                        O.Rag(lab, only_contour=True).merge_order_pb(pb, type=2))
    return _cache[name]


def _same(got, ref):
    return got[0].shape == ref[0].shape and (got[0] == ref[0]).all() and (got[1] == ref[1]).all()


def test_the_cases_are_what_they_claim(ctx):
    """region counts above 2048 / 4096, tie-heavy and tie-free saliencies, and the chain's first three merges as constructed"""
    for name, regions in (("ties", 4096), ("q8", 4096), ("constant", 4096), ("created", 6144), ("chain", kChain), ("hub10", 201), ("hub30", 1801)):
        lab, _, _, tree, _, cpu = _case(ctx, name)
        assert len(np.unique(lab)) == regions and len(tree[0]) == len(cpu[0]) == regions - 1, name
    # exact ties: with four levels fewer than a quarter as many distinct saliencies as merges, and fewer than half as many as with 256
    distinct = {name: len(np.unique(_case(ctx, name)[5][1])) for name in ("ties", "q8", "constant")}
    assert distinct["ties"] * 4 < 4095 and distinct["ties"] * 2 < distinct["q8"] and distinct["constant"] == 1, distinct
    o, s = _case(ctx, "chain")[5]
    assert sorted(o[0, :2].tolist()) == [10, 11] and sorted(o[1, :2].tolist()) == [2058, 2059] and sorted(o[2, :2].tolist()) == [12, int(o[0, 2])]
    assert s[0] > s[1] > s[2] > s[3]


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("env", SETTINGS)
def test_flagged_pairs_are_decided_exactly(ctx, name, env):
    from glia_amd import hmt
    _, d_lab, d_pb, tree, seq, cpu = _case(ctx, name)
    before = hmt.Context.internal_errors()
    got = _order(ctx, d_lab, d_pb, **env)
    assert _same(got, tree), ("against the tree kernel", name, env)
    assert _same(got, seq), ("against the one-at-a-time window kernel", name, env)
    assert _same(got, cpu), ("against the oracle", name, env)
    assert hmt.Context.internal_errors() == before == 0
