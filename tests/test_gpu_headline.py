"""Regression gates at BASELINE.json's headline sizes: the whole merge order and saliency arrays of the
1024^3 pb-mean loop and of the 512^3 classifier loop are compared with recorded SHA-1 digests, plus the size-independent invariants of
util/struct_merge.hxx:19-31.  The synthetic volume (glia_hmt_synth) and the synthetic forest (seed 1234) are deterministic.

Which digest is whose:
  * PB_512 is the REFERENCE's: oracle/_ref/ref_engine (the reference's own TBoundaryTable / TRegionMap / genMergeOrderGreedy) produced
    the 32 767 merges of the 512^3 volume, the oracle produced the same arrays, and their digests are this pair
    (tests/golden/gen_reference_orders.py, case pb512; tests/test_golden_reference_orders.py).  The [512] gate below also compares the
    device's arrays with the recorded ones element by element.
  * the 256^3 pb-mean and classifier orders (BC_256) are the ORACLE's (tests/golden/gen_headline256.py).
  * PB_1024 stays a digest the GPU produced: by the engine times measured at 4 096 and 32 768 regions (1.5 s, 308 s: about R^2.6) the
    reference's engine would need most of a day for 262 144 regions.  What stands behind it is that the same kernels equal the reference
    at 512^3 and, under every queue, in tests/test_gpu_reference_orders.py.
  * BC_512, BC_1024 and config 5 stay self-recorded: the oracle needed 49 minutes for the 256^3 classifier order and the reference's
    feature classes do not compile without ITK.  Every queue / loop variant has to reproduce them byte for byte."""
import hashlib
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# PB_1024, BC_512: recorded from the GPU with tools/pb_bench.py 1024 16 2 (profiles/r02q_pb_hash.txt) and tools/bc_bench.py 512 16
# (profiles/r03_bc_hash.txt).  PB_512 was recorded the same way and has since been reproduced by the reference's own engine and by the
# oracle (tests/golden/headline/reference_pb512.npz); BC_256 is the digest of the oracle's arrays.
PB_1024 = ("977022085e1a37a4d143841a51ea8834b6f53c59", "7923436b47d4484f1e95962ac87ff409d4f2c617")
PB_512 = ("652c84e7efe781bacc9df8c0a16675ca7e34cf17", "d78663710b1699d331a62c40471ba2d90ffc6515")
BC_512 = ("8e620b69eab2cc31991eaca662446f52ad2231df", "8e30e7ba92d7b89dc09c413260a0841df1cbf886")
BC_256 = ("51b7b5316e0d8fd648ab2b444527633d8eaf65c5", "5eadbd683d6a042f7bf950aa2352ef93bdc12956")
# the classifier loop at 1024^3: the digest of bench.py's `bc_loop` leg, identical in profiles/r03x_bench1024.json, r03y, r03z and the
# driver's BENCH_r03.json (four runs, three builds of the loop)
BC_1024 = ("6d930d8a816d75d194b20c5f4eb068a3bd362f3f", "1915075dc494d7c5b56baea947414d1890c2d8f8")


@pytest.fixture(scope="module")
def ctx():
    from glia_amd import hmt
    return hmt.Context(0)


def _sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def _invariants(order, R, first_new):
    n = len(order)
    assert n == R - 1                                                        # connected mutual-edge graph
    o = order.astype(np.int64)
    assert (o[:, 0] < o[:, 1]).all() and (o[:, 1] < o[:, 2]).all()
    assert (o[:, 2] == first_new + np.arange(n)).all()                       # x2 = maxKey + 1 + i
    assert len(np.unique(np.concatenate([o[:, 0], o[:, 1]]))) == 2 * n       # every region is merged exactly once


@pytest.mark.parametrize("size,expect", [(512, PB_512), (1024, PB_1024)])
def test_pb_mean_order_at_headline_size(ctx, size, expect):
    """BASELINE configs 3/4: 1024^3, S = 16, Q8 pb -- 262 143 merges, the loop bench.py times"""
    from glia_amd import hmt
    labels, pb = ctx.synth((size,) * 3, 16, 128)
    rm = hmt.RegionMap(ctx, labels, pb=pb, only_contour=True)
    R = rm.num_regions
    order, sal = rm.merge_order_pb(type=2)
    rm.close()
    _invariants(order, R, R + 1)                                             # labels are 1..R
    assert (np.diff(sal) <= 1e-12).all()                                     # mean linkage is reducible
    assert (_sha(order), _sha(sal)) == expect
    if size == 512:                                                          # the reference's own engine's arrays, element by element
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "headline", "reference_pb512.npz"))
        assert _sha(labels.cpu().numpy()) == str(g["labels_sha1"]) and _sha(pb.cpu().numpy()) == str(g["pb_sha1"])
        assert int(g["type2_first_new"]) == R + 1 and len(g["type2_x0"]) == len(order)
        assert (order[:, 0] == g["type2_x0"]).all() and (order[:, 1] == g["type2_x1"]).all() and (sal == g["type2_sal"]).all()


@pytest.mark.parametrize("size,expect", [(256, BC_256), (512, BC_512), (1024, BC_1024)])
def test_classifier_order_at_headline_size(ctx, size, expect):
    """the north-star linkage (255-tree forest, D_f = 104) at 512^3: invariants + the recorded digest"""
    from glia_amd import hmt
    from glia_amd.synth_forest import synthetic_forest, write_model
    labels, pb = ctx.synth((size,) * 3, 16, 128)
    cfg = hmt.make_config(pb, rb=[(pb, 8, 0.0, 1.0)])
    clf = _forest(ctx)
    rm = hmt.RegionMap(ctx, labels, pb=pb, cfg=cfg)
    R = rm.num_regions
    order, sal = rm.merge_order_bc(clf)
    rm.close()
    _invariants(order, R, R + 1)
    assert ((sal >= 0.0) & (sal <= 1.0)).all()                               # vote fractions
    assert np.all(np.abs(sal * 255.0 - np.round(sal * 255.0)) < 1e-9)        # k / ntree
    assert (_sha(order), _sha(sal)) == expect


# ---- BASELINE config 5: 2048 x 2048 x 512, RF-scored, label volume -> final segmentation, on one MI355X ----------------------
# recorded by this test's first run on the round-4 library (profiles/r04_config5.txt); the order / saliency digests of the same
# volume were also printed by tools/e2e_bench.py
C5_ORDER, C5_SAL = "15f7edfbc88e5b32aff621cd07c148e4bac66c35", "b4617f3fc80c24543b9b8374e4e30cf3a984ebe6"
C5_SEGMENTS, C5_SIZES_SHA, C5_CHECKSUM = 167593, "515ee46de3020d101d323cec4004bba1b9668850", 10347935045297336445


def _forest(ctx):
    from glia_amd import hmt
    from glia_amd.synth_forest import synthetic_forest, write_model
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "m.bin")
        write_model(path, synthetic_forest(ntree=255, dim=3))
        return hmt.RandomForest(ctx, path)


def test_the_256_cubed_orders_are_the_oracles(ctx):
    """Anchors the digest chain of this file in the ORACLE.  256^3 (S = 16, 4 096 regions) is the largest headline-shaped volume the CPU
    restatement finishes (49 minutes of one core: tests/golden/gen_headline256.py wrote tests/golden/headline/headline256_oracle.npz once).  The device's
    pb-mean order and its classifier order (the 255-tree forest of the gates above) are compared with the oracle's byte for byte, and
    the digest recorded above for the 256^3 classifier run -- same kernels, forest and generator as the 512^3 / 1024^3 ones -- is the
    digest of the ORACLE's arrays."""
    from glia_amd import hmt
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "headline", "headline256_oracle.npz")
    if not os.path.exists(path):
        pytest.skip("tests/golden/headline/headline256_oracle.npz has not been generated (python tests/golden/gen_headline256.py, 49 minutes of CPU)")
    g = np.load(path)
    labels, pb = ctx.synth((256,) * 3, 16, 128)
    assert _sha(labels.cpu().numpy()) == str(g["labels_sha1"]) and _sha(pb.cpu().numpy()) == str(g["pb_sha1"])     # the fixture's volume
    rm = hmt.RegionMap(ctx, labels, pb=pb, only_contour=True)
    order, sal = rm.merge_order_pb(type=2)
    rm.close()
    assert order.shape == g["pb_order"].shape and (order == g["pb_order"]).all() and (sal == g["pb_sal"]).all()
    cfg = hmt.make_config(pb, rb=[(pb, 8, 0.0, 1.0)])
    clf = _forest(ctx)
    rm = hmt.RegionMap(ctx, labels, pb=pb, cfg=cfg)
    order, sal = rm.merge_order_bc(clf)
    rm.close()
    assert order.shape == g["bc_order"].shape and (order == g["bc_order"]).all() and (sal == g["bc_sal"]).all()
    assert (_sha(g["bc_order"]), _sha(g["bc_sal"])) == BC_256


def _position_checksum(torch, lab):
    """sum over voxels of label * (1 + index mod 1000003), in wrapping int64, slab by slab on the device: depends on WHERE every
    label sits, costs one pass"""
    total = 0
    flat = lab.reshape(-1)
    step = 1 << 27
    for a in range(0, flat.numel(), step):
        part = flat[a:a + step].to(torch.int64)
        w = (torch.arange(a, a + part.numel(), device=lab.device, dtype=torch.int64) % 1000003) + 1
        total = (total + int((part * w).sum().item())) & 0xFFFFFFFFFFFFFFFF
    return total


def test_config5_end_to_end(ctx):
    """BASELINE config 5 (2048 x 2048 x 512 voxels, S = 16: 524 288 supervoxels; 255-tree forest, D_f = 104): RAG + statistics ->
    merge_order_bc -> genTreeWithNodePotentials -> resolveTreeGreedy -> genLabelTransform -> transformImage -> relabelImage.
    The oracle cannot reach this size; what is checked is what the domain offers at any size --
      * the merge order: invariants of util/struct_merge.hxx:19-31 (each merge joins two live regions and creates maxKey + 1 + k),
        saliencies are vote fractions k / 255;
      * the tree: 2R - 1 nodes, children before parents; the greedy picks are an antichain that covers every leaf exactly once
        (hmt/tree_greedy.hxx:104-152), the label transform maps every leaf;
      * the final volume: every voxel labelled 1..n, every label used, sizes non-increasing in the label (RelabelComponent),
        voxel conservation: the size of every final segment = the summed sizes of the supervoxels the transform sends there;
        relabelImage is idempotent;
    -- plus recorded SHA-1 digests of the order, the saliencies, the segment sizes and a position-dependent checksum of the final volume."""
    import time
    import torch
    from glia_amd import hmt
    shape, S = (512, 2048, 2048), 16
    labels, pb = ctx.synth(shape, S, 8 * S)
    N = labels.numel()
    cfg = hmt.make_config(pb, rb=[(pb, 8, 0.0, 1.0)])
    clf = _forest(ctx)
    t0 = time.time()
    rm = hmt.RegionMap(ctx, labels, pb=pb, cfg=cfg)
    R = rm.num_regions
    reg = rm.regions()
    order, sal = rm.merge_order_bc(clf)
    t_tree = time.time() - t0
    rm.close()
    assert R == 524288
    _invariants(order, R, R + 1)
    assert ((sal >= 0.0) & (sal <= 1.0)).all() and np.all(np.abs(sal * 255.0 - np.round(sal * 255.0)) < 1e-9)
    lab, par, c0, c1, pot = hmt.tree_potentials(order, sal)
    n_nodes = len(lab)
    assert n_nodes == 2 * R - 1 and par[-1] < 0 and (par[:-1] > np.arange(n_nodes - 1)).all()      # children before parents, root last
    picks = hmt.resolve_tree_greedy(par, c0, c1, pot)
    # every leaf has exactly one picked node among itself and its ancestors (pointer jumping over the parent array)
    cover = np.zeros(n_nodes + 1, np.int64); cover[picks] = 1
    assert cover.sum() == len(picks)
    ptr = np.where(par < 0, n_nodes, par).astype(np.int64); ptr = np.concatenate([ptr, [n_nodes]])
    for _ in range(22):
        cover = cover + cover[ptr]; cover[n_nodes] = 0
        ptr = ptr[ptr]
    leaves = np.nonzero(c0 < 0)[0]
    assert len(leaves) == R and (cover[leaves] == 1).all()
    src, dst = hmt.label_transform(lab, c0, c1, picks, 1)
    assert len(src) == R and (np.sort(src) == np.arange(1, R + 1)).all() and len(np.unique(dst)) == len(picks)
    # supervoxel sizes from the region map, summed per destination
    sizes_sv = np.zeros(R + 1, np.int64); sizes_sv[reg["label"]] = reg["count"]
    assert sizes_sv.sum() == N
    exp_sizes = np.bincount(dst, weights=sizes_sv[src].astype(np.float64)).astype(np.int64)
    exp_sizes = np.sort(exp_sizes[exp_sizes > 0])[::-1]
    ms = hmt.transform_image(ctx, labels, src, dst, fill_missing=True)
    n_seg = hmt.relabel_image(ctx, labels)
    assert n_seg == len(picks)
    sizes = torch.bincount(labels.reshape(-1), minlength=n_seg + 1).cpu().numpy()
    assert sizes[0] == 0 and sizes.sum() == N and (sizes[1:] > 0).all()                   # every voxel labelled, every label used
    assert (np.diff(sizes[1:]) <= 0).all()                                                # by decreasing size
    assert (sizes[1:] == exp_sizes).all()                                                 # voxel conservation through the whole chain
    chk = _position_checksum(torch, labels)
    before = labels.clone()
    assert hmt.relabel_image(ctx, labels) == n_seg and torch.equal(before, labels)        # idempotent
    del before
    got = dict(order=_sha(order), sal=_sha(sal), segments=int(n_seg), sizes=_sha(sizes.astype(np.int64)), checksum=chk)
    print("config 5: %d merges in %.2f s (RAG + merge tree), %d segments, transform kernel %.3f ms; digests %r" % (len(order), t_tree, n_seg, ms, got))
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out):
        with open(os.path.join(out, "config5_digests.txt"), "w") as f:
            f.write(repr(got) + "\n")
    if C5_ORDER is not None:
        assert got == dict(order=C5_ORDER, sal=C5_SAL, segments=C5_SEGMENTS, sizes=C5_SIZES_SHA, checksum=C5_CHECKSUM)
