"""-m gpu: the merge loops at 13 824 to 32 768 regions against the REFERENCE'S OWN engine.

tests/golden/headline/reference_<case>.npz hold the orders and saliencies that oracle/_ref/ref_engine (TBoundaryTable / TRegionMap /
genMergeOrderGreedy compiled in place) gave for each volume, recorded by tests/golden/gen_reference_orders.py together with the proof
that the oracle gives the same arrays.  Before this file, an independent answer stopped at 4 096 regions (pb-mean), 1 331 (pb-median), 512
(pre_merge) and about 300 (type 3, masks); beyond that the queue tests compare the kernels with each other, which a mistake in shared code
(edge table, contraction, record layout, tie rule) passes.  Here every linkage, and every queue of the pb-mean loop on its own, is
compared with the recorded reference byte for byte -- the volumes are Q8, so there is no tolerance:

  pb512              512^3, S = 16 (32 768 regions)   pb-mean; also MINCAP=1, the sequential window queue, the tournament tree
  median256s8        256^3, S = 8  (32 768 regions)   pb-median; also MINCAP=1 (every array grows mid-run)
  median192s8_upd    192^3, S = 8  (13 824 regions)   pb-median on a region map with points (the reference run with updateRegion)
  premerge256s8      256^3, S = 8  (32 768 regions)   pre_merge, two size thresholds and the mean-pb rule; also MINCAP=1
  premerge192s8_one  192^3, S = 8  (13 824 regions)   pre_merge, one size threshold
  minsize192s8       192^3, S = 8  (13 824 regions)   median x min-size (type 3): the ORACLE's answer, the reference has no caller of it
  pb_masked192s8     192^3, S = 8, masked             pb-mean (all three queues) and pb-median

The volume is made on the device (glia_hmt_synth), the mask as the generator made it; their SHA-1 must be the fixture's, and a missing
fixture fails."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_reference_orders as G                                                     # noqa: E402

MINCAP, SEQUENTIAL, TREE = dict(GLIA_HMT_MINCAP=1), dict(GLIA_HMT_PB_BATCH=0), dict(GLIA_HMT_PB_WINDOW=0)
# (case, run) -> option sets beyond the defaults
EXTRA = {("pb512", "type2"): [MINCAP, SEQUENTIAL, TREE], ("premerge256s8", "pre_merge"): [MINCAP], ("median256s8", "type1"): [MINCAP],
         ("pb_masked192s8", "type2"): [SEQUENTIAL, TREE]}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("case", sorted(G.CASES))
def test_device_order_is_the_references(ctx, case):
    import torch
    from glia_amd import hmt
    p = G.CASES[case]
    path = G.fixture_path(case)
    assert os.path.exists(path), "%s is missing (python tests/golden/gen_reference_orders.py %s)" % (path, case)
    g = np.load(path)
    labels, pb = ctx.synth((p["size"],) * 3, p["S"], p["G"])
    assert G.sha(labels.cpu().numpy()) == str(g["labels_sha1"]) and G.sha(pb.cpu().numpy()) == str(g["pb_sha1"])     # the fixture's volume
    d_mask = None
    if p.get("mask"):
        mask = G.mask_for((p["size"],) * 3)
        assert G.sha(mask) == str(g["mask_sha1"])
        d_mask = torch.from_numpy(mask.view(np.int32)).cuda()
    else:
        assert str(g["mask_sha1"]) == ""
    for name, kind, type_ in p["runs"]:
        x0 = g[name + "_x0"]
        want = np.stack([x0, g[name + "_x1"], (int(g[name + "_first_new"]) + np.arange(len(x0))).astype(np.uint32)], axis=1)
        want_sal = g[name + "_sal"]
        assert len(want) > 5000 and G.sha(want) == str(g[name + "_order_sha1"]) and G.sha(want_sal) == str(g[name + "_sal_sha1"])
        for env in [dict()] + EXTRA.get((case, name), []):
            with hmt.options(**env):
                rm = hmt.RegionMap(ctx, labels, pb=pb, mask=d_mask, only_contour=p["only_contour"])
                # contour-only maps do not test the centre voxel against the mask (util/struct.hxx:133-143): the device keeps a row for a
                # supervoxel the mask removed whole (no border, no edge, never merged), the reference's border map has no such key
                spare = len(g["absent_labels"]) if p.get("mask") and p["only_contour"] else 0
                assert int(g["regions"]) <= rm.num_regions <= int(g["regions"]) + spare
                order, sal = rm.pre_merge(p["sizes"], p["rpb"]) if kind == "pre_merge" else rm.merge_order_pb(type=type_)
                rm.close()
            assert order.dtype == want.dtype and sal.dtype == want_sal.dtype
            differ = np.nonzero((order[:min(len(order), len(want))] != want[:min(len(order), len(want))]).any(axis=1))[0]
            assert order.shape == want.shape and len(differ) == 0, (name, env, order.shape, want.shape, differ[:1],
                                                                    order[differ[:1]], want[differ[:1]])
            assert order.tobytes() == want.tobytes() and sal.tobytes() == want_sal.tobytes(), (name, env)
