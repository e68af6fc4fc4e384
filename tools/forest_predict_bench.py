"""Batch forest prediction at the size of the initial-edge case: rows/s of glia_hmt_forest_predict_device for 1.86 M rows of
104 columns under a forest of 255 trees of depth <= 12, and the host times of segment_ccm's tree inference on the pb-mean tree of a
synth volume of 262 144 regions.  One JSON line per stage, printed as soon as it is known (the confidence stage is O(nodes * depth)).
    python tools/forest_predict_bench.py [--rows 1860000] [--dim 104] [--ntree 255] [--depth 12] [--reps 5] [--ccm-size 1024] [--ccm-S 16]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from glia_amd import hmt, synth_forest


def predict_stage(ctx, a):
    forest = synth_forest.synthetic_forest(ntree=a.ntree, max_depth=a.depth)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "model.bin")
        synth_forest.write_model(path, forest)
        clf = hmt.RandomForest(ctx, path)
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = torch.rand((a.rows, a.dim), dtype=torch.float64, device="cuda", generator=g)
    # the columns the synthetic trees split on besides the [0, 1) image statistics: boundary length, area of the smaller region
    rows[:, 6] = 4.0 + 396.0 * rows[:, 6]
    rows[:, 35] = 50.0 + 19950.0 * rows[:, 35]
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps + 1):
        t = time.perf_counter()
        pred = clf.predict(rows)
        ms.append((time.perf_counter() - t) * 1e3)
    best = min(ms[1:])
    nodes = int((forest["nodestatus"] != 0).sum())
    print(json.dumps(dict(stage="predict", rows=a.rows, dim=a.dim, ntree=a.ntree, max_depth=a.depth, forest_nodes=nodes, ms_first=ms[0], ms_best=best,
                          rows_per_s=a.rows / (best * 1e-3), tree_walks_per_s=a.rows * a.ntree / (best * 1e-3), mean_pred=float(pred.mean()),
                          ratio_to_bc_init_score_9p65ms=best / 9.65)), flush=True)
    # a few hundred rows, as pred_rf on a 2D section has
    small = rows[:300].clone()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps + 1):
        t = time.perf_counter()
        clf.predict(small)
        ms.append((time.perf_counter() - t) * 1e3)
    print(json.dumps(dict(stage="predict_small", rows=300, ms_best=min(ms[1:]))), flush=True)


def ccm_stage(ctx, a):
    lab, pb = ctx.synth((a.ccm_size,) * 3, a.ccm_S, 8 * a.ccm_S)
    torch.cuda.synchronize()
    rm = hmt.RegionMap(ctx, lab, pb=pb, only_contour=True)
    order, sal = rm.merge_order_pb(type=2)
    regions = int(rm.num_regions)
    rm.close()
    del lab, pb
    probs = np.random.default_rng(2).random(len(order))
    t = time.perf_counter()
    lab_, par, c0, c1, em, es, Em, Es = hmt.tree_energies(order, probs)
    t_energy = time.perf_counter() - t
    t = time.perf_counter()
    picks = hmt.resolve_tree_ccm(c0, c1, Em, Es)
    t_resolve = time.perf_counter() - t
    depth = np.zeros(len(par), np.int32)
    for i in range(len(par) - 1, -1, -1):
        if par[i] >= 0:
            depth[i] = depth[par[i]] + 1
    print(json.dumps(dict(stage="ccm_tree", regions=regions, merges=int(len(order)), nodes=int(len(par)), max_depth=int(depth.max()),
                          mean_leaf_depth=float(depth[c0 < 0].mean()), energies_s=t_energy, resolve_s=t_resolve, picks=int(len(picks)))), flush=True)
    t = time.perf_counter()
    hmt.tree_ccm_confidence(par, c0, c1, es, Em, Es)
    print(json.dumps(dict(stage="ccm_confidence", nodes=int(len(par)), confidence_s=time.perf_counter() - t)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1860000)
    ap.add_argument("--dim", type=int, default=104)
    ap.add_argument("--ntree", type=int, default=255)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ccm-size", type=int, default=1024)
    ap.add_argument("--ccm-S", type=int, default=16)
    a = ap.parse_args()
    ctx = hmt.Context(0)
    predict_stage(ctx, a)
    if a.ccm_size > 0:
        ccm_stage(ctx, a)


if __name__ == "__main__":
    main()
