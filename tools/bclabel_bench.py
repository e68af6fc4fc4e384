"""bc_label stages at scale: the counting pass (device), the per-node values and the label rules (host), on a synth
volume with a pb-mean order; and the NumPy restatement of tests/test_gpu_bc_label.py at a small size for scale.
    python tools/bclabel_bench.py [--size 1024] [--S 16] [--reps 3] [--ref-size 128]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from glia_amd import hmt


def truth_of(labels, G):
    """a truth volume on the device: G-cubes, shifted per supervoxel so that a supervoxel meets one to a few truth labels"""
    shape = labels.shape
    jit = (labels.to(torch.int64) * 2654435761) % G
    t = None
    for ax, n in enumerate(shape):
        g = torch.arange(n, device=labels.device).view([-1 if i == ax else 1 for i in range(len(shape))])
        c = (g + jit) // G
        t = c if t is None else t * ((n + 2 * G - 1) // G) + c
        del c
    return (t + 1).to(torch.int32).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--S", type=int, default=16)
    ap.add_argument("--G", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-size", type=int, default=128)
    a = ap.parse_args()
    ctx = hmt.Context(0)
    out = {}
    lab, pb = ctx.synth((a.size,) * 3, a.S, 8 * a.S)
    truth = truth_of(lab, a.G)
    torch.cuda.synchronize()
    rm = hmt.RegionMap(ctx, lab, pb=pb)
    order, _ = rm.merge_order_pb(type=2)
    out.update(size=a.size, S=a.S, regions=int(rm.num_regions), merges=int(len(order)))
    for metric, opt in (("f1", 0), ("vi", 0), ("f1", 2)):
        runs = []
        for _ in range(a.reps):
            t = time.perf_counter()
            labels = rm.bc_label(truth, order, metric=metric, opt=opt)
            wall = (time.perf_counter() - t) * 1e3
            s = rm.last_bc_label_timing()
            s["wall_ms"] = wall
            runs.append(s)
        best = min(runs, key=lambda r: r["wall_ms"])
        best["count_GBps_at_8B"] = 8.0 * a.size ** 3 / (best["ms_count"] * 1e6)
        best["merge_labels"] = int((labels == -1).sum())
        out["%s_opt%d" % (metric, opt)] = best
    rm.close()
    # the restatement of the tests, on the CPU, for scale
    import test_gpu_bc_label as T
    from oracle import pyoracle as O
    shape = (a.ref_size,) * 3
    S = max(a.S // 2, 1)
    labels_np, pb_np = O.synth(shape, S, 8 * S)
    tr = T.truth_cells(shape, max(a.G // 2, 2)).astype(np.uint32) + 1
    d_lab = torch.from_numpy(labels_np.view(np.int32)).cuda()
    d_pb = torch.from_numpy(pb_np).cuda()
    rm = hmt.RegionMap(ctx, d_lab, pb=d_pb)
    o, _ = rm.merge_order_pb(type=2)
    t = time.perf_counter()
    want = T.Ref(labels_np, o).labels([tr], metric="f1")
    ref_s = time.perf_counter() - t
    t = time.perf_counter()
    got = rm.bc_label(T._dt(tr), o, metric="f1")
    lib_s = time.perf_counter() - t
    out["restatement"] = dict(size=a.ref_size, S=S, merges=int(len(o)), numpy_s=ref_s, library_s=lib_s, equal=bool(got.tolist() == want))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
