"""bc_feat for a pb-mean order, both routes in one process: the replay of the order through the classifier loop and the batch route over
the known merge tree (glia_hmt_bc_feat_batch).  Both are warmed up, then timed ALTERNATELY, `--repeats` times each, with the host
clock around the call -- it ends in the device-to-host copy of the rows, so the batch route's host plan is inside its time.  Prints
median and spread of each route, the SHA-1 of each route's rows (equal: the synthetic pb is Q8) and the batch route's stages.

    python tools/bcfeat_bench.py [--repeats 7] [--samples 128:8,256:16]
"""
import argparse
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from glia_amd import hmt  # noqa: E402


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--samples", default="128:8,256:16", help="size:S pairs of the synthetic volumes")
    a = ap.parse_args()
    assert a.repeats >= 1
    ctx = hmt.Context(0)
    for size, S in (tuple(int(v) for v in s.split(":")) for s in a.samples.split(",")):
        lab, pb = ctx.synth((size,) * 3, S, 8 * S)
        rm0 = hmt.RegionMap(ctx, lab, pb=pb, only_contour=True)
        order, _ = rm0.merge_order_pb(type=2)
        rm0.close()
        rm = hmt.RegionMap(ctx, lab, pb=pb, only_contour=False, cfg=hmt.make_config(pb, rb=[(pb, 8, 0.0, 1.0)]))
        routes = {"replay": rm.bc_feat, "batch": rm.bc_feat_batch}
        rows = {k: f(order) for k, f in routes.items()}                      # warm-up of both
        times = {k: [] for k in routes}
        for _ in range(a.repeats):
            for k, f in routes.items():
                t = time.perf_counter()
                rows[k] = f(order)
                times[k].append(time.perf_counter() - t)
        stages = rm.last_bc_feat_timing()                                    # of the last call: the batch route
        n, d = rows["batch"].shape
        med = {}
        for k in routes:
            ts = np.array(times[k])
            med[k] = float(np.median(ts))
            print("bc_feat %d^3 S=%d %-6s: %d rows x %d  median %.4f s  min %.4f  max %.4f  spread %.4f  = %.0f rows/s  sha1 %s" %
                  (size, S, k, n, d, med[k], ts.min(), ts.max(), ts.max() - ts.min(), n / med[k], sha(rows[k])), flush=True)
        print("bc_feat %d^3 S=%d: batch / replay = %.2fx, rows %s; batch stages: plan %.2f ms (host), sets %.2f ms, rows %.2f ms (device), "
              "tree height %d, %d launches, %d path updates" %
              (size, S, med["replay"] / med["batch"], "equal" if sha(rows["replay"]) == sha(rows["batch"]) else "DIFFER", stages["ms_plan"],
               stages["ms_sets"], stages["ms_rows"], stages["height"], stages["launches"], stages["path_updates"]), flush=True)
        rm.close()


if __name__ == "__main__":
    main()
