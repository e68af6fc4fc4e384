"""Times mini-batch training (glia_hmt_mlp_train_batches / glia_hmt_sshmt_train_batches, glia_amd/csrc/mlp_batch.hip) on the
rows tools/mlp_train_bench.py uses: 32 767 rows x 104 columns at 256:8, rescaled by their own min/max table, 10 + 10 units, Adam.
usage: minibatch_bench.py [--case 256:8] [--batches 64 256 4096] [--epochs 3] [--pairs 5] [--full-iters 500] [--paths 1] [--out FILE]

Per batch size B an iteration is one epoch of batches (--te 1).  The stream route (the batches of an epoch back to back on the stream,
the update on the device, one wait per epoch) and the step route (GLIA_HMT_BATCH=step: one batch per evaluation, the gradient read
back, the update on the host) alternate in one process; reported are the medians over the pairs of the wall clock per epoch of the
mini-batch steps alone (glia_hmt_batch_timing.ms_wall / steps: plan, upload, kernels, waits), the stream route's own split (plan built
on the host, plan upload, device time between events) and, as the scale, one full-batch iteration of train_mlp on the same rows in the
same process, measured as tools/mlp_train_bench.py measures it (profiles/mlp_train_bench.txt): the wall clock of a call of
--full-iters fixed-step iterations less the rows' upload, over the iterations, so that what a call costs once -- the scans and the
rescaling of the rows, allocations, the sigma evaluations -- is spread as thinly as there.  --paths 1 repeats everything with the merge-path term on: the order the rows came from is the unlabelled block, with
batches of B paths as well.  Both routes must return the same bytes; the tool asserts it."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from glia_amd import hmt
from train_bench import truth_of


def rows_labels_order(ctx, size, S):
    """train_bench.rows_and_labels, and the merge order the rows belong to (row k = merge k): the unlabelled block of --paths 1"""
    lab, pb = ctx.synth((size,) * 3, S, 8 * S)
    cfg = hmt.make_config(pb, rb=[(pb, 8, 0.0, 1.0)], thresholds=(0.2, 0.5, 0.8))
    rm = hmt.RegionMap(ctx, lab, pb=pb, only_contour=False, cfg=cfg)
    order, _ = rm.merge_order_pb(type=2)
    X = rm.bc_feat_batch(order)
    y = rm.bc_label(truth_of(lab, 5 * S // 2), order, metric="f1")
    return X, np.asarray(y, np.int32), np.asarray(order, np.uint32)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="256:8")
    ap.add_argument("--batches", nargs="+", type=int, default=[64, 256, 4096])
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--full-iters", type=int, default=500)
    ap.add_argument("--paths", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = hmt.Context(0)
    size, S = (int(v) for v in args.case.split(":"))
    X, y, order = rows_labels_order(ctx, size, S)
    mm = hmt.rows_minmax([X])
    hmt.Context.release_cached_memory()
    torch.cuda.empty_cache()
    n = int(((y == 1) | (y == -1)).sum())
    say("mini-batch training on %s: synth %d^3 at S = %d, %d rows x %d columns (%d labelled), 10 + 10 units, Adam, fixed step; %d epochs per call, "
        "median of %d alternating pairs after one warm-up pair" % (torch.cuda.get_device_name(0), size, S, X.shape[0], X.shape[1], n, args.epochs, args.pairs))
    base = dict(ws=1.0, wr=1e-4, sigma_s=0.5, step=1e-3, n_sigma_updates=1, optimizer=2, minmax=mm)

    def full_iteration(with_paths):
        runs = []
        for i in range(1 + args.pairs):
            t0 = time.perf_counter()
            if with_paths:
                m = hmt.train_sshmt(ctx, X, y, [(X, order)], 10, 10, max_iterations=args.full_iters, wu=0.5, sigma_u=0.7, **base)
            else:
                m = hmt.train_mlp(ctx, X, y, 10, 10, max_iterations=args.full_iters, **base)
            dt = time.perf_counter() - t0
            if with_paths:
                tu = hmt.last_sshmt_train_timing(ctx)
                up, its = tu["sup"]["ms_upload"] + tu["ms_u_upload"], tu["sup"]["iterations"]
            else:
                tm = hmt.last_mlp_train_timing(ctx)
                up, its = tm["ms_upload"], tm["iterations"]
            assert its == args.full_iters and not m.stopped_nonfinite
            m.close()
            if i:
                runs.append((dt * 1e3 - up) / args.full_iters)
        return median(runs)

    for with_paths in ([False, True] if args.paths else [False]):
        say("---- %s ----" % ("with the merge-path term (wu 0.5, paths of 2 to 3 merges, batches of B paths too)" if with_paths else "supervised term alone"))
        full = full_iteration(with_paths)
        say("one full-batch iteration (all %d rows, update on the host): %.3f ms wall clock (calls of %d iterations less the rows' upload, median of %d after "
            "one warm-up%s)" % (n, full, args.full_iters, args.pairs, "" if with_paths else "; profiles/mlp_train_bench.txt has 0.453 ms for the same rows, units and optimiser"))
        for B in args.batches:
            res = {"stream": [], "step": []}
            split = []
            models = {}
            for i in range(1 + args.pairs):
                for route in ("stream", "step"):
                    with hmt.options(GLIA_HMT_BATCH=route):
                        if with_paths:
                            m = hmt.train_sshmt_batches(ctx, X, y, [(X, order)], 10, 10, batch=dict(seed=1), sup_batch_size=B, uns_batch_size=B,
                                                        max_iterations=args.epochs, wu=0.5, sigma_u=0.7, **base)
                        else:
                            m = hmt.train_mlp_batches(ctx, X, y, 10, 10, batch=dict(seed=1), sup_batch_size=B, max_iterations=args.epochs, **base)
                    tm = hmt.last_batch_timing(ctx)
                    assert tm["steps"] == args.epochs and not m.stopped_nonfinite
                    models[route] = m.weights().tobytes()
                    m.close()
                    if i:
                        res[route].append(tm["ms_wall"] / tm["steps"])
                        if route == "stream":
                            split.append((tm["ms_plan"] / tm["steps"], tm["ms_upload"] / tm["steps"], tm["ms_steps"] / tm["steps"], tm["batches"] / tm["steps"],
                                          tm["syncs"] / tm["steps"], tm["plan_bytes"]))
                assert models["stream"] == models["step"], "the routes differ"
            a, b = median(res["stream"]), median(res["step"])
            sp = sorted(split, key=lambda r: r[2])[len(split) // 2]
            say("B = %-5d %6.1f batches per epoch: stream %.3f ms per epoch (min %.3f, max %.3f; %.4f ms per batch), step %.3f ms per epoch (min %.3f, max %.3f; "
                "%.4f ms per batch): step / stream = %.2f; epoch / full-batch iteration: stream %.2f, step %.2f"
                % (B, sp[3], a, min(res["stream"]), max(res["stream"]), a / sp[3], b, min(res["step"]), max(res["step"]), b / sp[3], b / a, a / full, b / full))
            say("          stream route per epoch: plan built on the host %.3f ms, plan upload %.3f ms, device time %.3f ms (%.4f ms per batch), waits %.0f, "
                "plan %.0f KiB" % (sp[0], sp[1], sp[2], sp[2] / sp[3], sp[4], sp[5] / 1024.0))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
