"""Times the merge-path term of train_sshmt (glia_hmt_sshmt_train, glia_amd/csrc/sshmt_train.hip) with the term alone on
(wu 1, wr 1e-4, no labelled rows), 10 + 10 units, 104 columns, paths of (3, 2):
  synth   the rows and the pb-mean merge order of a synth volume (256:8 -> 32 767 rows), as tools/train_bench.py makes them;
  large   262 143 rows: the synth rows drawn with replacement and jittered, under the merge order of a random balanced tree.
usage: sshmt_bench.py [--case 256:8] [--large 262143] [--units 10] [--iters 200] [--reps 5] [--warmup 1] [--host-iters 1] [--out FILE]

Per case: the median over the repetitions of the call's wall clock per optimiser iteration (the call prepares rows, paths and incidence
lists on the host once, which is in that figure), and from the median run the device time per evaluation of every stage (events around
each): weights up, forward of all rows, paths, gather, chunk kernel, fold, read-back.  Forward, paths, fold and read-back run in every
evaluation; gather and the chunk kernel only in those that want the gradient.  The host definition (train_sshmt_host, one core) is
timed once: a scale, not a competitor -- the reference trainer cannot be built here, so nothing in this file is a speed-up over it."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from glia_amd import hmt


def synth_rows_and_order(ctx, size, S):
    lab, pb = ctx.synth((size,) * 3, S, 8 * S)
    cfg = hmt.make_config(pb, rb=[(pb, 8, 0.0, 1.0)], thresholds=(0.2, 0.5, 0.8))
    rm = hmt.RegionMap(ctx, lab, pb=pb, only_contour=False, cfg=cfg)
    order, _ = rm.merge_order_pb(type=2)
    X = rm.bc_feat_batch(order)
    rm.close()
    return X, order


def random_tree_order(n_merges, seed):
    """the order of a random binary tree over n_merges + 1 leaves, merged level by level (odd ones wait for the next level)"""
    rng = np.random.default_rng(seed)
    live = rng.permutation(n_merges + 1).astype(np.int64)
    nxt, out = n_merges + 1, []
    while len(live) > 1:
        k = len(live) // 2
        created = np.arange(nxt, nxt + k)
        out.append(np.stack([live[0:2 * k:2], live[1:2 * k:2], created], axis=1))
        live = rng.permutation(np.concatenate([created, live[2 * k:]]))
        nxt += k
    return np.concatenate(out).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="256:8")
    ap.add_argument("--large", type=int, default=262143)
    ap.add_argument("--units", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = hmt.Context(0)
    size, S = (int(v) for v in args.case.split(":"))
    X, order = synth_rows_and_order(ctx, size, S)
    hmt.Context.release_cached_memory()
    torch.cuda.empty_cache()
    cases = [("synth %d^3 at S = %d" % (size, S), X, order)]
    if args.large > 0:
        rng = np.random.default_rng(1)
        XL = X[rng.integers(0, len(X), args.large)] * (1.0 + 0.01 * rng.standard_normal((args.large, 1)))
        cases.append(("large", XL, random_tree_order(args.large, 2)))
    say("train_sshmt, the merge-path term alone, on %s: %d + %d units, paths of (3, 2), %d iterations in one round, fixed step; median of %d runs "
        "after %d warm-up" % (torch.cuda.get_device_name(0), args.units, args.units, args.iters, args.reps, args.warmup))
    say("the reference trainer cannot be built here: nothing below is a speed-up over it; host exp pinned: %s" % (ctx.libm_exp() != 0))
    base = dict(wu=1.0, wr=1e-4, sigma_u=0.5, step=1e-3, n_sigma_updates=1)
    n = args.units
    for name, Xc, oc in cases:
        mm = hmt.rows_minmax([Xc])
        runs = []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            m = hmt.train_sshmt(ctx, None, None, [(Xc, oc)], n, n, minmax=mm, max_iterations=args.iters, **base)
            dt = time.perf_counter() - t0
            tm = hmt.last_sshmt_train_timing(ctx)
            assert not m.stopped_nonfinite and tm["sup"]["iterations"] == args.iters
            P = m.n_paths
            m.close()
            if i >= args.warmup:
                runs.append((dt, tm))
        runs.sort(key=lambda r: r[0])
        dt, tm = runs[len(runs) // 2]
        ev, gev = tm["u_evals"], tm["u_grad_evals"]
        stages = ("weights", "forward", "paths", "gather", "chunk", "fold", "readback")
        per = {k: tm["ms_u_" + k] / (gev if k in ("gather", "chunk") else ev) for k in stages}
        say("%s: %d rows x %d columns, %d paths; call %.3f s (min %.3f, max %.3f): %.3f ms per iteration wall clock, the host's once-per-call preparation "
            "(validation, paths, incidence lists, rescaling) included, the upload (%.1f ms) not; device memory %.0f MiB"
            % (name, Xc.shape[0], Xc.shape[1], P, dt, runs[0][0], runs[-1][0], (dt * 1e3 - tm["ms_u_upload"]) / args.iters, tm["ms_u_upload"],
               tm["u_device_bytes"] / 2 ** 20))
        say("      device ms per evaluation (%d evaluations, %d with the gradient): " % (ev, gev) + "  ".join("%s %.3f" % (k, per[k]) for k in stages)
            + "   an evaluation with the gradient %.3f, without %.3f" % (sum(per.values()), sum(per[k] for k in stages if k not in ("gather", "chunk"))))
        if args.host_iters > 0:
            t0 = time.perf_counter()
            m = hmt.train_sshmt_host(None, None, [(Xc, oc)], n, n, minmax=mm, max_iterations=args.host_iters, **base)
            dt = time.perf_counter() - t0
            m.close()
            say("      host definition on one core (scale only): %.0f ms for %d iteration(s), the final evaluation and two evaluations of L_U alone"
                % (dt * 1e3, args.host_iters))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
