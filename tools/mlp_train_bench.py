"""Times train_mlp (glia_hmt_mlp_train, glia_amd/csrc/mlp_train.hip) on the rows tools/train_bench.py makes: synth volume ->
pb-mean merge order -> bc_feat rows -> bc_label labels (32 767 rows x 104 columns at 256:8), rescaled by their own min/max table.
usage: mlp_train_bench.py [--case 256:8] [--units 10 32] [--iters 500] [--reps 5] [--warmup 1] [--host-iters 2] [--out FILE]

Per hidden size (n + n units) and optimiser (1 vanilla, 2 Adam, 3 momentum; fixed step): the median over the repetitions of the call's
wall-clock time per optimiser iteration (rows on the host in, model on the host out; the upload of the rows is reported separately and
not divided), iterations per second, and from the median run the device time per evaluation of the chunk kernel and of the fold kernel
(events around each), the weights' upload and the read-back of L and the gradient, and the read-back's share of the device time.  The
host definition (train_mlp_host, one core) is timed once per hidden size over --host-iters iterations: a scale, not a competitor -- the
reference trainer cannot be built here, so nothing in this file is a speed-up over it."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from glia_amd import hmt
from train_bench import rows_and_labels

OPT = {1: "vanilla", 2: "Adam", 3: "momentum"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="256:8")
    ap.add_argument("--units", nargs="+", type=int, default=[10, 32])
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = hmt.Context(0)
    size, S = (int(v) for v in args.case.split(":"))
    X, y = rows_and_labels(ctx, size, S)
    mm = hmt.rows_minmax([X])
    hmt.Context.release_cached_memory()
    torch.cuda.empty_cache()
    say("train_mlp on %s: synth %d^3 at S = %d, %d rows x %d columns, labels %s; %d iterations in one round, fixed step; median of %d runs after %d warm-up"
        % (torch.cuda.get_device_name(0), size, S, X.shape[0], X.shape[1], ", ".join("%d: %d" % (v, (y == v).sum()) for v in sorted(set(y.tolist()))),
           args.iters, args.reps, args.warmup))
    say("the reference trainer cannot be built here: nothing below is a speed-up over it; host exp pinned: %s" % (ctx.libm_exp() != 0))
    base = dict(ws=1.0, wr=1e-4, sigma_s=0.5, step=1e-3, n_sigma_updates=1)
    for n in args.units:
        for opt in (1, 2, 3):
            runs = []
            for i in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                m = hmt.train_mlp(ctx, X, y, n, n, minmax=mm, optimizer=opt, max_iterations=args.iters, **base)
                dt = time.perf_counter() - t0
                tm = hmt.last_mlp_train_timing(ctx)
                assert not m.stopped_nonfinite and tm["iterations"] == args.iters
                m.close()
                if i >= args.warmup:
                    runs.append((dt, tm))
            runs.sort(key=lambda r: r[0])
            dt, tm = runs[len(runs) // 2]
            ev, gev = tm["evals"], tm["grad_evals"]
            dev = tm["ms_weights"] + tm["ms_chunk"] + tm["ms_fold"] + tm["ms_readback"]
            it_ms = (dt * 1e3 - tm["ms_upload"]) / args.iters
            say("%2d + %2d units, %-8s  %.3f ms per iteration wall clock (%.1f iterations/s; call %.3f s, min %.3f, max %.3f; rows up %.1f ms once)"
                % (n, n, OPT[opt], it_ms, 1e3 / it_ms, dt, runs[0][0], runs[-1][0], tm["ms_upload"]))
            say("      device ms per evaluation (%d evaluations, %d with the gradient): weights up %.3f  chunk kernel %.3f  fold kernel %.3f  read-back %.3f"
                "   read-back share of device time %.1f %%; host side of an iteration (update, norms, launches) %.3f ms; device memory %.0f MiB"
                % (ev, gev, tm["ms_weights"] / ev, tm["ms_chunk"] / ev, tm["ms_fold"] / ev, tm["ms_readback"] / ev, 100.0 * tm["ms_readback"] / dev,
                   (tm["ms_total"] - tm["ms_upload"] - dev) / args.iters, tm["device_bytes"] / 2 ** 20))
        if args.host_iters > 0:
            t0 = time.perf_counter()
            m = hmt.train_mlp_host(X, y, n, n, minmax=mm, optimizer=1, max_iterations=args.host_iters, **base)
            dt = time.perf_counter() - t0
            m.close()
            say("%2d + %2d units, host definition on one core (scale only): %.1f ms per iteration over %d iterations (+ the final evaluation)"
                % (n, n, dt * 1e3 / (args.host_iters + 1), args.host_iters))
    say("the update runs on the host after the gradient's read-back; an update on the device was not built and not measured")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
