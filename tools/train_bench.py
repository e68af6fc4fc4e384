"""Times train_forest (glia_hmt_forest_train, glia_amd/csrc/forest_train.hip) on the rows the library's own tools make: synth
volume -> pb-mean merge order -> bc_feat rows (batch route) -> bc_label labels (F1 against shifted truth cubes, tools/bclabel_bench.truth_of).
usage: train_bench.py [--cases 256:8 512:16] [--ntree 255] [--ns 1] [--reps 5] [--warmup 1] [--oob] [--imp] [--rows FILE.npz] [--sklearn]
                      [--out FILE]

Per case (size:S): rows x columns, class counts, then the median of the repetitions' wall-clock seconds (rows on the host in, model on
the host out -- what train_rf spends between reading and writing its files), trees/s, rows x trees/s and the per-phase split of the
median run (device milliseconds from events, glia_hmt_last_forest_train_timing).  There is no reference trainer to compare with: the
reference's classRF is not part of its source tree.  With --sklearn, and only if scikit-learn is importable, a RandomForestClassifier of
the same size on the host's threads is timed once beside it -- another algorithm on another machine part, printed as context only.

--oob / --imp train with the out-of-bag error / the variable importances and add their phases (walk, tally, importance;
glia_hmt_last_forest_oob_timing) and the rate of the importance pass in walks/s -- nominal (out-of-bag rows x columns, what the
definition walks) and made (after the rule that a column a row's path never tests needs no walk).  --rows keeps the first case's rows
in a file, so that runs of two builds of the library (GLIA_HMT_LIB) train on the same bytes without making them twice."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from bclabel_bench import truth_of
from glia_amd import hmt

PHASES = ("upload", "bootstrap", "prepare", "gather", "sort", "scan", "split", "partition", "download")


def rows_and_labels(ctx, size, S):
    lab, pb = ctx.synth((size,) * 3, S, 8 * S)
    cfg = hmt.make_config(pb, rb=[(pb, 8, 0.0, 1.0)], thresholds=(0.2, 0.5, 0.8))
    rm = hmt.RegionMap(ctx, lab, pb=pb, only_contour=False, cfg=cfg)
    order, _ = rm.merge_order_pb(type=2)
    X = rm.bc_feat_batch(order)
    y = rm.bc_label(truth_of(lab, 5 * S // 2), order, metric="f1")
    return X, np.asarray(y, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["256:8", "512:16"])
    ap.add_argument("--ntree", type=int, default=255)
    ap.add_argument("--ns", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--oob", action="store_true")
    ap.add_argument("--imp", action="store_true")
    ap.add_argument("--rows", default=None)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = hmt.Context(0)
    say("train_forest on %s: %d trees, nodesize %d, defaults otherwise (mtry floor(sqrt(D)), sample ratio 0.7, balanced); median of %d runs"
        % (torch.cuda.get_device_name(0), args.ntree, args.ns, args.reps))
    say("no reference trainer exists to compare with (classRF is not in the reference's source tree); nothing here is a speed-up over anything")
    for case in args.cases:
        size, S = (int(v) for v in case.split(":"))
        if args.rows and os.path.exists(args.rows):
            with np.load(args.rows) as z:
                X, y = z["X"], z["y"]
        else:
            X, y = rows_and_labels(ctx, size, S)
            if args.rows:
                np.savez(args.rows, X=X, y=y)
        hmt.Context.release_cached_memory()
        torch.cuda.empty_cache()
        say("synth %d^3 at S = %d: %d rows x %d columns, labels %s" % (size, S, X.shape[0], X.shape[1],
                                                                      ", ".join("%d: %d" % (v, (y == v).sum()) for v in sorted(set(y.tolist())))))
        runs = []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            extra = dict(oob=args.oob, importance=args.imp) if args.oob or args.imp else {}
            model = hmt.train_forest(ctx, X, y, ntree=args.ntree, nodesize=args.ns, **extra)
            dt = time.perf_counter() - t0
            if i >= args.warmup:
                runs.append((dt, hmt.last_forest_train_timing(ctx), model.sizes(), hmt.last_forest_oob_timing(ctx) if extra else None,
                             model.oob() if extra else None))
            model.close()
        runs.sort(key=lambda r: r[0])
        dt, tm, sz, otm, oob = runs[len(runs) // 2]
        say("  median %.3f s (min %.3f, max %.3f)   %.1f trees/s   %.3g rows x trees/s   [%s]"
            % (dt, runs[0][0], runs[-1][0], args.ntree / dt, X.shape[0] * args.ntree / dt, " ".join("%.3f" % r[0] for r in runs)))
        say("  %d trees in flight, %d batches, %d levels, %d launches, %d nodes in all (largest tree %d), %.0f MiB of device memory planned"
            % (tm["trees_in_flight"], tm["batches"], tm["levels"], tm["launches"], tm["nodes"], sz["nrnodes"], tm["device_bytes"] / 2 ** 20))
        say("  phases of the median run, device ms: " + "  ".join("%s %.1f" % (k, tm["ms_" + k]) for k in PHASES)
            + "   (call, wall clock: %.1f)" % tm["ms_total"])
        if otm:
            say("  out-of-bag passes of the median run, device ms: walk %.1f  tally %.1f  importance %.1f   (%d out-of-bag rows over all trees, "
                "%.0f MiB of the plan)" % (otm["ms_walk"], otm["ms_tally"], otm["ms_importance"], otm["oob_rows"], otm["device_bytes"] / 2 ** 20))
            if args.imp and otm["ms_importance"] > 0:
                say("  importance pass: %.3g walks/s nominal (%d), %.3g walks/s made (%d: %.1f %% of the nominal ones)"
                    % (otm["walks_nominal"] / otm["ms_importance"] * 1e3, otm["walks_nominal"], otm["walks_done"] / otm["ms_importance"] * 1e3,
                       otm["walks_done"], 100.0 * otm["walks_done"] / max(1, otm["walks_nominal"])))
            if "errtr" in oob:
                say("  out-of-bag error of the forest: %.4f (per class: %s)" % (oob["errtr"][-1, 0], " ".join("%.4f" % v for v in oob["errtr"][-1, 1:])))
            if "importance" in oob:
                top = np.argsort(-oob["importance"][:, -2])[:5]
                say("  columns of the largest mean decrease in accuracy: " + "  ".join("%d: %.4f" % (v, oob["importance"][v, -2]) for v in top))
        if args.sklearn:
            try:
                from sklearn.ensemble import RandomForestClassifier
            except ImportError:
                say("  scikit-learn is not importable here: no host time beside it")
            else:
                t0 = time.perf_counter()
                RandomForestClassifier(n_estimators=args.ntree, min_samples_leaf=args.ns, max_samples=0.7, class_weight="balanced",
                                       n_jobs=int(os.environ.get("OMP_NUM_THREADS", "16"))).fit(X, y)
                import sklearn
                say("  context only: scikit-learn %s RandomForestClassifier, same size, host threads: %.3f s (another algorithm; not a baseline)"
                    % (sklearn.__version__, time.perf_counter() - t0))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
