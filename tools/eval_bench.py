"""Times the counting pass of glia_hmt_label_overlap (label_overlap.hip), with and without a mask, on the same two volumes
in the same process, the calls alternating.  (profiles/eval_bench.txt is a run of an earlier version, which also timed the counting
kernel glia_hmt_bc_label had then; bc_label counts with label_overlap now.)
usage: eval_bench.py [--sizes 512 1024] [--reps 7] [--warmup 2] [--out FILE]

Inputs (device synth, S = 16 labels; truth cells of side 40, tools/bclabel_bench.truth_of): label_overlap without a mask (8 B/voxel)
and with an all-ones mask (12 B/voxel).  The times are device milliseconds of the counting kernel alone,
glia_hmt_last_eval_timing().ms_count.  Reported per size: median and minimum of the repetitions, GB/s of the algorithmic bytes, their
share of the 8 TB/s HBM peak, the entries of the table and the passes repeated because the global table was too small."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from bclabel_bench import truth_of
from glia_amd import hmt

HBM_PEAK = 8.0e12      # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = hmt.Context(0)
    say("label_overlap on %s; synth S = 16 labels against truth cells of side 40" % torch.cuda.get_device_name(0))
    for size in args.sizes:
        n_vox = size ** 3
        lab, _ = ctx.synth((size,) * 3, 16, 128)
        truth = truth_of(lab, 40)
        ones = torch.ones_like(lab)
        torch.cuda.synchronize()

        def run(which):
            ctx.label_overlap(lab, truth, mask=ones if which == "label_overlap+mask" else None)
            t = ctx.last_eval_timing()
            return t["ms_count"], t["entries"], t["repeats"]

        names = ("label_overlap", "label_overlap+mask")
        for _ in range(args.warmup):
            for w in names:
                run(w)
        ms = {w: [] for w in names}
        info = {}
        for _ in range(args.reps):
            for w in names:                                    # alternating
                t, entries, repeats = run(w)
                ms[w].append(t)
                info[w] = (entries, repeats)
        say("%d^3 (%d voxels):" % (size, n_vox))
        for w in names:
            nbytes = (12.0 if w.endswith("mask") else 8.0) * n_vox
            med = statistics.median(ms[w])
            say("  %-18s median %.3f ms, min %.3f ms, %.0f GB/s of %d B/voxel = %.1f %% of 8 TB/s; %d entries, %d repeated passes   [%s]"
                % (w, med, min(ms[w]), nbytes / (med * 1e6), nbytes / n_vox, 100.0 * nbytes / HBM_PEAK / (med * 1e-3), info[w][0], info[w][1],
                   " ".join("%.3f" % v for v in ms[w])))
        del lab, truth, ones
        hmt.Context.release_cached_memory()
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
