"""Times glia_hmt_label_components on both routes (GLIA_HMT_CC = tiled | global), HIP events around each call, the routes
alternating.  usage: cc_bench.py [--size 512] [--reps 7] [--warmup 2] [--out FILE]

Inputs (device synth, S = 16): the labels in identity mode (many small components), the same labels modulo 5 (many pieces per
label), pb > 0.5 in binary mode (few huge components: the longest root walks).  Reported per input and route: ms (median, min) and
the fraction of the HBM bound of the 8 algorithmic bytes per voxel (4 read, 4 written) at 8 TB/s peak; then who won each alternating
pair.  Where scipy is present: scipy.ndimage.label on the host for the binary input at 256^3, for orientation."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from glia_amd import hmt

HBM_PEAK = 8.0e12      # bytes / s
ROUTES = ("tiled", "global")


def inputs(ctx, size):
    labels, pb = ctx.synth((size,) * 3, 16, 128)
    return [("synth S=16, identity", labels, "identity"),
            ("synth S=16 modulo 5, identity", (labels % 5 + 1).contiguous(), "identity"),
            ("pb > 0.5, binary", (pb > 0.5).to(torch.int32).contiguous(), "binary")]


def timed(ctx, vol, mode, route):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with hmt.options(GLIA_HMT_CC=route):
        a.record()
        out, n = ctx.label_components(vol, mode=mode)
        b.record()
    b.synchronize()
    return a.elapsed_time(b), out, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # the library's kernels run on the stream the events are recorded on
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = hmt.Context(0, stream=stream.cuda_stream)
    n_vox = args.size ** 3
    bound_ms = 8.0 * n_vox / HBM_PEAK * 1e3
    say("label_components %d^3 on %s: 8 B/voxel at %.0f TB/s = %.3f ms" % (args.size, torch.cuda.get_device_name(0), HBM_PEAK / 1e12, bound_ms))
    all_won = True
    for name, vol, mode in inputs(ctx, args.size):
        outs = {}
        for _ in range(args.warmup):
            for r in ROUTES:
                _, outs[r], n = timed(ctx, vol, mode, r)
        same = torch.equal(outs["tiled"], outs["global"])
        ms = {r: [] for r in ROUTES}
        for _ in range(args.reps):
            for r in ROUTES:                                   # alternating pairs
                ms[r].append(timed(ctx, vol, mode, r)[0])
        wins = sum(t < g for t, g in zip(ms["tiled"], ms["global"]))
        all_won = all_won and wins == args.reps
        say("%s: %d components, routes byte-identical: %s" % (name, n, same))
        for r in ROUTES:
            med = statistics.median(ms[r])
            say("  %-6s median %.3f ms, min %.3f ms, %.1f %% of the 8 B/voxel bound   [%s]"
                % (r, med, min(ms[r]), 100.0 * bound_ms / med, " ".join("%.3f" % v for v in ms[r])))
        say("  tiled faster in %d of %d alternating pairs" % (wins, args.reps))
        del outs
    say("tiled beats global on all inputs in every pair: %s" % all_won)
    try:
        import scipy.ndimage as ndi
        small = (ctx.synth((256,) * 3, 16, 128)[1] > 0.5).cpu().numpy()
        t0 = time.time()
        _, n = ndi.label(small)
        say("for orientation, host: scipy.ndimage.label 256^3 binary (%d components): %.0f ms" % (n, (time.time() - t0) * 1e3))
    except ImportError:
        say("scipy is absent: no host figure")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
