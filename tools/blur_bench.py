"""Times glia_hmt_blur_image on both routes (GLIA_HMT_BLUR = march | passes), HIP events around each call, the routes alternating.
usage: blur_bench.py [--size 512] [--reps 7] [--warmup 2] [--out FILE]

Input: the device synth's pb volume (float32).  Cases: sigma 1 with width 3 (radius 3), sigma 2 with width 8 (radius 5), and the
slice-wise mode (sigma 1, width 3, z left alone).  Reported per case and route: ms (median, min) and the fraction of the HBM bound of
the 8 algorithmic bytes per voxel (4 read, 4 written) at 8 TB/s peak; who won each alternating pair; whether the two routes returned
the same bytes.  Where scipy is present: three scipy.ndimage.correlate1d passes on the host at 256^3, for orientation."""
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
ROUTES = ("march", "passes")
CASES = [("sigma 1, width 3", 1.0, 3, -1), ("sigma 2, width 8", 2.0, 8, -1), ("sigma 1, width 3, slice-wise (z left alone)", 1.0, 3, 2)]


def timed(ctx, vol, sigma, width, skip, route):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with hmt.options(GLIA_HMT_BLUR=route):
        a.record()
        out = ctx.blur_image(vol, sigma, width, dim=skip)
        b.record()
        used = ctx.last_blur_timing()[1]
    b.synchronize()
    assert used == route, (used, route)
    return a.elapsed_time(b), out


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
    say("blur_image %d^3 float32 on %s: 8 B/voxel at %.0f TB/s = %.3f ms" % (args.size, torch.cuda.get_device_name(0), HBM_PEAK / 1e12, bound_ms))
    pb = ctx.synth((args.size,) * 3, 16, 128)[1]
    first_won = None
    for name, sigma, width, skip in CASES:
        outs = {}
        for _ in range(args.warmup):
            for r in ROUTES:
                _, outs[r] = timed(ctx, pb, sigma, width, skip, r)
        same = torch.equal(outs["march"].view(torch.int32), outs["passes"].view(torch.int32))
        del outs
        ms = {r: [] for r in ROUTES}
        for _ in range(args.reps):
            for r in ROUTES:                                   # alternating pairs
                ms[r].append(timed(ctx, pb, sigma, width, skip, r)[0])
        wins = sum(m < p for m, p in zip(ms["march"], ms["passes"]))
        if first_won is None:
            first_won = wins == args.reps
        say("%s (radius %d): routes byte-identical: %s" % (name, hmt.gaussian_kernel(sigma * sigma, width)[1], same))
        for r in ROUTES:
            med = statistics.median(ms[r])
            say("  %-6s median %.3f ms, min %.3f ms, %.1f %% of the 8 B/voxel bound   [%s]"
                % (r, med, min(ms[r]), 100.0 * bound_ms / med, " ".join("%.3f" % v for v in ms[r])))
        say("  march faster in %d of %d alternating pairs" % (wins, args.reps))
    say("march wins every pair for sigma 1, width 3: %s" % first_won)
    try:
        import scipy.ndimage as ndi
        small = ctx.synth((256,) * 3, 16, 128)[1].cpu().numpy()
        c = hmt.gaussian_kernel(1.0, 3)[0]
        full = np.concatenate([c[:0:-1], c])
        t0 = time.time()
        v = small
        for ax in (2, 1, 0):
            v = ndi.correlate1d(v, full, axis=ax, mode="nearest")
        say("for orientation, host: scipy.ndimage.correlate1d x 3 at 256^3, sigma 1, width 3: %.0f ms" % ((time.time() - t0) * 1e3))
    except ImportError:
        say("scipy is absent: no host figure")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
