"""Batch MLP prediction: rows/s of glia_hmt_mlp_predict_device on device rows of 104 columns under hidden layers of
10 and 10 units (the reference's defaults) and of 64 and 64, logits and probabilities written; one warm-up, the median of 7; the share
of 8 TB/s at 8 * dim bytes per row.  For scale only, glia_hmt_mlp_predict_host on one thread.  One JSON line per stage.
    python tools/mlp_bench.py [--rows 2097152] [--dim 104] [--host-rows 20000] [--out profiles/mlp_bench.txt]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from glia_amd import hmt

HBM_BYTES_PER_S = 8e12


def stage(ctx, a, n1, n2, out):
    rng = np.random.default_rng(n1)
    D = a.dim + 1
    w = rng.standard_normal(D * n1 + (n1 + 1) * n2 + n2 + 1) * 0.1
    mn, mx = np.zeros(a.dim), np.ones(a.dim)
    clf = hmt.MLP.from_arrays(ctx, w, n1, n2, mn, mx)
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = torch.rand((a.rows, a.dim), dtype=torch.float64, device="cuda", generator=g)
    pred = torch.empty(a.rows, dtype=torch.float64, device="cuda")
    logit = torch.empty(a.rows, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ms = []
    for _ in range(8):
        t = time.perf_counter()
        hmt._check(hmt.lib().glia_hmt_mlp_predict_device(ctx.h, clf.h, C.c_void_p(rows.data_ptr()), C.c_int64(a.rows), C.c_int(a.dim), C.c_int64(a.dim),
                                                         C.c_void_p(pred.data_ptr()), C.c_void_p(logit.data_ptr())))
        ctx.sync()
        ms.append((time.perf_counter() - t) * 1e3)
    med = statistics.median(ms[1:])
    tile, staged = hmt.mlp_tile_rows(a.dim, n1, n2)
    host_rows = rows[:a.host_rows].cpu().numpy()
    t = time.perf_counter()
    hp, hl = clf.predict_host(host_rows, want_logits=True)
    host_s = time.perf_counter() - t
    same = bool((logit[:a.host_rows].cpu().numpy().view(np.uint64) == hl.view(np.uint64)).all())
    rec = dict(stage="mlp_predict_device", rows=a.rows, dim=a.dim, n1=n1, n2=n2, tile_rows=tile, staged=staged, ms_first=ms[0], ms_median=med,
               ms_min=min(ms[1:]), ms_max=max(ms[1:]), rows_per_s=a.rows / (med * 1e-3), share_of_8TBps=a.rows * 8.0 * a.dim / (med * 1e-3) / HBM_BYTES_PER_S,
               mul_add_pairs_per_row=D * n1 + (n1 + 1) * n2 + n2 + 1, host_one_thread_rows_per_s=a.host_rows / host_s,
               logits_equal_host_bits=same, mean_pred=float(pred.mean()))
    line = json.dumps(rec)
    print(line, flush=True)
    out.append(line)
    clf.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 21)
    ap.add_argument("--dim", type=int, default=104)
    ap.add_argument("--host-rows", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = hmt.Context(0)
    out = []
    stage(ctx, a, 10, 10, out)
    stage(ctx, a, 64, 64, out)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
