"""The small image and the two dense models of test_gpu_bc_mlp.py's part 2 (brute-force author: tests/_loopdef_rows.py)."""
import numpy as np

import _loopdef_rows
import _mlpdef

kSeed = 7          # chosen on the CPU: every region of the image has an area of its own, and both replays keep their gaps (see the tests)


def image(seed=kSeed, shape=(40, 48), n=30):
    """a Voronoi partition of `shape` into n regions (labels 1 .. n) and a Q8 image that is darker inside the regions"""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(0, shape[0], n), rng.uniform(0, shape[1], n)], 1)
    y, x = np.indices(shape)
    d = (y[..., None] - pts[:, 0]) ** 2 + (x[..., None] - pts[:, 1]) ** 2
    lab = (np.argmin(d, axis=2) + 1).astype(np.uint32)
    pb = (rng.integers(0, 256, shape) / 256.0).astype(np.float32)
    return lab, pb


def models(init_rows, dim):
    """10 + 10 with a min/max table, and three 7 + 12 members behind a distributor on x0.b0.mean and x1.area; the table spans the
    initial rows"""
    rng = np.random.default_rng(99)
    mn, mx = init_rows.min(0) - 0.25, init_rows.max(0) + 0.25
    one = dict(weights=rng.standard_normal(_mlpdef.n_weights(dim, 10, 10)) * 0.4, n1=10, n2=10, mn=mn, mx=mx, dist=None)
    d0, d1 = 31, 35
    mn3, mx3 = mn.copy(), mx.copy()
    for d in (d0, d1):
        mid, half = float(np.mean(init_rows[:, d])), float(np.ptp(init_rows[:, d])) + 1.0
        mn3[d], mx3[d] = mid - half, mid + half
    ws = [rng.standard_normal(_mlpdef.n_weights(dim, 7, 12)) * 0.4 for _ in range(3)]
    return {"10+10 minmax": one, "ensemble": dict(weights=ws, n1=7, n2=12, mn=mn3, mx=mx3, dist=(float(d0), float(d1), 0.0))}
