"""Arguments for the exp / sigmoid restatement tests (test_libm_exp.py, test_gpu_libm_exp.py) and the host's own values for them."""
import math

import numpy as np

# arguments on which glibc's FMA and non-FMA builds of exp return different doubles (found by comparing the two restatements)
PROBE = [float.fromhex("0x1.abe9a7aa19388p-1"), float.fromhex("0x1.2993abd96c7dp+4"), float.fromhex("-0x1.31e0da89a5188p-2")]
SPECIAL = [0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.0 ** -54, -2.0 ** -54, 2.0 ** -55, 512.0, -512.0, 709.782712893384, 709.7827128933841,
           1024.0, -1024.0, 1e308, -1e308, math.inf, -math.inf, math.nan]


def inputs(seed=17, n=100_000):
    """n seeded values over [-1100, 1100], [-50, 50] and +-[500, 720], the probe arguments and the special values"""
    rng = np.random.default_rng(seed)
    k = n // 4
    wide = rng.uniform(-1100.0, 1100.0, k)
    mid = rng.uniform(-50.0, 50.0, n - 3 * k)
    hi = rng.uniform(500.0, 720.0, k)
    lo = -rng.uniform(500.0, 720.0, k)
    return np.concatenate([wide, mid, hi, lo, np.array(PROBE), np.array(SPECIAL)])


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:      # math.exp raises where the C function returns +inf
        return math.inf


def host_exp(x):
    return np.array([_exp(float(v)) for v in x], np.float64)


def host_sigmoid(x):
    """1.0 / (1.0 + exp(-h)) as a host program computes it (mlp_model.hpp: mlp_sigmoid)"""
    out = np.empty(len(x), np.float64)
    for i, v in enumerate(x):
        e = _exp(-float(v))
        out[i] = 1.0 / (1.0 + e) if e != math.inf else 0.0
    return out


def same_bits(a, b):
    """bit for bit; NaNs equal each other"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
