"""blur_image without a GPU: the coefficient rule and the host definition of the library (glia_hmt_gaussian_kernel,
glia_hmt_blur_image_host) against the NumPy second author (tests/_blurdef.py) bit for bit, both anchored to known answers and to
scipy, every argument error of the device call (answered before the first HIP call: the device pointers below are made-up
addresses), and the stand-alone check program under AddressSanitizer and UBSan."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import _blurdef as D
from glia_amd import hmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cli")
ERR_ARG = -1
TS = sorted(set(t for t, _ in D.RADII) | {0.01, 0.5, 2.25, 16, 256})
# The restatement's largest relative distance to scipy.special.ive(n, t) / covered over TS with max_width 128 measured 2.06e-14 (at
# t = 100; 6.6e-15 at t = 256, <= 1.3e-15 up to t = 64: exp(-t) and a sum that has grown to about e^t each carry their own rounding).
# The bar is 8 x that: other scipy builds' ive is itself only good to a few ulp.
SCIPY_BAR = 8 * 2.06e-14


def test_known_radii_and_covered_masses():
    for (t, w), r in D.RADII.items():
        c, radius, covered = hmt.gaussian_kernel(t, w)
        assert radius == r and len(c) == r + 1, (t, w, radius)
        assert D.kernel(t, w)[1] == r
        if (t, w) in D.COVERED:
            assert abs(covered - D.COVERED[(t, w)]) <= 1e-5, (t, w, covered)


@pytest.mark.parametrize("t", TS)
def test_library_coefficients_equal_the_restatement_bit_for_bit(t):
    for w in sorted({w for tt, w in D.RADII if tt == t} | {3, 32, 128}):
        c, r, cov = hmt.gaussian_kernel(t, w)
        c2, r2, cov2 = D.kernel(t, w)
        assert r == r2 and cov == cov2 and c.tobytes() == c2.tobytes(), (t, w)
        assert 1 <= r <= w


def test_restatement_against_scipy():
    sp = pytest.importorskip("scipy.special", reason="scipy is not installed: no third witness for the Bessel values")
    worst = 0.0
    for t in TS:
        c, r, cov = D.kernel(t, 128)
        ref = sp.ive(np.arange(r + 1), float(t)) / cov
        d = float(np.max(np.abs(c - ref) / ref))
        print("t = %g: radius %d, relative distance to scipy %.3g" % (t, r, d))
        worst = max(worst, d)
    print("largest: %.3g, bar %.3g" % (worst, SCIPY_BAR))
    assert worst <= SCIPY_BAR


SHAPES = [(1, 1, 1), (1, 3, 2), (70, 2, 3), (65, 17, 9), (130, 5), (1, 7)]            # (x, y[, z])
KERNELS = [(1.0, 3), (3.0, 5), (0.1, 32), (4.0, 32)]                                   # (sigma, max_width)


def test_the_kernels_of_the_image_cases_are_what_they_are_meant_to_be():
    assert hmt.gaussian_kernel(9.0, 5)[1] == 5 and hmt.gaussian_kernel(9.0, 5)[2] < 0.99          # cut
    assert hmt.gaussian_kernel(0.1 * 0.1, 32)[1] == 1
    assert hmt.gaussian_kernel(16.0, 32)[1] == D.kernel(16.0, 32)[1] > 5


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["q8", "u8", "u16"])
def test_host_definition_equals_the_restatement_bit_for_bit(shape, kind):
    img = D.inputs(shape[::-1], kind, seed=len(shape) * 100 + shape[0])
    dim = len(shape)
    for (sigma, w), skip in itertools.product(KERNELS, range(-1, dim)):
        got = hmt.blur_image_host(img, sigma, w, dim=skip)
        want = D.blur(img, sigma, w, skip)
        assert got.dtype == img.dtype and got.tobytes() == want.tobytes(), (shape, kind, sigma, w, skip)
    per_axis = [0.7, 2.0, 1.3][:dim]
    for skip in range(-1, dim):
        assert hmt.blur_image_host(img, per_axis, 32, dim=skip).tobytes() == D.blur(img, per_axis, 32, skip).tobytes(), (shape, kind, skip)


def test_impulse_known_answer():
    img = np.zeros((9, 9, 9), np.float32)
    img[4, 4, 4] = 1.0
    c, r, _ = hmt.gaussian_kernel(1.0, 3)
    assert r == 3
    out = hmt.blur_image_host(img, 1.0, 3)
    f32 = np.float32
    for dx, dy, dz in [(2, 0, 1), (0, 0, 0), (-3, 3, -1), (1, -2, 3)]:
        want = f32(c[abs(dz)] * float(f32(c[abs(dy)] * float(f32(c[abs(dx)])))))
        assert out[4 + dz, 4 + dy, 4 + dx] == want, (dx, dy, dz)
    assert out[4, 4, 0] == 0 and out[0, 4, 4] == 0                 # beyond the radius


def test_scipy_is_a_third_witness():
    """three correlate1d(mode="nearest") passes in float64, each rounded to float32: each pass leaves both sides within half a float32
    ulp of nearly the same exact value, so the difference grows by at most 2^-23 max|input| per pass; three passes, plus one for the
    order of the double sums"""
    ndi = pytest.importorskip("scipy.ndimage", reason="scipy is not installed")
    for shape, (sigma, w) in itertools.product([(70, 2, 3), (65, 17, 9), (130, 5)], KERNELS):
        img = D.inputs(shape[::-1], "q8", seed=5)
        c = hmt.gaussian_kernel(sigma * sigma, w)[0]
        full = np.concatenate([c[:0:-1], c])
        v = img
        for ax in range(img.ndim - 1, -1, -1):                     # x first
            v = ndi.correlate1d(v.astype(np.float64), full, axis=ax, mode="nearest").astype(np.float32)
        diff = float(np.max(np.abs(v.astype(np.float64) - hmt.blur_image_host(img, sigma, w).astype(np.float64))))
        bar = 4 * 2.0 ** -23 * float(np.max(np.abs(img)))
        print(shape, sigma, w, "difference to scipy %.3g, bar %.3g" % (diff, bar))
        assert diff <= bar, (shape, sigma, w)


@pytest.mark.parametrize("value", [0.5, 2.0 ** -20, 64.0])
def test_a_constant_power_of_two_stays_within_one_ulp_per_pass(value):
    img = np.full((5, 6, 7), value, np.float32)
    for sigma, w in KERNELS:
        out = hmt.blur_image_host(img, sigma, w)
        ulp = value * 2.0 ** -23
        assert float(np.max(np.abs(out.astype(np.float64) - value))) <= 3 * ulp, (sigma, w)


def test_integer_results_stay_in_range_and_are_truncated():
    # a hand-made case: along a line of 8-bit pixels 7 7 7 10 10 10 10 (y and z extents 1), kernel (t = 1, width 3), the pixel at
    # x = 2 gets c1 * 3 + c2 * 3 + c3 * 3 more than 7
    c, r, _ = hmt.gaussian_kernel(1.0, 3)
    line = np.array([[7, 7, 7, 10, 10, 10, 10]], np.uint8)
    exact = 7.0 + 3.0 * (c[1] + c[2] + c[3])
    assert 7.75 < exact < 8.0                                       # 7.79...: rounding would give 8
    out = hmt.blur_image_host(line, 1.0, 3, dim=1)                  # y left alone: a 1D blur
    assert out[0, 2] == 7 and out.dtype == np.uint8
    # x.75 exactly: 0.75 = 3 / 4 cannot come from these kernels, so the cast is also checked on its own against the restatement
    v = np.array([7.75, 255.75, 300.0, -0.75, 65535.75, 0.999], np.float32)
    assert D.to_pixels(v, np.uint8).tolist() == [7, 255, 255, 0, 255, 0]
    assert D.to_pixels(v, np.uint16).tolist() == [7, 255, 300, 0, 65535, 0]
    for kind in ("u8", "u16"):
        img = D.inputs((9, 17, 65), kind, seed=2)
        for sigma, w in KERNELS:
            out = hmt.blur_image_host(img, sigma, w)
            assert out.dtype == img.dtype and out.min() >= img.min() and out.max() <= img.max()
    sat = np.full((3, 4, 5), 65535, np.uint16)
    assert (hmt.blur_image_host(sat, 2.0, 8) >= 65534).all()       # a saturated image stays at the top within the casts' one unit
    assert (hmt.blur_image_host(np.zeros((3, 4), np.uint8), 2.0, 8) == 0).all()


def test_slice_wise_mode_blurs_every_slice_on_its_own():
    img = D.inputs((6, 9, 11), "q8", seed=9)
    whole = hmt.blur_image_host(img, [1.0, 1.5, 7.0], 8, dim=2)                       # z left alone: its sigma is not read
    for z in range(img.shape[0]):
        assert whole[z].tobytes() == hmt.blur_image_host(img[z], [1.0, 1.5], 8).tobytes()
    whole = hmt.blur_image_host(img, [7.0, 1.5, 1.0], 8, dim=0)                       # x left alone
    for x in range(img.shape[2]):
        assert np.ascontiguousarray(whole[:, :, x]).tobytes() == hmt.blur_image_host(np.ascontiguousarray(img[:, :, x]), [1.5, 1.0], 8).tobytes()
    tall = D.inputs((9, 1), "q8")                                                     # 2D, x left alone: the lines along y are blurred
    col = hmt.blur_image_host(tall, 1.0, 3, dim=0)
    assert col.tobytes() == D.blur(tall, 1.0, 3, 0).tobytes() and col.tobytes() != tall.tobytes()


# ---- argument errors of the device call: before any HIP call ------------------------------------------------------------------
def _call(ctx=0x1000, dim=3, dims=(4, 5, 6), ptype=0, src=0x2000, var=(1.0, 1.0, 1.0), width=3, skip=-1, dst=0x3000, host=False):
    lib = hmt.lib()
    d = None if dims is None else (C.c_int64 * 3)(*dims)
    v = None if var is None else (C.c_double * 3)(*var)
    if host:
        rc = lib.glia_hmt_blur_image_host(C.c_int(dim), d, C.c_int(ptype), C.c_void_p(src), v, C.c_int(width), C.c_int(skip), C.c_void_p(dst))
    else:
        rc = lib.glia_hmt_blur_image(C.c_void_p(ctx), C.c_int(dim), d, C.c_int(ptype), C.c_void_p(src), v, C.c_int(width), C.c_int(skip),
                                     C.c_void_p(dst))
    return rc, lib.glia_hmt_last_error().decode()


ERRORS = [
    ("NULL ctx", dict(ctx=None)),
    ("NULL dims", dict(dims=None)),
    ("NULL variance", dict(var=None)),
    ("NULL input", dict(src=None)),
    ("NULL output", dict(dst=None)),
    ("dim 1", dict(dim=1)),
    ("dim 4", dict(dim=4)),
    ("zero extent", dict(dims=(4, 0, 6))),
    ("negative extent", dict(dims=(-4, 5, 6))),
    ("zero z extent in 3D", dict(dims=(4, 5, 0))),
    ("2^32 - 1 voxels", dict(dims=(0xFFFFFFFF, 1, 1))),
    ("product past 2^64", dict(dims=(1 << 31, 1 << 31, 1 << 31))),
    ("zero variance", dict(var=(1.0, 0.0, 1.0))),
    ("negative variance", dict(var=(-1.0, 1.0, 1.0))),
    ("NaN variance", dict(var=(1.0, 1.0, float("nan")))),
    ("infinite variance", dict(var=(float("inf"), 1.0, 1.0))),
    ("variance above the limit", dict(var=(1.0, 256.5, 1.0))),
    ("width 0", dict(width=0)),
    ("width above the limit", dict(width=129)),
    ("pixel type -1", dict(ptype=-1)),
    ("pixel type 3", dict(ptype=3)),
    ("skip_axis = dim", dict(skip=3)),
    ("skip_axis = dim in 2D", dict(dim=2, skip=2)),
    ("skip_axis -2", dict(skip=-2)),
    ("in place", dict(src=0x2000, dst=0x2000)),
]


@pytest.mark.parametrize("what,kw", ERRORS)
def test_argument_errors_come_before_any_hip_call(what, kw):
    rc, msg = _call(**kw)
    assert rc == ERR_ARG, what
    assert msg.startswith("blur_image:"), (what, msg)


@pytest.mark.parametrize("what,kw", [e for e in ERRORS if e[0] not in ("NULL ctx",)])
def test_the_host_definition_refuses_the_same_arguments(what, kw):
    """(none of them lets the host function follow the made-up pointers)"""
    rc, msg = _call(host=True, **kw)
    assert rc == ERR_ARG and msg.startswith("blur_image:"), (what, msg)


def test_a_bad_variance_on_the_skipped_axis_is_not_read():
    hmt.set_option("GLIA_HMT_BLUR", "rows")         # the call gets past its argument tests and stops at the option, still without a GPU
    try:
        rc, msg = _call(var=(1.0, float("nan"), 1.0), skip=1)
        assert rc == ERR_ARG and "GLIA_HMT_BLUR" in msg
        rc, msg = _call(dim=2, dims=(4, 5, 0), var=(1.0, 1.0, -1.0))          # dims[2] and variance[2] are not looked at in 2D
        assert rc == ERR_ARG and "GLIA_HMT_BLUR" in msg
    finally:
        hmt.set_option("GLIA_HMT_BLUR", None)


def test_option_key_is_known_and_an_unknown_value_is_refused_by_name():
    for v in ("march", "passes", "rows"):           # the table takes any string: the call refuses it
        hmt.set_option("GLIA_HMT_BLUR", v)
    try:
        rc, msg = _call()
        assert rc == ERR_ARG and msg.startswith("blur_image:") and "GLIA_HMT_BLUR" in msg and "rows" in msg
    finally:
        hmt.set_option("GLIA_HMT_BLUR", None)


def test_gaussian_kernel_argument_errors():
    lib = hmt.lib()
    buf = (C.c_double * 4)()
    r = C.c_int(-1)

    def call(t=1.0, w=3, e=0.01, c=buf, cap=4, radius=r):
        rc = lib.glia_hmt_gaussian_kernel(C.c_double(t), C.c_int(w), C.c_double(e), c, C.c_int(cap), C.byref(radius) if radius is not None else None, None)
        return rc, lib.glia_hmt_last_error().decode()

    assert call()[0] == 0 and r.value == 3
    for kw in (dict(t=0.0), dict(t=-1.0), dict(t=float("nan")), dict(t=256.5), dict(w=0), dict(w=129), dict(e=0.0), dict(e=1.0), dict(c=None),
               dict(radius=None)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and msg.startswith("gaussian_kernel:"), kw
    rc, msg = call(cap=3)
    assert rc == hmt.ERR_CAPACITY and r.value == 3


def test_limits_and_header():
    lim = hmt.blur_limits()
    assert lim["tile_x"] >= 1 and lim["tile_y"] >= 1 and 1 <= lim["max_march_radius"] <= lim["max_radius"] == 128
    hdr = open(os.path.join(ROOT, "include", "glia_hmt.h")).read()
    for name in ("glia_hmt_gaussian_kernel", "glia_hmt_blur_image_host", "glia_hmt_blur_image", "glia_hmt_blur_limits", "glia_hmt_last_blur_timing",
                 "util/image.hxx:376-407", "GLIA_HMT_BLUR"):
        assert name in hdr


def test_sanitized_check_program_runs_clean():
    """cli/gaussian_kernel_check under -fsanitize=address,undefined: a stand-alone program on the CPU, nothing preloaded"""
    subprocess.check_call(["make", "-C", CLI, "gaussian_kernel_check_san"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(CLI, "gaussian_kernel_check_san")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
