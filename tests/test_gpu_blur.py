"""-m gpu: glia_hmt_blur_image on both routes (GLIA_HMT_BLUR = passes | march) against the host definition
(glia_hmt_blur_image_host, itself pinned to the NumPy second author by tests/test_blur_host.py) -- equality of bytes, no tolerance.
Shapes are sized from glia_hmt_blur_limits: the march tile (tx, ty) and the largest radius R the march route takes."""
import numpy as np
import pytest

import _blurdef as D
from glia_amd import hmt

pytestmark = pytest.mark.gpu
ROUTES = ("passes", "march")
LIM = hmt.blur_limits()
TX, TY, R = LIM["tile_x"], LIM["tile_y"], LIM["max_march_radius"]


def cut(r):
    """(sigma, max_width) of a kernel with radius exactly r: variance 64 reaches radius 21 on its own and is cut at r"""
    assert 2 <= r <= 21
    return 8.0, r


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    c = hmt.Context(0)
    yield c
    c.close()


def _check(ctx, img, sigma, width, skip=-1, expect_march=True):
    """both routes against the host definition; -> the bytes"""
    import torch
    want = hmt.blur_image_host(img, sigma, width, dim=skip)
    for route in ROUTES:
        d = torch.from_numpy(img).cuda()
        with hmt.options(GLIA_HMT_BLUR=route):
            out = ctx.blur_image(d, sigma, width, dim=skip)
            used = ctx.last_blur_timing()[1]
            again = ctx.blur_image(d, sigma, width, dim=skip)
        assert used == (route if expect_march else "passes"), (route, used)
        got = out.cpu().numpy()
        assert got.dtype == img.dtype and got.shape == img.shape
        assert got.tobytes() == want.tobytes(), (route, img.shape, sigma, width, skip, int((got.view(np.uint8) != want.view(np.uint8)).sum()))
        assert again.cpu().numpy().tobytes() == got.tobytes(), route                    # two calls return identical bytes
        assert d.cpu().numpy().tobytes() == img.tobytes(), route                        # the input is unchanged
    return want.tobytes()


def _radius(sigma, width):
    return hmt.gaussian_kernel(sigma * sigma, width)[1]


# (name, shape as (x, y[, z]), (sigma, max_width), radius it must have)
SHAPE_CASES = [
    ("one voxel", (1, 1, 1), (1.0, 3), 3),
    ("every extent below the radius", (2, 3, 2), cut(5), 5),
    ("tile edge -1 / +1", (TX - 1, TY + 1, 3), (1.0, 3), 3),
    ("tile edge +1 / -1, z = 2r", (TX + 1, TY - 1, 6), (1.0, 3), 3),
    ("several ragged tiles, z just past one ring", (2 * TX + 3, 2 * TY + 1, 8), (1.0, 3), 3),
    ("z extent 1", (TX + 1, TY + 1, 1), (1.0, 3), 3),
    ("z extent 2r + 1", (5, 7, 7), (1.0, 3), 3),
    ("several runs of planes", (7, 5, 131), cut(R), R),
    ("radius 1", (TX + 1, TY + 1, 2 * R + 3), (0.1, 32), 1),
    ("radius R", (TX + 1, TY + 1, 2 * R + 3), cut(R), R),
    ("2D tile + 1", (TX + 1, TY + 1), (1.0, 3), 3),
    ("2D one column", (1, 9), cut(R), R),
]


@pytest.mark.parametrize("name,shape,kernel,radius", SHAPE_CASES, ids=[c[0] for c in SHAPE_CASES])
def test_both_routes_equal_the_host_definition(ctx, name, shape, kernel, radius):
    assert _radius(*kernel) == radius
    _check(ctx, D.inputs(shape[::-1], "q8", seed=len(name)), *kernel)


def test_a_radius_above_the_march_limit_takes_passes_and_says_so(ctx):
    kernel = cut(R + 1)
    assert _radius(*kernel) == R + 1
    _check(ctx, D.inputs((2 * R + 3, TY + 1, TX + 1), "q8", seed=3), *kernel, expect_march=False)
    # one wide axis is enough
    _check(ctx, D.inputs((9, TY + 1, TX + 1), "q8", seed=4), [1.0, 8.0, 1.0], R + 1, expect_march=False)
    # ... but not when that axis is left alone
    assert _radius(1.0, R + 1) <= R
    _check(ctx, D.inputs((9, TY + 1, TX + 1), "q8", seed=4), [1.0, 8.0, 1.0], R + 1, skip=1)


@pytest.mark.parametrize("shape,skip", [((TX + 1, TY + 1, 9), 0), ((TX + 1, TY + 1, 9), 1), ((TX + 1, TY + 1, 9), 2), ((TX + 1, TY + 1), 0),
                                        ((TX + 1, TY + 1), 1)], ids=["3D skip x", "3D skip y", "3D skip z", "2D skip x", "2D skip y"])
def test_slice_wise_mode(ctx, shape, skip):
    _check(ctx, D.inputs(shape[::-1], "q8", seed=skip), 1.0, 3, skip=skip)
    _check(ctx, D.inputs(shape[::-1], "u8", seed=skip), *cut(R), skip=skip)


def test_unequal_sigma_per_axis(ctx):
    sig = [0.7, 2.0, 1.3]
    radii = [_radius(s, 32) for s in sig]
    assert len(set(radii)) == 3 and max(radii) <= R
    a = _check(ctx, D.inputs((2 * R + 2, TY + 3, TX + 5), "q8", seed=7), sig, 32)
    b = _check(ctx, D.inputs((2 * R + 2, TY + 3, TX + 5), "q8", seed=7), sig[::-1], 32)
    assert a != b
    _check(ctx, D.inputs((TY + 3, TX + 5), "q8", seed=7), sig[:2], 32)


@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_integer_pixels(ctx, kind):
    _check(ctx, D.inputs((2 * R + 2, TY + 1, TX + 1), kind, seed=1), 1.0, 3)
    _check(ctx, D.inputs((3, TY - 1, 2 * TX + 1), kind, seed=2), *cut(R))
    _check(ctx, D.inputs((TY + 1, TX + 1), kind, seed=3), 2.0, 8)
    top = np.full((4, 5, 6), np.iinfo(D.inputs((1,), kind).dtype).max, D.inputs((1,), kind).dtype)
    _check(ctx, top, 2.0, 8)


def test_int16_tensors_carry_uint16_pixels(ctx):
    import torch
    img = D.inputs((5, TY + 1, TX + 1), "u16", seed=5)
    want = hmt.blur_image_host(img, 1.0, 3)
    for route in ROUTES:
        with hmt.options(GLIA_HMT_BLUR=route):
            out = ctx.blur_image(torch.from_numpy(img.view(np.int16)).cuda(), 1.0, 3)
        assert out.dtype == torch.int16 and out.cpu().numpy().view(np.uint16).tobytes() == want.tobytes()


def test_nan_and_infinities_follow_ieee(ctx):
    img = D.inputs((2 * R + 2, TY + 1, TX + 1), "q8", seed=11)
    img[3, 5, 7] = np.float32("nan")
    img[6, TY, TX] = np.float32("inf")
    img[1, 0, 0] = np.float32("-inf")
    img[0, 2, 3] = np.float32(-0.0)
    got = np.frombuffer(_check(ctx, img, 1.0, 3), np.float32)
    assert np.isnan(got).any() and np.isinf(got).any() and np.isfinite(got).any()
    _check(ctx, img, 1.0, 3, skip=2)
    _check(ctx, img, 1.0, 3, skip=0)


def test_default_route_is_one_of_the_two_and_equals_the_definition(ctx):
    import torch
    img = D.inputs((9, TY + 1, TX + 1), "q8", seed=13)
    out = ctx.blur_image(torch.from_numpy(img).cuda(), 1.0, 3)
    ms, used = ctx.last_blur_timing()
    assert used in ROUTES and ms > 0.0
    assert out.cpu().numpy().tobytes() == hmt.blur_image_host(img, 1.0, 3).tobytes()


def test_mid_size_volume(ctx):
    _check(ctx, D.inputs((64, 80, 96), "q8", seed=17), 1.5, 8)
