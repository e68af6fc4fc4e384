"""-m gpu: the watershed's convergence machinery on inputs that reach it (tests/_ws_cases.py), exact equality throughout.
tests/test_gpu_watershed.py floods smooth noise, where every path is a few voxels long; here: one-voxel corridors 8x and 16x
the tile kernels' inner-iteration caps inside ONE tile (they finish only because a capped tile queues itself again) and corridors
that cross tile faces on every row (the dirty lists hand the flood back and forth), plateaus through every tile (constants, slabs,
shells: the union-find under contention), exact ties (markers equidistant on a flat plateau; a level equal to a minimum's depth),
degenerate extents (one voxel, lines along each axis, last tiles one voxel thick, exact tiles), the block cache reused by calls of
other sizes, and the argument checks.  The analytic families are compared with their closed forms directly AND with the oracle
(pinned to the same closed forms without a GPU in tests/test_oracle_watershed.py); the rest with the oracle."""
import ctypes as C

import numpy as np
import pytest

import _ws_cases as W

pytestmark = pytest.mark.gpu

ANALYTIC = W.analytic_cases()
OTHERS = W.structured_cases() + W.random_cases()


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    c.close()


def _run(ctx, img, level):
    """the device's labels and n; also: the call leaves its input alone, and a second call returns the same bytes"""
    import torch
    d_img = torch.from_numpy(img).cuda()
    lab, n, sweeps = ctx.watershed(d_img, level)
    got = lab.cpu().numpy().view(np.uint32)
    assert d_img.cpu().numpy().tobytes() == img.tobytes()
    lab2, n2, _ = ctx.watershed(d_img, level)
    assert n2 == n and lab2.cpu().numpy().tobytes() == got.tobytes()
    assert d_img.cpu().numpy().tobytes() == img.tobytes()
    assert sweeps > 0
    return got, n, sweeps


@pytest.mark.parametrize("make", [c[1] for c in ANALYTIC], ids=[c[0] for c in ANALYTIC])
def test_device_equals_the_analytic_answer_and_the_oracle(ctx, make, request):
    from oracle import pyoracle as O
    img, level, exp, n_exp = make()
    got, n, sweeps = _run(ctx, img, level)
    if request.node.callspec.id.startswith("snake"):
        print("sweeps %s: %d" % (request.node.callspec.id, sweeps))
    assert n == n_exp
    assert got.shape == exp.shape and (got == exp).all()            # the closed form, not routed through the oracle
    ref, n_ref = O.watershed(img, level)
    assert n == n_ref and (got == ref).all()


@pytest.mark.parametrize("make", [c[1] for c in OTHERS], ids=[c[0] for c in OTHERS])
def test_device_equals_the_oracle(ctx, make):
    from oracle import pyoracle as O
    img, level, _, n_exp = make()
    got, n, _ = _run(ctx, img, level)
    ref, n_ref = O.watershed(img, level)
    assert n == n_ref and (n_exp is None or n == n_exp)
    assert (got == ref).all()


def test_block_cache_reused_by_calls_of_other_sizes(ctx):
    """scratch blocks come back from the process-wide cache uninitialised and up to half again too large: a call after calls of
    other sizes must give what a fresh context on an empty cache gives"""
    import torch
    from glia_amd import hmt
    cases = {img.shape: (img, level) for img, level, _, _ in (make() for _, make in W.random_cases()[:15])}
    order = [(32, 16, 48), (1, 1, 1), (65, 65), (32, 16, 48)]
    fresh = {}
    for shape in set(order):
        hmt.Context.release_cached_memory()
        c = hmt.Context(0)
        lab, n, _ = c.watershed(torch.from_numpy(cases[shape][0]).cuda(), cases[shape][1])
        fresh[shape] = (lab.cpu().numpy().tobytes(), n)
        c.close()
    hmt.Context.release_cached_memory()
    for shape in order:
        lab, n, _ = ctx.watershed(torch.from_numpy(cases[shape][0]).cuda(), cases[shape][1])
        assert (lab.cpu().numpy().tobytes(), n) == fresh[shape], shape
    assert fresh[(32, 16, 48)][1] > 1


def test_invalid_arguments_touch_nothing(ctx):
    """level < 0, level = nan, dim outside {2, 3}: GLIA_HMT_ERR_ARG before any work -- the label volume, n and sweeps keep what they
    held -- and the context goes on working"""
    import torch
    from glia_amd import hmt
    img, exp, n_exp = W.flat_with_pits(*W.FLAT_CASES[3])
    d_img = torch.from_numpy(img).cuda()
    for level in (-0.01, float("nan")):
        with pytest.raises(hmt.HmtError) as e:
            ctx.watershed(d_img, level)
        assert e.value.code == hmt.ERR_ARG
    out = torch.full(img.shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dims = (C.c_int64 * 3)(*img.shape[::-1])
    for dim, level in ((1, 0.0), (4, 0.0), (3, -0.01), (3, float("nan"))):
        n, sw = C.c_uint32(77), C.c_int(-5)
        rc = hmt.lib().glia_hmt_watershed(ctx.h, C.c_int(dim), dims, C.c_void_p(d_img.data_ptr()), C.c_double(level), C.c_void_p(out.data_ptr()),
                                          C.byref(n), C.byref(sw))
        assert rc == hmt.ERR_ARG and n.value == 77 and sw.value == -5
    ctx.sync()
    assert (out.cpu().numpy() == 0x5A5A5A5A).all()
    lab, n, _ = ctx.watershed(d_img, 0.0)
    assert n == n_exp and (lab.cpu().numpy().view(np.uint32) == exp).all()
