"""-m gpu: glia_hmt_label_components (labelicc_image / labelcc_image) on both routes against the CPU reference of
tests/_cc_cases.py -- equality of uint32 volumes, no tolerance."""
import numpy as np
import pytest

import _cc_cases as K

pytestmark = pytest.mark.gpu
ROUTES = ("tiled", "global")


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _run(ctx, labels, mask, mode, route):
    """-> (components, n, the input volume as it is on the device after the call)"""
    from glia_amd import hmt
    d = _dev(labels)
    m = None if mask is None else _dev(mask)
    with hmt.options(GLIA_HMT_CC=route):
        out, n = ctx.label_components(d, mask=m, mode=mode)
    return out.cpu().numpy().view(np.uint32), n, d.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", [c.name for c in K.cases()])
def test_both_routes_equal_the_reference(ctx, name):
    c = K.case(name)
    ref, n_ref = K.expected(name)
    got = {}
    for route in ROUTES:
        out, n, after = _run(ctx, c.labels, c.mask, c.mode, route)
        assert n == n_ref, route
        assert (out == ref).all(), route
        assert n == int(out.max()) and len(np.unique(out[out != 0])) == n, route        # the labels 1..n are all used
        assert (after == c.labels).all(), route                                        # the input volume is unchanged
        got[route] = out
    assert got["tiled"].tobytes() == got["global"].tobytes()


@pytest.mark.parametrize("route", ROUTES)
def test_default_route_and_explicit_route_agree(ctx, route):
    c = K.case("synth_mod5_cropped")
    out, n = ctx.label_components(_dev(c.labels))
    ref, n_ref = K.expected(c.name)
    assert n == n_ref and (out.cpu().numpy().view(np.uint32) == ref).all()
    assert (_run(ctx, c.labels, None, "identity", route)[0] == ref).all()


@pytest.mark.parametrize("route", ROUTES)
def test_smaller_volume_after_a_larger_one_on_the_same_context(ctx, route):
    """the scratch blocks of the first call come back from the block cache with its contents"""
    for name in ("synth_mod5", "checker3d_two_labels", "mask_random_identity", "hand_identity", "one_voxel_label7"):
        c = K.case(name)
        out, n, _ = _run(ctx, c.labels, c.mask, c.mode, route)
        assert n == K.expected(name)[1] and (out == K.expected(name)[0]).all(), name


@pytest.mark.parametrize("route", ROUTES)
def test_three_different_extents_through_the_abi_order(ctx, route):
    """dims = (x, y, z) with x fastest: a tensor of shape (z, y, x) = (5, 37, 23) holding one rod along each axis.  The number of
    components and their order only come out right if the extents are taken in the ABI's order."""
    nz, ny, nx = 5, 37, 23
    a = np.zeros((nz, ny, nx), np.uint32)
    a[0, 0, :] = 1          # along x: starts at voxel 0
    a[2:, 3, 4] = 1         # along z
    a[4, 5:, 20] = 1        # along y
    a[1, 20, 7:9] = 1
    ref, n_ref = K.cc_reference(a)
    assert n_ref == 4 and ref[0, 0, nx - 1] == 1 and ref[1, 20, 8] == 2 and ref[nz - 1, 3, 4] == 3 and ref[4, ny - 1, 20] == 4
    out, n, _ = _run(ctx, a, None, "identity", route)
    assert n == 4 and (out == ref).all()
    # the same bytes read as another shape are another image
    b = a.reshape(nx, nz, ny)
    ref_b, n_b = K.cc_reference(b)
    out, n, _ = _run(ctx, b, None, "identity", route)
    assert n == n_b and (out == ref_b).all()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["synth_mod5_cropped", "mask_random_identity", "checker2d_two_labels"])
def test_identity_labelling_is_idempotent(ctx, route, name):
    c = K.case(name)
    once, n1, _ = _run(ctx, c.labels, c.mask, "identity", route)
    twice, n2, _ = _run(ctx, once, c.mask, "identity", route)
    assert n1 == n2 and (once == twice).all()


def test_relabel_after_components_sorts_by_size(ctx):
    """relabel_image after the labelling: sizes descending, ties by the first voxel (the component number is the tie's key)"""
    from glia_amd import hmt
    c = K.case("synth_mod5_cropped")
    ref, n_ref = K.expected(c.name)
    out, n = ctx.label_components(_dev(c.labels))
    m = hmt.relabel_image(ctx, out)
    got = out.cpu().numpy().view(np.uint32)
    assert m == n == n_ref
    sizes = np.bincount(ref.ravel(), minlength=n_ref + 1)[1:]
    order = np.lexsort((np.arange(n_ref), -sizes.astype(np.int64)))       # by size descending, then by component number
    new = np.zeros(n_ref + 1, np.uint32)
    new[order + 1] = np.arange(1, n_ref + 1)
    assert (got == new[ref]).all()
    assert (np.diff(np.bincount(got.ravel())[1:].astype(np.int64)) <= 0).all()
