"""The CPU reference of the component labelling (tests/_cc_cases.py) against answers that do not come from it: the hand literals,
closed-form component counts, and scipy.ndimage.label as a partition."""
import numpy as np
import pytest

import _cc_cases as K


@pytest.mark.parametrize("mode", K.MODES)
def test_hand_literals(mode):
    got, n = K.cc_reference(K.HAND_IN, None, mode)
    want, n_want = K.HAND_OUT[mode]
    assert n == n_want and (got == want).all()


@pytest.mark.parametrize("name", sorted(K.KNOWN_N))
def test_closed_form_counts(name):
    ref, n = K.expected(name)
    c = K.case(name)
    assert n == K.known_n(name)
    assert ref.shape == c.labels.shape and ref.dtype == np.uint32
    assert int(ref.max(initial=0)) == n and len(np.unique(ref[ref != 0])) == n


def test_every_case_has_a_unique_name_and_is_small():
    names = [c.name for c in K.cases()]
    assert len(set(names)) == len(names)
    assert all(c.labels.size <= 48 * 64 * 64 for c in K.cases())


def test_numbering_follows_the_first_voxel_not_the_tile():
    c, (ref, _) = K.case("raster_not_tile_order_2d"), K.expected("raster_not_tile_order_2d")
    assert ref[0, K.T2 + 3] == 1 and ref[1, 0] == 2
    ref, _ = K.expected("raster_not_tile_order_3d")
    assert ref[0, 0, K.T + 3] == 1 and ref[K.T + 3, 0, K.T + 3] == 1 and ref[0, 1, 0] == 2 and ref[K.T + 1, 3, 0] == 3
    assert c.labels[0, K.T2 + 3] == c.labels[1, 0]


def test_first_voxels_ascend_in_raster_order():
    for c in K.cases():
        ref, n = K.expected(c.name)
        flat = ref.ravel()
        first = np.full(n + 1, flat.size, np.int64)
        np.minimum.at(first, flat, np.arange(flat.size))
        assert (np.diff(first[1:]) > 0).all(), c.name


def test_mask_cases():
    ref, n = K.expected("mask_removes_first_voxel")
    assert n == 2 and ref.tolist() == [[0, 0, 1, 1], [2, 2, 2, 0]]
    ref, n = K.expected("mask_removes_first_voxel_unmasked")
    assert ref.tolist() == [[1, 0, 2, 2], [1, 1, 1, 0]]
    ref, n = K.expected("mask_removes_bridge")
    assert ref.tolist() == [[0] * 5, [1, 1, 0, 2, 2], [0] * 5]
    for c in K.cases():
        if c.mask is not None:
            assert (K.expected(c.name)[0][c.mask == 0] == 0).all(), c.name


def _same_partition(a, b):
    """a bijection between the non-zero labels of a and b that maps one volume onto the other"""
    a, b = a.ravel().astype(np.int64), b.ravel().astype(np.int64)
    if ((a == 0) != (b == 0)).any():
        return False
    pairs = np.unique(np.stack([a, b]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))


@pytest.mark.parametrize("name", [c.name for c in K.cases()])
def test_reference_against_scipy_as_a_partition(name):
    ndi = pytest.importorskip("scipy.ndimage")
    c = K.case(name)
    ref, n = K.expected(name)
    ok = np.ones(c.labels.shape, bool) if c.mask is None else c.mask != 0
    if c.mode != "identity":
        part = ((c.labels == 0) if c.mode == "binary_inverted" else (c.labels != 0)) & ok
        got, n_sp = ndi.label(part)                        # default structure: face connectivity
        assert n_sp == n and _same_partition(ref, got)
        return
    total = 0
    for v in np.unique(c.labels[(c.labels != 0) & ok]):
        got, n_sp = ndi.label((c.labels == v) & ok)
        total += n_sp
        assert _same_partition(np.where(got != 0, ref, 0), got)
    assert total == n
