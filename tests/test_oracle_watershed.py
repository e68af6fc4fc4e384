"""orc_watershed against answers nobody computed with a watershed (tests/_ws_cases.py): the device code is only ever compared
with this oracle, and both were written to the same tie rules, so the oracle itself is pinned here -- flat images with pits
(nearest pit in Manhattan distance, ties to the smaller label), checkerboards, one-voxel corridors thousands of cells long
(levels 0 and 0.2: two basins split by path distance; 0.25: the far pit filled exactly to the corridor, the g == f equality; 0.3),
constants.  Also: the random family of tests/test_gpu_watershed_edges.py is shown non-degenerate on the oracle alone, and every
oracle output is held to the label invariants (1..n all used; markers numbered in raster order of their first voxel)."""
import numpy as np
import pytest

import _ws_cases as W
from oracle import pyoracle as O

ANALYTIC = W.analytic_cases()
STRUCTURED = W.structured_cases()
RANDOM = W.random_cases()


def _check_labels(img, level, lab, n):
    """labels are 1..n, all used; at level 0 the markers are the image's regional minima (recomputed here), one label per minimum,
    numbered in the raster order of their first voxels"""
    sizes = np.bincount(lab.reshape(-1), minlength=n + 1)
    assert len(sizes) == n + 1 and sizes[0] == 0 and (sizes[1:] > 0).all()
    if level != 0:
        return
    minima, comp = W.regional_minima(img)
    flat, cflat = lab.reshape(-1), comp.reshape(-1)
    at = np.flatnonzero(minima.reshape(-1))
    roots = np.unique(cflat[at])                                   # a plateau's id is its first voxel: sorted = raster order
    assert len(roots) == n
    assert (flat[roots] == np.arange(1, n + 1)).all()              # k-th minimum in raster order carries label k
    assert (flat[at] == flat[cflat[at]]).all()                     # and all of its plateau does


@pytest.mark.parametrize("make", [c[1] for c in ANALYTIC], ids=[c[0] for c in ANALYTIC])
def test_oracle_equals_the_analytic_answer(make):
    img, level, exp, n_exp = make()
    lab, n = O.watershed(img, level)
    assert n == n_exp
    assert (lab == exp).all()
    _check_labels(img, level, lab, n)


@pytest.mark.parametrize("shape", list(W.SNAKE_SHAPES), ids=W._sid)
def test_snake_geometry(shape):
    """the generator itself: a simple face-connected path of the documented length, and the expectation along it is the stated rule"""
    img, exp, n, path = W.snake(shape)
    L = W.SNAKE_SHAPES[shape]
    assert len(path) == L and len(set(path)) == L
    p = np.array(path)
    assert (np.abs(np.diff(p, axis=0)).sum(axis=1) == 1).all()
    cell = {c: i for i, c in enumerate(path)}                       # no shortcut: corridor cells touch only their path neighbours
    for i, c in enumerate(path):
        for ax in range(len(shape)):
            for s in (-1, 1):
                q = tuple(v + (s if k == ax else 0) for k, v in enumerate(c))
                assert abs(cell.get(q, i + 1) - i) == 1
    assert (img[tuple(p.T)][1:-1] == 0.5).all() and img[path[0]] == 0.0 and img[path[-1]] == 0.25 and (img == 1.0).sum() == img.size - L
    on_path = exp[tuple(p.T)]
    i = np.arange(L)
    assert (on_path[(i - 1 < L - 2 - i)] == 1).all() and (on_path[(i - 1 > L - 2 - i)] == 2).all() and (on_path[i - 1 == L - 2 - i] == 1).all()
    assert n == 2 and set(np.unique(exp)) == {1, 2}


@pytest.mark.parametrize("make", [c[1] for c in STRUCTURED], ids=[c[0] for c in STRUCTURED])
def test_oracle_on_volume_spanning_plateaus(make):
    img, level, _, n_exp = make()
    lab, n = O.watershed(img, level)
    assert n == n_exp
    _check_labels(img, level, lab, n)


def test_random_family_is_not_degenerate():
    """asserted on the oracle alone, so that a device pass on this family is not a pass on trivial inputs.  Reseeding
    (_ws_cases.SEED) is allowed only to a seed for which these hold as they stand."""
    shapes, deep, deep_between, many = set(), 0, 0, 0
    for _, make in RANDOM:
        img, level, _, _ = make()
        shapes.add(img.shape)
        lab, n = O.watershed(img, level)
        _check_labels(img, level, lab, n)
        many += n > 1
        if level > 0:
            n0 = O.watershed(img, 0.0)[1]
            assert n <= n0
            deep += 1
            deep_between += 1 < n < n0
    assert len(RANDOM) == 30 and shapes == set(W.RANDOM_SHAPES)
    assert deep > 0 and 2 * deep_between >= deep, (deep_between, deep)
    assert many >= 20, many
