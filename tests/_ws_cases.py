"""Watershed inputs whose answers are known without running any watershed (numpy only: no GPU, no oracle).

The tie rules under test (glia_amd/csrc/watershed.hip, oracle/hmt_oracle.cc: orc_watershed): markers are the regional minima of
the h-minima transform, numbered 1..n in raster order of their first voxel; every other voxel takes the marker that reaches it at
the lowest (flood level, steps since the level last rose, label).  The generators below build images on which that rule has a
closed form; each returns (image float32, expected labels uint32 or None, expected n or None) -- snake() adds the path.  Shapes
are numpy shapes, (z, y, x) or (y, x); raster order is C order.
"""
import numpy as np

SEED = 20240611

FLAT_CASES = [
    # pits in pairs at even distance (voxels exactly between two markers), across tile faces, in corners
    ((20, 35, 33), [(0, 0, 0), (19, 34, 32), (10, 17, 16), (3, 30, 5), (3, 30, 9), (15, 2, 20), (15, 4, 20), (15, 15, 15), (16, 16, 16)]),
    ((70, 130), [(0, 0), (69, 129), (35, 64), (35, 66), (10, 100), (60, 20), (63, 63), (64, 64)]),
    ((1, 1, 50), [(0, 0, 3), (0, 0, 20), (0, 0, 22), (0, 0, 49)]),
    ((33, 1, 17), [(0, 0, 0), (32, 0, 16), (16, 0, 8), (16, 0, 10)]),
]
FLAT_LEVELS = [0.0, 0.25, 0.5, 0.75]            # below the plateau (twice), exactly the plateau, above it
CHECKER_SHAPES = [(18, 17, 19), (65, 66)]
SNAKE_SHAPES = {(64, 64): 2079, (63, 130): 4191, (16, 16, 16): 1087, (5, 40, 40): 2459, (17, 18, 35): 2915}   # shape: path length
SNAKE_LEVELS = [0.0, 0.2, 0.25, 0.3]
CONSTANT_SHAPES = [(33, 40, 36), (130, 70)]
RANDOM_SHAPES = [(1, 1, 1), (1, 1, 37), (1, 37, 1), (37, 1, 1), (16, 16, 16), (17, 17, 17), (15, 33, 16), (2, 65, 18), (32, 16, 48),
                 (64, 64), (65, 65), (1, 130), (130, 1), (63, 129), (3, 200)]
N_RANDOM = 30


def _neighbour_min(a, fill):
    """per voxel: the minimum of a over its face neighbours (fill outside the volume)"""
    p = np.pad(a, 1, constant_values=fill)
    out = np.full(a.shape, fill, a.dtype)
    for ax in range(a.ndim):
        for s in (0, 2):
            idx = tuple(slice(s, s + a.shape[k]) if k == ax else slice(1, 1 + a.shape[k]) for k in range(a.ndim))
            out = np.minimum(out, p[idx])
    return out


def flat_with_pits(shape, pits, plateau=0.5, level=0.0):
    """Constant `plateau` with value 0 at each pit.  Below the plateau every pit is a marker; the flood rises once (pit -> its
    neighbours, distance 0) and then walks the plateau, so a voxel takes the pit at the smallest Manhattan distance (the box is
    unobstructed: geodesic = Manhattan), ties to the smaller label.  At level >= plateau the h-minima transform fills every pit
    up to one plateau: one label."""
    pits = sorted(tuple(int(c) for c in p) for p in pits)                       # raster order = lexicographic in (z, y, x)
    for i, a in enumerate(pits):
        for b in pits[i + 1:]:
            assert sum(abs(u - v) for u, v in zip(a, b)) >= 2, "pits must not touch"
    img = np.full(shape, plateau, np.float32)
    for p in pits:
        img[p] = 0.0
    if level >= plateau or not pits:
        return img, np.ones(shape, np.uint32), 1
    grid = np.indices(shape)
    dist = np.stack([sum(np.abs(grid[k] - p[k]) for k in range(len(shape))) for p in pits])
    return img, (np.argmin(dist, axis=0) + 1).astype(np.uint32), len(pits)      # argmin: the first (smallest label) of equals


def checkerboard(shape):
    """f = (x + y + z) mod 2 at level 0: every 0-voxel is a marker of its own (raster numbering), every 1-voxel is one rise
    above all its neighbours and takes the smallest of their labels."""
    img = (np.indices(shape).sum(axis=0) % 2).astype(np.float32)
    zero = img == 0
    lab = np.zeros(shape, np.int64)
    lab[zero] = np.arange(1, int(zero.sum()) + 1)
    big = np.iinfo(np.int64).max
    nb = _neighbour_min(np.where(zero, lab, big), big)
    assert (nb[~zero] < big).all()
    return img, np.where(zero, lab, nb).astype(np.uint32), int(zero.sum())


def snake_path(shape):
    """the corridor's voxels in walking order: every second row, alternating direction, joined through one voxel of the odd
    rows; in 3D every second slice holds that 2D walk (alternately forwards and backwards), joined through one voxel of the odd slices"""
    ny, nx = shape[-2], shape[-1]
    plane = []
    for r, y in enumerate(range(0, ny, 2)):
        xs = range(nx) if r % 2 == 0 else range(nx - 1, -1, -1)
        if r:
            plane.append((y - 1, plane[-1][1]))
        plane.extend((y, x) for x in xs)
    if len(shape) == 2:
        return plane
    path = []
    for s, z in enumerate(range(0, shape[0], 2)):
        if s:
            path.append((z - 1,) + path[-1][1:])
        path.extend((z,) + c for c in (plane if s % 2 == 0 else plane[::-1]))
    return path


def snake(shape, level=0.0):
    """One-voxel corridor (0.5) through walls (1.0), first cell 0.0, last cell 0.25 -> (image, labels, n, path).
    Level < 0.25: two markers.  Along the corridor (flood level 0.5) the start's flood rises at cell 1 and the end's at cell
    L - 2, so cell i is i - 1 steps from the start and L - 2 - i from the end; the fewer steps win, equal steps go to label 1.
    The walls (flood level 1.0) rise from whatever touches them: a wall voxel with lower neighbours takes the smallest of their
    labels at distance 0, the remaining wall voxels are reached layer by layer over the wall plateau, each taking the smallest
    label of the layer before.  Level >= 0.25: the far pit is filled up to (0.25: exactly to) the corridor: one label."""
    path = snake_path(shape)
    L = len(path)
    img = np.ones(shape, np.float32)
    idx = tuple(np.array(path).T)
    img[idx] = 0.5
    img[path[0]] = 0.0
    img[path[-1]] = 0.25
    if level >= 0.25:
        return img, np.ones(shape, np.uint32), 1, path
    big = np.iinfo(np.int64).max
    lab = np.full(shape, big, np.int64)
    lab[idx] = snake_expected_on_path(L)
    while (lab == big).any():                                  # one layer of the wall plateau per pass
        nb = _neighbour_min(lab, big)
        lab = np.where(lab == big, nb, lab)
    return img, lab.astype(np.uint32), 2, path


def snake_expected_on_path(L):
    """the issue's rule, stated on its own: cell i of L belongs to the start if i - 1 < L - 2 - i, to the end if i - 1 > L - 2 - i,
    to the smaller label if equal"""
    out = np.empty(L, np.uint32)
    for i in range(L):
        a, b = i - 1, L - 2 - i
        out[i] = 1 if a < b else 2 if a > b else 1
    out[0], out[L - 1] = 1, 2
    return out


def constant(shape, value=0.5):
    return np.full(shape, value, np.float32), np.ones(shape, np.uint32), 1


# ---- structured images without a closed form for the whole volume: compared with the oracle only (n where it is evident) ----------
def staircase(shape, axis):
    """floor(c / 5) / 8 along one axis: slabs through every tile, one marker (the lowest step)"""
    c = np.indices(shape)[axis]
    return (np.floor(c / 5) / 8).astype(np.float32), None, 1


def shells(shape, inverted=False):
    """quantised L-infinity distance from the centre, relative to the half extent of each axis: six nested box shells; inverted,
    the one marker is the hollow outer shell (every face of the volume)"""
    grid = np.indices(shape)
    rel = np.max(np.stack([np.abs(2 * grid[k] - (shape[k] - 1)) / (shape[k] - 1) for k in range(len(shape))]), axis=0)
    q = np.minimum(np.floor(6 * rel), 5)
    if inverted:
        q = 5 - q
    return (q / 8).astype(np.float32), None, 1


def w_profile(shape):
    """|  |2x - (nx - 1)| - 2 (nx / 4)  | / 64 along x: two equal minima with a hump between them.  -> (image, None, 2, hump):
    hump = the height of the middle above the minima (level == hump joins the two, the g == f equality of the transform)"""
    nx = shape[-1]
    x = np.indices(shape)[-1]
    v = np.abs(np.abs(2 * x - (nx - 1)) - 2 * (nx // 4))
    img = (v / 64).astype(np.float32)
    hump = float(v[..., (nx - 1) // 2].max() - v.min()) / 64
    return img, None, 2, hump


def random_quantised(i):
    """case i of the random family -> (image, level).  Deterministic.  Noise, 0-2 box passes, normalised, floored to q dyadic
    steps, then mapped by x1 / x255 / -0.5 / +1000; level = {0, 1, 2} / q of the scale, i.e. often exactly a step's depth."""
    shape = RANDOM_SHAPES[i % len(RANDOM_SHAPES)]
    rng = np.random.default_rng([SEED, i])
    img = rng.random(shape)
    for _ in range(int(rng.integers(0, 3))):
        for ax in range(len(shape)):
            if shape[ax] > 1:
                img = (img + np.roll(img, 1, ax) + np.roll(img, -1, ax)) / 3.0
    span = img.max() - img.min()
    img = (img - img.min()) / span if span > 0 else np.zeros(shape)
    q = int(rng.choice([2, 4, 8, 16]))
    img = np.minimum(np.floor(img * q), q - 1) / q
    k = int(rng.integers(0, 3))
    m = int(rng.integers(0, 4))
    scale = 255.0 if m == 1 else 1.0
    img = img * 255.0 if m == 1 else img - 0.5 if m == 2 else img + 1000.0 if m == 3 else img
    return img.astype(np.float32), k / q * scale


# ---- independent restatement of steps 1-2 at level 0, for the label invariants -------------------------------------------------
def regional_minima(img):
    """(mask of the voxels on a face-connected plateau without a lower neighbour, plateau id per voxel = its smallest raster index)"""
    n = img.size
    comp = np.arange(n, dtype=np.int64).reshape(img.shape)
    while True:                                                  # the smallest index spreads over each plateau
        new = comp
        for ax in range(img.ndim):
            for shift in (1, -1):
                nb_c = np.roll(new, shift, ax)
                same = np.roll(img, shift, ax) == img
                edge = [slice(None)] * img.ndim
                edge[ax] = 0 if shift == 1 else -1
                same[tuple(edge)] = False                        # no wrap-around
                new = np.where(same, np.minimum(new, nb_c), new)
        new = new.reshape(-1)[new]                               # (an id is a voxel of the same plateau: follow it)
        if (new == comp).all():
            break
        comp = new
    lower = _neighbour_min(img.astype(np.float64), np.inf) < img
    has_lower = np.zeros(n, bool)
    has_lower[comp[lower]] = True
    return ~has_lower[comp], comp


# ---- the case lists both test modules walk: (id, factory); factory() -> (image, level, expected labels or None, expected n or None) --
def _sid(shape):
    return "x".join(str(s) for s in shape)


def _at(level, r):
    return r[0], level, r[1], r[2]


def analytic_cases():
    out = []
    for shape, pits in FLAT_CASES:
        for lv in FLAT_LEVELS:
            out.append(("flat-%s-l%g" % (_sid(shape), lv), lambda s=shape, p=pits, l=lv: _at(l, flat_with_pits(s, p, level=l))))
    for shape in CHECKER_SHAPES:
        out.append(("checker-%s" % _sid(shape), lambda s=shape: _at(0.0, checkerboard(s))))
    for shape in SNAKE_SHAPES:
        for lv in SNAKE_LEVELS:
            out.append(("snake-%s-l%g" % (_sid(shape), lv), lambda s=shape, l=lv: _at(l, snake(s, l))))
    for shape in CONSTANT_SHAPES:
        for lv in (0.0, 0.5):
            out.append(("constant-%s-l%g" % (_sid(shape), lv), lambda s=shape, l=lv: _at(l, constant(s))))
    return out


def _w_at_hump(shape):
    img, _, _, hump = w_profile(shape)
    return img, hump, None, 1


def structured_cases():
    out = []
    for shape in CONSTANT_SHAPES:
        for ax in range(len(shape)):
            out.append(("stairs-%s-ax%d" % (_sid(shape), ax), lambda s=shape, a=ax: _at(0.0, staircase(s, a))))
        for inv in (False, True):
            out.append(("shells-%s-%s" % (_sid(shape), "inv" if inv else "out"), lambda s=shape, v=inv: _at(0.0, shells(s, v))))
        out.append(("w-%s-l0" % _sid(shape), lambda s=shape: _at(0.0, w_profile(s))))
        out.append(("w-%s-hump" % _sid(shape), lambda s=shape: _w_at_hump(s)))
    return out


def random_cases():
    return [("random-%02d-%s" % (i, _sid(RANDOM_SHAPES[i % len(RANDOM_SHAPES)])), lambda i=i: random_quantised(i) + (None, None)) for i in range(N_RANDOM)]
