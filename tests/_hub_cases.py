"""Hub images: one background region that touches every other region, so that its contractions are as wide as the image has regions.

hub_image(levels, grid): 6 grid x 6 grid pixels, background = label 1, a grid x grid array of 6 x 6 cells each holding a 3 x 4 blob split
into two 3 x 2 labels -- 2 grid^2 + 1 regions, and the background starts with 2 grid^2 list entries.  Every contact is mutual: each
label has pixels whose first differing neighbour is the hub and pixels whose first differing neighbour is its sibling, and the hub has
pixels that point at either.

thin_hub_image(grid): 4 x 4 cells, each holding a 2 x 2 blob split into two 2 x 1 labels.  Every pixel of a left half has the hub at x-1,
every pixel of a right half its sibling there (neighbours are visited x-1, x+1, y-1, y+1 and the FIRST differing one names the pair,
tests/_featdef.py contour_traits): a right half's only directed pair points at the left half, which never points back, and the hub's
pixels beside and above / below a right half point at it without an answer.  Only hub <-> left half is mutual, so only those merge, and
the right halves' entries are the ones whose membership in a shared boundary depends on the state of the merge forest.

width_classes(lab, order) replays an order on neighbour sets and list lengths and counts the merges that are certain to fall into each
class of CLASSES (tests/test_gpu_wide_passes.py says how a class is counted from both sides)."""
import numpy as np

CLASSES = [("global marks", 1409, None), ("three passes", 1025, 1408), ("two passes", 513, 1024), ("one pass", 193, 512),
           ("narrow, three per lane", 129, 192), ("narrow, two per lane", 65, 128)]
kMargin = 8
kGrid, kRegions = 30, 1801


def _quantised(shape, levels):
    pb = np.random.default_rng(20251020).integers(0, 256, shape).astype(np.float32) / np.float32(256)
    if levels:
        pb = np.floor(pb * levels).astype(np.float32) / np.float32(levels)
    return pb


def hub_image(levels, grid=kGrid):
    """labels (uint32) and pb (float32, seeded random Q8, floored to `levels` levels if given)"""
    lab = np.ones((6 * grid, 6 * grid), np.uint32)
    nxt = 2
    for cy in range(grid):
        for cx in range(grid):
            y, x = 6 * cy + 1, 6 * cx + 1
            lab[y:y + 3, x:x + 2] = nxt
            lab[y:y + 3, x + 2:x + 4] = nxt + 1
            nxt += 2
    assert nxt - 1 == 2 * grid * grid + 1
    return lab, _quantised(lab.shape, levels)


def thin_hub_image(grid, levels=None):
    """labels and pb as hub_image's; 2 grid^2 + 1 regions on 4 grid x 4 grid pixels"""
    lab = np.ones((4 * grid, 4 * grid), np.uint32)
    nxt = 2
    for cy in range(grid):
        for cx in range(grid):
            y, x = 4 * cy + 1, 4 * cx + 1
            lab[y:y + 2, x] = nxt
            lab[y:y + 2, x + 1] = nxt + 1
            nxt += 2
    assert nxt - 1 == 2 * grid * grid + 1
    return lab, _quantised(lab.shape, levels)


def width_classes(lab, order, complete=True):
    """Replays `order` (rows a, b, c: regions a and b become c) on neighbour sets.  Returns per class of CLASSES the number of merges
    whose contraction is certain to fall into it (see the module docstring).  complete: the order merges everything into one region."""
    nb = {}
    for a, b in ((lab[:, :-1], lab[:, 1:]), (lab[:-1, :], lab[1:, :])):
        m = a != b
        for u, v in set(zip(a[m].tolist(), b[m].tolist())):
            nb.setdefault(u, set()).add(v)
            nb.setdefault(v, set()).add(u)
    length = {r: len(s) for r, s in nb.items()}
    hits = [0] * len(CLASSES)
    for a, b, c in order.tolist():
        assert b in nb[a] and a in nb[b], "the order merges regions that are not neighbours"
        live, entries = len(nb[a]) + len(nb[b]), length[a] + length[b]
        assert live <= entries
        for j, (_, lo, hi) in enumerate(CLASSES):
            if live >= lo and (hi is None or entries <= hi - kMargin):
                hits[j] += 1
        new = (nb.pop(a) | nb.pop(b)) - {a, b}
        for r in new:
            nb[r] -= {a, b}
            nb[r].add(c)
        nb[c] = new
        length[c] = len(new)
    assert len(nb) == 1 or not complete
    return hits
