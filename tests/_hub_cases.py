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

fragile_comb_image(n): one record whose shared boundary holds n fragile leaf pairs, half of them dead when its edge pops.
fragile_comb_image_f32(n): the same labels under float32 values (the Q8 values plus a jitter below half a Q8 step), whose f64 sums of
squares depend on the order of the additions.
touching_comb_image(gy, gx, m, m2): a thin hub whose hub touches every region, so that a contraction has as many list entries as the
image has regions while only gy gx regions ever merge.  Their docstrings go through the contacts.

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


def fragile_comb_image(n, ysplit=1, ycol=(170, 192), seed=20251021):
    """labels and pb (Q8) of the fragile comb: 2 n + 1 rows x 7 columns, 2 n + 1 + ysplit regions.

        column    0 1 2 3 4 5 6
        row 0     W W W W W Y Y      the only W | Y contact
        row r     W W W W X Y Y      r = 1 + 2 i, cell i
        row r+1   W W V V X Y Y

    W = 1 (the hub), Y = 2 .. 1 + ysplit, X_i = 2 + ysplit + 2 i, V_i = X_i + 1.  Neighbours are visited x-1, x+1, y-1, y+1 and the
    FIRST differing one names the pair (tests/_featdef.py contour_traits):
      W <-> Y      mutual: (0, 4) has Y at x+1, (0, 5) has W at x-1 -- the table edge W-Y, and the only one Y has with the comb
      X_i <-> W    mutual: X's top pixel has W at x-1, W's (r, 3) has X at x+1
      X_i <-> V_i  mutual: X's bottom pixel has V at x-1, V's (r+1, 3) has X at x+1 (its x-1 is V itself)
      V_i <-> W    mutual: V's (r+1, 2) has W at x-1, W's (r+1, 1) has V at x+1; W's (r, 2) and (r+2, 2) reach V_{i-1} / V_i at y-1
      X_i, X_i+1   touch in column 4, but either pixel has a differing neighbour at x-1: no pair, no record
      Y -> X_i     NON-mutual: Y's two pixels (r, 5), (r+1, 5) have X at x-1, and no pixel of X ever gets as far as x+1.  X_i owns
                   mutual pairs only, so the pair is FRAGILE (_loopdef.Replay.fragile): it is on the shared boundary of Y and whoever
                   holds X_i exactly until X_i, W and V_i are one region.
    Values: background, row 0 aside, and Y in [0.75, 1); row 0 is 128/256; the W | X contact (row r, columns 3-4) in [0, 0.25); row r+1,
    columns 1-4, in [0.5, 0.75); Y's column 5 beside the cells in [ycol[0], ycol[1]) / 256, inside [0.5, 0.75).  Under 1 - mean (and
    any decreasing function of the mean) the hub first takes every X_i: the record W'-Y collects their n entries in one chain.  Then the
    V_i follow (mean of four pixels in [0.5, 0.75) and one or two of the background, 0.675 on average), and each kills one entry of
    that chain.  ycol puts W'-Y (the mean of column 5, and of two pixels of row 0) into the MIDDLE of them, so the edge pops on a chain
    that is part alive, part dead -- over the whole of [0.5, 0.75) it would pop in front of nearly all of them.
    The entries of a chain stand in the order in which the hub took the X_i (or its reverse), the order of their W | X contacts'
    means.  The tenth of the cells with the darkest contacts and the tenth with the brightest have column 5 in [0.5, 0.53) instead: a
    scorer that loses one END of the chain -- the entries past a full work list -- sees a mean that is off by 0.01, several steps of a
    255-stump forest, where the loss of as many entries of one kind would move it by a tenth of a step.
    ysplit > 1: Y is cut into ysplit labels stacked vertically, at cell boundaries.  Y_k <-> Y_k+1 is mutual through column 6 (y+1 / y-1;
    column 5 still sees X first); only the topmost part touches W mutually, the others get their table edge with the hub when the
    part above them has been merged into it.  Every part has a chain of its own; the two pixels of a Y_k | Y_k+1 contact are 179/256,
    just above the mean of column 5: the edge Y_k-Y_k+1 waits behind hub-Y_k, and the edge hub-Y_k+1 that follows it is worth what its
    chain is worth (with background values there it would lose saliency with every entry that dies, and pop when all are dead; with
    row 0's value the parts would merge with each other first)."""
    assert n >= 1 and 1 <= ysplit <= n and 128 <= ycol[0] < ycol[1] <= 192
    rng = np.random.default_rng(seed)
    H = 2 * n + 1
    lab = np.ones((H, 7), np.uint32)
    q8 = rng.integers(192, 256, (H, 7))
    cut = [0] + [1 + 2 * (n * k // ysplit) for k in range(1, ysplit)] + [H]
    for k in range(ysplit):
        lab[cut[k]:cut[k + 1], 5:] = 2 + k
    r = 1 + 2 * np.arange(n)
    x = (2 + ysplit + 2 * np.arange(n)).astype(np.uint32)
    lab[r, 4] = lab[r + 1, 4] = x
    lab[r + 1, 2] = lab[r + 1, 3] = x + 1
    q8[0, :] = 128
    q8[r, 3:5] = rng.integers(0, 64, (n, 2))
    q8[r + 1, 1:5] = rng.integers(128, 192, (n, 4))
    q8[1:, 5] = rng.integers(ycol[0], ycol[1], H - 1)
    by_contact = np.argsort(q8[r, 3] + q8[r, 4], kind="stable")
    ends = r[np.concatenate([by_contact[:n // 10], by_contact[n - n // 10:]])]
    q8[ends, 5], q8[ends + 1, 5] = rng.integers(128, 136, (2, len(ends)))
    for c in cut[1:-1]:
        q8[c - 1:c + 1, 6] = 179
    assert len(np.unique(lab)) == 2 * n + 1 + ysplit
    return lab, (q8 / 256.0).astype(np.float32)


def fragile_comb_image_f32(n, ysplit=1, ycol=(170, 192), seed=20251021, jitter_seed=1, width=2.0 ** -9):
    """fragile_comb_image's labels, and every pixel its Q8 value plus a seeded jitter in [0, width), width <= 2^-9, drawn with more
    bits than a float has and rounded once: a float32 with a full 24-bit mantissa.  A pixel stays inside its Q8 step [q, q + 1/256),
    so every value band of fragile_comb_image's docstring is kept -- column 5 beside the cells stays in [ycol) / 256 within [0.5, 0.75)
    -- and with them the shape of the order.  What changes is the arithmetic: the values of [0.5, 1) are multiples of 2^-24, whose
    plain sums are still exact in double, but a square needs 48 bits and the sum of a few dozen squares more than 53; the values
    below 2^-2 (the W | X contacts) have finer steps, and their plain sums are inexact too."""
    assert 0.0 < width <= 2.0 ** -9
    lab, q8 = fragile_comb_image(n, ysplit, ycol, seed)
    jitter = np.random.default_rng(jitter_seed).random(q8.shape) * width
    pb = (q8.astype(np.float64) + jitter).astype(np.float32)
    assert (np.floor(pb.astype(np.float64) * 256.0) == q8.astype(np.float64) * 256.0).all(), "a pixel left its Q8 step"
    return lab, pb


def touching_comb_image(gy, gx, m, m2=None, levels=None):
    """labels and pb as hub_image's: gy x gx cells of 4 x (max(m, m2) + 3) pixels around the hub (label 1), each holding one comb
    L R_1 .. R_t, every tooth 1 pixel wide and 2 tall, t = m in the even cells (counted row by row) and m2 (default m) in the odd ones.
      L <-> hub    mutual: L's pixels have the hub at x-1, the hub's pixel left of L has L at x+1
      R_1 -> L, R_k -> R_k-1   NON-mutual: every pixel of a tooth has its left neighbour at x-1 and gets no further; R_1 -> L is
                   fragile (L owns only its mutual pair with the hub), R_k -> R_k-1 is not (R_k-1 owns a non-mutual pair)
      hub -> R_k   NON-mutual: the hub's pixels above and below a tooth reach it at y+1 / y-1 (left and right of them is the hub),
                   the pixel right of R_t at x-1; never fragile
    As on the thin hub only hub <-> L merges (gy gx merges), but the hub TOUCHES every tooth: its list starts with one entry per other
    region and a contraction's `total` (both lists) falls by one per merge, from regions + 1."""
    m2 = m if m2 is None else m2
    w = max(m, m2) + 3
    lab = np.ones((4 * gy, w * gx), np.uint32)
    nxt = 2
    for cy in range(gy):
        for cx in range(gx):
            t = m2 if (cy * gx + cx) % 2 else m
            y, x = 4 * cy + 1, w * cx + 1
            lab[y:y + 2, x:x + t + 1] = nxt + np.arange(t + 1, dtype=np.uint32)
            nxt += t + 1
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
