"""The classifier merge loop under a scorer that reads the FULL feature row, stated a second time: a brute-force author for dense MLP
weights (tests/test_gpu_bc_mlp.py, part 2).

The table, the alive-pair rule, the insertion order and the tie rule are tests/_loopdef.py's Replay, unchanged.  What differs is where a
new edge's saliency comes from: its full row, by tests/_featdef.py (Geometry + feature_rows for the order so far plus the candidate
merge), and the probability of that row by tests/_mlpdef.py.  No ctypes, no oracle, no device.

Geometry builds the region of a merge from its two parts and keeps the parts, so all candidate edges (rs, r2) of one step go into ONE
order as merges with keys of their own, and one feature_rows call gives their rows.  The row of (x0, x1) does not depend on the order
of the two unless their areas are equal (main_bc_feat.cxx:85-89 swaps on strictly greater).  An edge a merge creates is handed over as
(rs, r2) here and in the loop; an INITIAL edge in the region map's iteration order, which this file does not know: equal_area_edges
counts the initial edges of equal areas, and a test image has none.

Python sums the statistics in its own order, so a feature may differ from the device's in the last ulp and a probability with it:
`gaps` holds, per step, the distance between the best and the second-best saliency of the table; a test compares orders only where
every gap is either exactly 0 (the tie rule decides) or far above rounding."""
import numpy as np

import _featdef
import _loopdef
import _mlpdef


class RowReplay(_loopdef.Replay):
    def __init__(self, labels, image, model, bins=8, leaves=None):
        """model: dict(weights, n1, n2, mn, mx, dist) as tests/_bc_mlp_cases.py's"""
        self.labels_img, self.image_img, self.model, self.bins = np.asarray(labels), np.asarray(image), model, bins
        self.order_keys, self.rows_scored, self.equal_area_edges = [], [], 0
        self._cur = None
        super().__init__(labels, image, None, None, leaves)

    # Replay asks boundary_sums(r) for sums indexed by region and hands _saliency the entries of the neighbours it scores: here the
    # "sums" are the region ids themselves, so _saliency learns which edges (neighbour, r) it is asked about
    def boundary_sums(self, r):
        self._cur = int(r)
        return np.arange(self.nreg, dtype=np.float64), np.ones(self.nreg)

    def rows_of(self, pairs):
        """the full rows of the edges `pairs` [(x0, x1)] (region ids) in the current state"""
        if not len(pairs):
            return np.zeros((0, 0))
        top = self.key0 + 4 * self.L                       # keys no region has
        order = self.order_keys + [(self.key(a), self.key(b), top + i) for i, (a, b) in enumerate(pairs)]
        g = _featdef.Geometry(self.labels_img, None, order)
        if not self.order_keys:                            # (later edges are handed over as (rs, r2) on both sides)
            self.equal_area_edges += sum(len(g.lists[self.key(a)][0]) == len(g.lists[self.key(b)][0]) for a, b in pairs)
        pb = self.image_img
        rows = _featdef.feature_rows(g, pb, rb=[(pb, self.bins, 0.0, 1.0)])
        return rows[len(self.order_keys):]

    def _saliency(self, s, n):
        others = [int(v) for v in np.asarray(s).tolist()]
        # initial edges are (lo, hi) = (r, other); updated edges are passed as (rs, r2) (util/struct_merge_bc.hxx)
        pairs = [(self._cur, o) if not self.order_keys else (o, self._cur) for o in others]
        rows = self.rows_of(pairs)
        if not len(pairs):
            return np.zeros(0)
        self.rows_scored.extend(rows)
        m = self.model
        return _mlpdef.sigmoid(_mlpdef.logits(m["weights"], m["n1"], m["n2"], rows, m["mn"], m["mx"], m["dist"]))

    def merge(self, r0, r1, want_stats=False):
        self.order_keys.append((self.key(r0), self.key(r1), self.key0 + self.step))
        return super().merge(r0, r1, want_stats)


def initial_rows(labels, image, bins=8):
    """(table edges [(lo, hi)] as labels in lexicographic order, their full rows): what min/max tables are made from"""
    rp = RowReplay(labels, image, dict(weights=np.zeros(_mlpdef.n_weights(_featdef.feat_dim(np.ndim(labels), 3, [bins], [], [bins]), 1, 1)),
                                       n1=1, n2=1, mn=None, mx=None, dist=None), bins)
    return [(rp.key(int(a)), rp.key(int(b))) for a, b in zip(rp.e_lo, rp.e_hi)], np.array(rp.rows_scored)


def generate(labels, image, model, bins=8):
    """(order [n, 3] uint32, saliencies [n], gaps [n], replay): gaps[i] = best minus second-best saliency in the table before
    merge i (inf with one value left)"""
    rp = RowReplay(labels, image, model, bins)
    order, sal, gaps = [], [], []
    while True:
        t = rp.top()
        if t is None:
            break
        r0, r1, s = t
        top2 = np.sort(rp.e_sal)[-2:]
        gaps.append(float(top2[1] - top2[0]) if len(top2) > 1 else np.inf)
        r2 = rp.merge(r0, r1)
        order.append((rp.key(r0), rp.key(r1), rp.key(r2)))
        sal.append(s)
    return np.array(order, np.uint32).reshape(len(order), 3), np.array(sal, np.float64), np.array(gaps), rp
