"""The classifier merge loop under a one-column scorer, stated a second time in plain numpy / Python.

No ctypes, no oracle, no device.  The scorer is the stub the tests use -- saliency of an edge = 1 - mean of the boundary image over the
shared boundary of its two regions (full-vector column 31 with one image: x0.b0.mean) -- or F(mean) for a step function F (a forest of
stumps on that column).  With that scorer the loop needs no feature vector, only the sum and count of the image per directed leaf pair,
so a replay of 1800 merges on a 1801-region hub image takes about a second where the oracle, which re-scores from voxel lists, takes
more than nine minutes.  The oracle is the first author; tests/test_loop_definition.py holds this file to it where it can go, and
tests/test_gpu_wide_linkages.py holds the device to this file where it cannot.

    order, sal = generate(labels, image)                 # what merge_order_bc(FeatureStubClassifier(31)) has to return
    step = check(labels, image, order, sal)              # first step that breaks a rule, or -1
    st = stats(labels, image)                            # per merge: neighbour counts, list lengths, new edges, fragile pairs
    step, n, alive = chain_at_pop(labels, image, order, key)   # the fragile chain of the edge that merges leaf `key` away
    step, pairs, alive = chain_entries_at_pop(labels, image, order, key)   # ... its entries in the device's chain order

Rules, each with the place in the reference (glia/code/...) it restates:
  leaf pairs      _featdef.leaf_lists: the directed pair (own label, first differing valid neighbour) of every boundary voxel.
  alive pairs     a pair is alive unless its two leaves are in the same region and the reverse pair exists (TRegion::merge,
                  type/region.hxx:66-75, as _featdef.Region.merge: only a pair whose REVERSE is present cancels).
  shared boundary of regions X and Y: the alive pairs (a, b) with a in one and b in the other whose target leaf b still has an
                  alive pair of its own (TRegion::boundaryWith, region.hxx:42-51; getBoundary, util/struct.hxx:10-16).
  edge table      one edge per unordered label pair whose BOTH directed pairs exist (TBoundaryTable::init, type/boundary_table.hxx:
                  91-114); after a merge the new region inherits the table neighbours of the two it replaces (update, :121-167).
                  Regions that merely touch are no candidates.
  tie rule        among the edges of maximal saliency the one inserted last wins (top, :46-52, walks a multimap from its end).
                  Insertion order: the initial edges in lexicographic (r0, r1) order; after a merge of r0 < r1 the table is walked
                  in key order, which visits the neighbours rs < r0 (of either region) ascending, then the neighbours of r0 above
                  r0 ascending, then those of r1 alone ascending.
  new key         largest label + 1 + step (util/struct_merge.hxx:19-31).
Sums of Q8 values are exact in double, so on such images every saliency is the oracle's bit for bit.
"""
import numpy as np

import _featdef


def stub_score(mean):
    """orc_merge_order_bc / FeatureStubClassifier: 1 - x[index]; like every scorer here it maps an array of means to saliencies"""
    return 1.0 - mean


def stump_forest_score(thresholds):
    """F of a forest of stumps on the column: tree i sends x <= t_i to the leaf that votes for the predicted label (the walk goes
    left on <=, ml/rf: classForest), the value is votes / trees."""
    t = np.sort(np.asarray(thresholds, np.float64))
    n = len(t)
    return lambda mean: (n - np.searchsorted(t, mean, side="left")).astype(np.float64) / float(n)


def leaf_pairs(labels, image, mask=None):
    """(labels of the leaves ascending, directed leaf pairs ascending, sum of the image over each pair's voxels, their number) -- all the
    loop needs of the volume; the walk over the voxels is the slow part of a replay, so callers that replay an image several times pass
    this on as `leaves`"""
    pts, _, bnd = _featdef.leaf_lists(np.asarray(labels), mask)
    pairs = sorted(bnd)
    img = np.asarray(image).ravel()
    psum = np.array([float(np.sum(img[bnd[p]].astype(np.float64))) for p in pairs], np.float64)
    return sorted(pts), pairs, psum, np.array([len(bnd[p]) for p in pairs], np.float64)


def _others(lo, hi, r):
    """(which pairs of the unordered pair list (lo, hi) name r, the other end of each)"""
    m = (lo == r) | (hi == r)
    return m, np.where(lo[m] == r, hi[m], lo[m])


class Replay:
    """The state of the loop: the partition of the leaves, the edge table with saliencies and insertion numbers, and for stats()
    the touching pairs and list lengths.  Regions are dense ids: leaves 0 .. L-1 in label order, the region of step k is L + k;
    keys (labels) are monotone in ids, so id comparisons are key comparisons.  The table and the touching pairs are flat arrays of
    the LIVE pairs (never more than there were at the start), so a merge is a handful of array operations however wide it is."""

    def __init__(self, labels, image, mask=None, F=None, leaves=None):
        self.leaf_keys, pairs, psum, pcnt = leaves if leaves is not None else leaf_pairs(labels, image, mask)
        self.score = F if F is not None else stub_score
        self.L = L = len(self.leaf_keys)
        self.key0 = self.leaf_keys[-1] + 1                     # TRegionMap::maxKey() + 1 (type/region_map.hxx:70-75)
        self.id_of = {k: i for i, k in enumerate(self.leaf_keys)}
        self.pair_keys = pairs
        self.pa = np.array([self.id_of[a] for a, _ in pairs], np.int64)
        self.pb = np.array([self.id_of[b] for _, b in pairs], np.int64)
        self.psum, self.pcnt = psum, pcnt
        have = set(pairs)
        self.has_rev = np.array([(b, a) in have for a, b in pairs], bool)
        # a non-mutual pair is "fragile" when its target leaf has only mutual pairs of its own: whether it belongs to a shared
        # boundary then depends on which of the target's partners have been merged with it
        nm_out = np.bincount(self.pa[~self.has_rev], minlength=L)
        self.fragile = ~self.has_rev & (nm_out[self.pb] == 0)
        self.reg = np.arange(L, dtype=np.int64)
        self.nreg = 2 * L
        self.step = 0
        # touching pairs: regions that share a leaf pair in either direction (what the device keeps a record and list entries for)
        t = np.unique(np.stack([np.minimum(self.pa, self.pb), np.maximum(self.pa, self.pb)], 1), axis=0).reshape(-1, 2)
        self.t_lo, self.t_hi = t[:, 0].copy(), t[:, 1].copy()
        self.length = np.zeros(self.nreg, np.int64)
        self.length[:L] = np.bincount(t.ravel(), minlength=L)
        # the table: the mutual pairs, in lexicographic (r0, r1) order (pairs are sorted by label, ids follow the labels)
        m = self.has_rev & (self.pa < self.pb)
        self.e_lo, self.e_hi = self.pa[m].copy(), self.pb[m].copy()
        sal = np.empty(len(self.e_lo), np.float64)
        for a in np.unique(self.e_lo).tolist():
            S, N = self.boundary_sums(a)
            own = self.e_lo == a
            sal[own] = self._saliency(S[self.e_hi[own]], N[self.e_hi[own]])
        self.e_sal = sal
        self.e_seq = np.arange(1, len(sal) + 1, dtype=np.int64)
        self.seq = len(sal)

    def key(self, rid):
        return self.leaf_keys[rid] if rid < self.L else self.key0 + (rid - self.L)

    def rid(self, key):
        """dense id of a key, or None if no region has it (yet)"""
        key = int(key)
        if key in self.id_of:
            return self.id_of[key]
        k = key - self.key0
        return self.L + k if 0 <= k < self.step else None

    def _shared(self, r):
        """the pairs on the shared boundaries of region r with every other region, and the other region of each"""
        ra, rb = self.reg[self.pa], self.reg[self.pb]
        alive = ~(self.has_rev & (ra == rb))
        own = np.bincount(self.pa[alive], minlength=self.L)     # alive pairs per leaf
        sel = ((ra == r) != (rb == r)) & (own[self.pb] > 0)      # between r and somebody else: alive by the rule above
        return sel, np.where(ra == r, rb, ra)

    def boundary_pairs(self, x, y):
        """the directed leaf pairs (as labels) of the shared boundary of regions x and y"""
        sel, other = self._shared(x)
        return {self.pair_keys[i] for i in np.flatnonzero(sel & (other == y))}

    def boundary_sums(self, r):
        """sum and count of the image over the shared boundary of r with every other region, indexed by region id"""
        sel, other = self._shared(r)
        o = other[sel]
        return (np.bincount(o, weights=self.psum[sel], minlength=self.nreg), np.bincount(o, weights=self.pcnt[sel], minlength=self.nreg))

    def fragile_counts(self, r):
        ra, rb = self.reg[self.pa], self.reg[self.pb]
        sel = ((ra == r) != (rb == r)) & self.fragile
        return np.bincount(np.where(ra == r, rb, ra)[sel], minlength=self.nreg)

    def fragile_chain(self, x, y):
        """(the fragile pairs between regions x and y -- what the device chains on their record --, how many of them are on the shared
        boundary now: those whose target leaf has an alive pair left)"""
        ra, rb = self.reg[self.pa], self.reg[self.pb]
        sel = self.fragile & (((ra == x) & (rb == y)) | ((ra == y) & (rb == x)))
        own = np.bincount(self.pa[~(self.has_rev & (ra == rb))], minlength=self.L)
        return int(sel.sum()), int((sel & (own[self.pb] > 0)).sum())

    def _saliency(self, s, n):
        mean = np.zeros(len(s), np.float64)                     # ImageRealFeats::generate: nothing is touched for an empty list
        np.divide(s, n, out=mean, where=n > 0)
        return np.asarray(self.score(mean), np.float64)

    def edge(self, r0, r1):
        """position of the table edge (r0, r1), r0 < r1, or None"""
        i = np.flatnonzero((self.e_lo == r0) & (self.e_hi == r1))
        return int(i[0]) if len(i) else None

    def top(self):
        """(r0, r1, saliency) of the edge TBoundaryTable::top returns: greatest saliency, among equals the last inserted; None when
        the table is empty"""
        if not len(self.e_sal):
            return None
        i = np.flatnonzero(self.e_sal == self.e_sal.max())
        i = int(i[np.argmax(self.e_seq[i])])
        return int(self.e_lo[i]), int(self.e_hi[i]), float(self.e_sal[i])

    def merge(self, r0, r1, want_stats=False):
        """TBoundaryTable::update + TRegionMap::merge for the table edge (r0, r1), r0 < r1; returns the new region's id"""
        assert r0 < r1 and self.edge(r0, r1) is not None
        r2 = self.L + self.step
        m0, n0 = _others(self.e_lo, self.e_hi, r0)
        m1, n1 = _others(self.e_lo, self.e_hi, r1)
        tm0, t0 = _others(self.t_lo, self.t_hi, r0)
        tm1, t1 = _others(self.t_lo, self.t_hi, r1)
        info = None
        if want_stats:
            info = dict(tab0=len(n0), tab1=len(n1), live0=len(t0), live1=len(t1), len0=int(self.length[r0]), len1=int(self.length[r1]))
        self.reg[(self.reg == r0) | (self.reg == r1)] = r2
        self.step += 1
        n0, n1 = n0[n0 != r1], n1[n1 != r0]
        both = np.union1d(n0, n1)
        # the walk of the table in key order: rs < r0 first, then r0's neighbours above it, then those of r1 alone
        cat = np.where(both < r0, 0, np.where(np.isin(both, n0), 1, 2))
        visit = both[np.lexsort((both, cat))]
        S, N = self.boundary_sums(r2)
        keep = ~(m0 | m1)
        self.e_lo = np.concatenate([self.e_lo[keep], visit])
        self.e_hi = np.concatenate([self.e_hi[keep], np.full(len(visit), r2, np.int64)])
        self.e_sal = np.concatenate([self.e_sal[keep], self._saliency(S[visit], N[visit])])
        self.e_seq = np.concatenate([self.e_seq[keep], self.seq + 1 + np.arange(len(visit), dtype=np.int64)])
        self.seq += len(visit)
        new = np.union1d(t0[t0 != r1], t1[t1 != r0])
        tkeep = ~(tm0 | tm1)
        self.t_lo = np.concatenate([self.t_lo[tkeep], new])
        self.t_hi = np.concatenate([self.t_hi[tkeep], np.full(len(new), r2, np.int64)])
        self.length[r2] = len(new)
        if want_stats:
            fc = self.fragile_counts(r2)
            info.update(new_edges=len(both), new_records=len(new), fragile=int(fc.max()) if len(fc) else 0)
            return r2, info
        return r2


def generate(labels, image, mask=None, F=None, leaves=None, want_stats=False):
    """(order [n, 3] uint32, saliencies [n] float64) of the loop: genMergeOrderGreedy (util/struct_merge.hxx:13-33) with the
    condition that is always true.  want_stats: also what stats() returns for that order, from the same replay."""
    rp = Replay(labels, image, mask, F, leaves)
    order, sal, rows = [], [], []
    while True:
        t = rp.top()
        if t is None:
            break
        r0, r1, s = t
        r2 = rp.merge(r0, r1, want_stats)
        if want_stats:
            r2, info = r2
            rows.append(info)
        order.append((rp.key(r0), rp.key(r1), rp.key(r2)))
        sal.append(s)
    out = np.array(order, np.uint32).reshape(len(order), 3), np.array(sal, np.float64)
    return out + (_columns(rows),) if want_stats else out


def _columns(rows):
    return {k: np.array([r[k] for r in rows], np.int64) for k in (rows[0] if rows else {})}


def check(labels, image, order, saliencies, mask=None, F=None, explain=False, leaves=None):
    """The first step of (order, saliencies) that breaks a rule of the loop, or -1; len(order) when the order ends with edges left
    in the table.  explain: returns (step, which rule) instead."""
    rp = Replay(labels, image, mask, F, leaves)

    def out(i, why):
        return (i, why) if explain else i

    for i, ((a, b, c), s) in enumerate(zip(np.asarray(order).tolist(), np.asarray(saliencies, np.float64).tolist())):
        if c != rp.key0 + i:
            return out(i, "the new key is not the largest label + 1 + step")
        r0, r1 = rp.rid(a), rp.rid(b)
        e = rp.edge(r0, r1) if r0 is not None and r1 is not None and r0 < r1 else None
        if e is None:
            return out(i, "the merged pair is no edge of the table")
        sal = float(rp.e_sal[e])
        if np.float64(sal).view(np.uint64) != np.float64(s).view(np.uint64):
            return out(i, "the saliency is not the recomputed one (%r, recomputed %r)" % (s, sal))
        t0, t1, ts = rp.top()
        if ts > sal:
            return out(i, "a table edge has a greater saliency")
        if (t0, t1) != (r0, r1):
            return out(i, "among equal saliencies another edge was inserted later")
        rp.merge(r0, r1)
    if rp.top() is not None:
        return out(len(order), "the order ends with edges left in the table")
    return out(-1, "")


def chain_at_pop(labels, image, order, key, mask=None, leaves=None):
    """(the step of `order` that merges the region with label `key` away, the fragile pairs between the two merged regions at that
    step, how many of them are alive): how long and how dead the chain is that the popped edge was scored with"""
    rp = Replay(labels, image, mask, leaves=leaves)
    for i, (a, b, _) in enumerate(np.asarray(order).tolist()):
        r0, r1 = rp.rid(a), rp.rid(b)
        if key in (a, b):
            return (i,) + rp.fragile_chain(r0, r1)
        rp.merge(r0, r1)
    return None


def chain_entries_at_pop(labels, image, order, key, mask=None, leaves=None):
    """(the step of `order` that merges the region with label `key` away, the fragile pairs (a, b) -- leaf labels -- between the two
    merged regions in the order of the device's chain, whether each is alive).  The chain's order is structural: a record of two
    leaves starts with its one fragile pair (a leaf pair has at most one non-mutual direction); when r0 < r1 become r2, a neighbour's
    record with r2 takes the chain of its record with r0 followed by that of its record with r1 (greedy_bc.hip, "the fragile-entry
    chains of the parents, concatenated in (r0 side, r1 side) order").  No float goes into it."""
    rp = Replay(labels, image, mask, leaves=leaves)
    chains = {}                                   # region -> {other region -> list of pair indices}, the same list from both sides
    for i in np.flatnonzero(rp.fragile).tolist():
        a, b = int(rp.pa[i]), int(rp.pb[i])
        lst = [i]
        chains.setdefault(a, {})[b] = lst
        chains.setdefault(b, {})[a] = lst
    for step, (a, b, _) in enumerate(np.asarray(order).tolist()):
        r0, r1 = rp.rid(a), rp.rid(b)
        if key in (a, b):
            entries = chains.get(r0, {}).get(r1, [])
            ra, rb = rp.reg[rp.pa], rp.reg[rp.pb]
            own = np.bincount(rp.pa[~(rp.has_rev & (ra == rb))], minlength=rp.L)
            return step, [rp.pair_keys[i] for i in entries], [bool(own[rp.pb[i]] > 0) for i in entries]
        r2 = rp.merge(r0, r1)
        new = {}
        for side, partner in ((r0, r1), (r1, r0)):
            for other, lst in chains.pop(side, {}).items():
                if other != partner:
                    new[other] = new[other] + lst if other in new else lst
                    del chains[other][side]
        for other, lst in new.items():
            chains[other][r2] = lst
        if new:
            chains[r2] = new
    return None


def stats(labels, image, mask=None, F=None, order=None, leaves=None):
    """Per merge of `order` (default: the generated one), as int arrays in a dict:
         tab0, tab1     live table neighbours of r0 and r1 before the merge
         live0, live1   regions that touch r0 / r1 (share a leaf pair in either direction, mutual or not)
         len0, len1     lengths of the device's incident lists of r0 / r1: a list is created with one entry per touching region and
                        never changes its length (an entry is reused in place or dies)
         new_edges      table edges the merge inserts;   new_records: touching regions of the new region
         fragile        the largest number of fragile leaf pairs (see Replay.__init__) between the new region and one neighbour"""
    if order is None:
        return generate(labels, image, mask, F, leaves, want_stats=True)[2]
    rp = Replay(labels, image, mask, F, leaves)
    return _columns([rp.merge(rp.rid(a), rp.rid(b), want_stats=True)[1] for a, b, _ in np.asarray(order).tolist()])
