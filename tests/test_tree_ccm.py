"""segment_ccm's tree inference on the host (glia_hmt_tree_energies / _tree_energy_tuples / _resolve_tree_ccm / _tree_ccm_confidence) against
 - tests/golden/ccm/ccm_reference.npz: what the reference's own hmt/tree_build.hxx + hmt/tree_ccm.hxx compute for the same inputs (recorded
   by tests/golden/gen_ccm_reference.py; this test never touches the reference): tree arrays and picks identical, doubles bit-equal;
 - an independent known answer: for every small tree, the energy of the picks is the minimum over ALL cuts of the tree.
No GPU is needed.  Only the node energies -log(p) pass through a libm -- the recording host's in the file, the running host's in the
library, as in the reference -- and the two need not round alike.  So the chain is checked link by link, each bit for bit and none
depending on the host: the recorded energies are the project's pinned glibc log (variant 2, the FMA build the file was recorded with);
the library's energies are the pinned log of the variant THIS host's libm is (glia_hmt_host_libm_probe) -- on a host of variant 2 the two
together are bit equality with the file --; tuples, picks and confidences are computed from the RECORDED energies.  Where the host's
libm is no known variant, the library's energies are compared with the file directly."""
import itertools
import os

import numpy as np
import pytest

FMAX = np.finfo(np.float64).max
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ccm", "ccm_reference.npz")


@pytest.fixture(scope="module")
def ref():
    z = np.load(GOLDEN)
    return {name: {k: z[name + "/" + k] for k in ("order", "probs", "label", "parent", "child0", "child1", "em", "es", "Em", "Es", "pos", "neg",
                                                   "conf", "picks")} for name in z["names"].tolist()}


@pytest.fixture(scope="module")
def ours(ref):
    """the library's answer for every recorded case, computed once: tree and own energies from (order, probabilities); tuples, picks and
    confidences from the recorded own energies"""
    from glia_amd import hmt
    out = {}
    for name, c in ref.items():
        lab, par, c0, c1, em, es, Em_host, Es_host = hmt.tree_energies(c["order"], c["probs"])
        Em, Es = hmt.tree_energy_tuples(c0, c1, c["em"], c["es"])
        pos, neg, conf = hmt.tree_ccm_confidence(par, c0, c1, c["es"], Em, Es)
        out[name] = dict(label=lab, parent=par, child0=c0, child1=c1, em=em, es=es, Em=Em, Es=Es, Em_host=Em_host, Es_host=Es_host, pos=pos,
                         neg=neg, conf=conf, picks=hmt.resolve_tree_ccm(c0, c1, Em, Es))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_fixture_holds_the_cases_the_checks_rely_on(ref):
    names = list(ref)
    for kind in ("balanced", "chain", "random", "partial"):
        assert any(n.startswith(kind) for n in names)
    for kind in ("uniform", "edges", "half", "one", "zero"):
        assert any(kind in n for n in names)
    leaves = [int((c["child0"] < 0).sum()) for c in ref.values()]
    assert min(leaves) == 2 and max(leaves) == 400
    # a partial order's tree is a forest: more roots than one, the last node is one of them
    assert any((c["parent"] < 0).sum() > 1 and c["parent"][-1] < 0 for n, c in ref.items() if n.startswith("partial"))
    # both isfeq branches, FMAX saturation and exact ties occur
    allp = np.concatenate([c["probs"] for c in ref.values()])
    assert (allp == 0).any() and (allp == 1).any() and ((allp > 0) & (allp < 2.22e-16)).any() and ((allp < 1) & (1 - allp < 2.22e-16)).any()
    assert any((c["Em"] == FMAX).any() and (c["Es"] == FMAX).any() for c in ref.values())
    assert any(((c["Em"] == c["Es"]) & (c["child0"] >= 0)).any() for c in ref.values())


def _pinned_energies(c, variant):
    """own energies of the inner nodes in merge order through the project's restatement of glibc's log: (em, es)"""
    import ctypes as C
    from glia_amd import hmt
    p = np.ascontiguousarray(c["probs"][:len(c["order"])], np.float64)
    out = []
    for q in (p, 1.0 - p):
        q = np.ascontiguousarray(q)
        lg = np.empty_like(q)
        safe = np.where(np.abs(q) < 2.22e-16, 1.0, q)                          # isfeq(q, 0): FMAX, no logarithm taken
        assert hmt.lib().glia_hmt_host_libm_eval(C.c_int(1), C.c_int(variant), safe.ctypes.data_as(C.c_void_p), lg.ctypes.data_as(C.c_void_p),
                                                 C.c_int64(len(q))) == 0
        out.append(np.where(np.abs(q) < 2.22e-16, FMAX, -lg))
    return out


def _host_log_variant():
    import ctypes as C
    from glia_amd import hmt
    a, b = C.c_int(0), C.c_int(0)
    assert hmt.lib().glia_hmt_host_libm_probe(C.byref(a), C.byref(b)) == 0
    return b.value


def test_tree_arrays_identical(ref, ours):
    for name, c in ref.items():
        for k in ("label", "parent", "child0", "child1"):
            assert ours[name][k].shape == c[k].shape and (ours[name][k] == c[k]).all(), (name, k)


def test_recorded_energies_are_the_pinned_log(ref):
    for name, c in ref.items():
        inner, leaf = c["child0"] >= 0, c["child0"] < 0
        em, es = _pinned_energies(c, 2)
        assert (_bits(c["em"][inner]) == _bits(em)).all() and (_bits(c["es"][inner]) == _bits(es)).all(), name
        assert (c["em"][leaf] == 0).all() and (c["es"][leaf] == FMAX).all(), name


def test_own_energies_bit_equal(ref, ours):
    variant = _host_log_variant()
    for name, c in ref.items():
        o, inner = ours[name], c["child0"] >= 0
        if variant:
            em, es = _pinned_energies(c, variant)
            assert (_bits(o["em"][inner]) == _bits(em)).all() and (_bits(o["es"][inner]) == _bits(es)).all(), name
            assert (_bits(o["em"][~inner]) == _bits(c["em"][~inner])).all() and (_bits(o["es"][~inner]) == _bits(c["es"][~inner])).all(), name
        if variant in (0, 2):
            for k in ("em", "es"):
                assert (_bits(o[k]) == _bits(c[k])).all(), (name, k)
            assert (_bits(o["Em_host"]) == _bits(c["Em"])).all() and (_bits(o["Es_host"]) == _bits(c["Es"])).all(), name     # the one-call form


def test_energy_tuples_bit_equal(ref, ours):
    for name, c in ref.items():
        for k in ("Em", "Es"):
            assert (_bits(ours[name][k]) == _bits(c[k])).all(), (name, k)


def test_picks_identical(ref, ours):
    for name, c in ref.items():
        assert ours[name]["picks"].tolist() == c["picks"].tolist(), name


def test_confidence_bit_equal(ref, ours):
    for name, c in ref.items():
        for k in ("pos", "neg", "conf"):
            assert (_bits(ours[name][k]) == _bits(c[k])).all(), (name, k)


def _cuts(i, c0, c1):
    """all antichains that cover the leaves below node i"""
    yield (i,)
    if c0[i] >= 0:
        for a, b in itertools.product(list(_cuts(c0[i], c0, c1)), list(_cuts(c1[i], c0, c1))):
            yield a + b


def _below(i, c0, c1):
    out, stack = [], [i]
    while stack:
        x = stack.pop()
        out.append(x)
        if c0[x] >= 0:
            stack += [c0[x], c1[x]]
    return out


def _cut_energy(cut, root, c, em, es):
    """es of the nodes above the cut + em of the nodes at or below it (a leaf's em is 0).  An FMAX term saturates the sum, as
    stats::plusEqual does: returned as (saturated, finite sum)."""
    below = set()
    for x in cut:
        below.update(_below(x, c["child0"], c["child1"]))
    terms = [em[x] for x in below] + [es[x] for x in _below(root, c["child0"], c["child1"]) if x not in below]
    if any(t == FMAX for t in terms):
        return (1, 0.0)
    return (0, float(np.sum(np.array(terms, np.float64))))


def test_picks_minimise_the_cut_energy(ref, ours):
    """The reference plays no part here.  Tolerance: a tree of <= 9 leaves has <= 17 nodes, so every energy is a sum of <= 17 non-negative
    terms; the dynamic programme and this enumeration add them in different orders, each with a relative error below 17 * 2^-53, so the
    energy of the picks may exceed the enumerated minimum by at most ~4e-15 of it: 1e-13 relative (and absolute, for sums near 0) is asserted."""
    done = 0
    for name, c in ref.items():
        o = ours[name]
        o = dict(o, em=c["em"], es=c["es"])          # the energies the picks were made from
        root = len(o["parent"]) - 1
        if sum(1 for x in _below(root, o["child0"], o["child1"]) if o["child0"][x] < 0) > 9:
            continue
        best = min(_cut_energy(cut, root, o, o["em"], o["es"]) for cut in _cuts(root, o["child0"], o["child1"]))
        got = _cut_energy(tuple(o["picks"].tolist()), root, o, o["em"], o["es"])
        # the picks are a cut: an antichain covering the leaves below the root
        cover = sorted(x for p in o["picks"] for x in _below(p, o["child0"], o["child1"]) if o["child0"][x] < 0)
        assert cover == sorted(x for x in _below(root, o["child0"], o["child1"]) if o["child0"][x] < 0), name
        assert got[0] == best[0], name
        assert abs(got[1] - best[1]) <= 1e-13 * max(1.0, best[1]), (name, got, best)
        done += 1
    assert done >= 30


def test_argument_errors():
    import ctypes as C
    from glia_amd import hmt
    L = hmt.lib()
    L.glia_hmt_tree_energies.restype = C.c_int64
    L.glia_hmt_resolve_tree_ccm.restype = C.c_int64
    assert L.glia_hmt_tree_energies(None, C.c_int64(1), None, None, None, None, None, None, None, None, None, C.c_int64(0)) == -1
    assert L.glia_hmt_resolve_tree_ccm(None, None, None, None, C.c_int64(3), None, C.c_int64(0)) == -1
    assert L.glia_hmt_tree_ccm_confidence(None, None, None, None, None, None, C.c_int64(3), None, None, None) == -1
    assert L.glia_hmt_tree_energy_tuples(None, None, None, None, C.c_int64(3), None, None) == -1
    # capacity of the pick array
    lab, par, c0, c1, em, es, Em, Es = hmt.tree_energies(np.array([[1, 2, 4], [4, 3, 5]], np.uint32), np.array([0.1, 0.1]))
    picks = np.empty(1, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.glia_hmt_resolve_tree_ccm(ptr(c0), ptr(c1), ptr(Em), ptr(Es), C.c_int64(5), ptr(picks), C.c_int64(1)) == -4
    # both merges improbable: the root splits, node 2 (children queued behind leaf 3) splits: leaf 3 comes out first, then leaves 0, 1
    assert hmt.resolve_tree_ccm(c0, c1, Em, Es).tolist() == [3, 0, 1]
