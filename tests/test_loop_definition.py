"""-m "not gpu": tests/_loopdef.py (the classifier loop under a one-column scorer, second author) held to the oracle's loop.

The oracle re-scores every new edge from voxel lists, so it reaches a hub image of 201 regions in a few seconds and one of 1801 not
at all; _loopdef.py replays that one in a second.  Here both run on everything the oracle can afford -- hub images (mutual contact
only; few levels and a constant image, where the tie rule decides), the thin hub image (mostly non-mutual contact), compact supervoxels
in 2D and 3D, a mask -- and must agree on the order and, bit for bit, on the saliencies; check() must accept the oracle's answer and
name the step of every spoiled one.  The flat shared-boundary rule is compared with _featdef.get_boundary on region objects."""
import numpy as np
import pytest

import _featdef
import _loopdef
from _hub_cases import fragile_comb_image, hub_image, thin_hub_image, touching_comb_image

STUB = 11 + 4 * 3 + 7 + 1          # x0.b0.mean: mean of the boundary image over the shared boundary


def _synth(shape, S):
    from oracle import pyoracle as O
    return O.synth(shape, S, 16 if len(shape) == 2 else 12)


def _masked():
    lab, pb = _synth((48, 40), 4)
    mask = (np.random.default_rng(3).random(lab.shape) > 0.15).astype(np.uint32)
    mask[:, :3] = 0
    return lab, pb, mask


def _const():
    lab, pb = hub_image(None, 8)
    return lab, np.full(pb.shape, 0.5, np.float32)


CASES = {
    "hub8": lambda: hub_image(None, 8), "hub10": lambda: hub_image(None, 10), "hub8_4levels": lambda: hub_image(4, 8),
    "hub8_constant": _const, "thin_hub8": lambda: thin_hub_image(8),
    "fragile_comb40": lambda: fragile_comb_image(40), "fragile_comb36_split3": lambda: fragile_comb_image(36, ysplit=3),
    "touching_comb3x4": lambda: touching_comb_image(3, 4, 5, 4),
    "synth64x64_S4": lambda: _synth((64, 64), 4), "synth96x96_S8": lambda: _synth((96, 96), 8), "synth48x40_S4": lambda: _synth((48, 40), 4),
    "synth72x72_S4": lambda: _synth((72, 72), 4), "synth24x24x24_S6": lambda: _synth((24, 24, 24), 6), "masked48x40_S4": _masked,
}
_cache = {}


def _case(name):
    """(labels, image, mask, the oracle's order, its saliencies), computed once"""
    if name not in _cache:
        from oracle import pyoracle as O
        c = CASES[name]()
        lab, pb, mask = c if len(c) == 3 else (c[0], c[1], None)
        assert (pb * 256 == np.round(pb * 256)).all(), "Q8: sums are exact, saliencies comparable bit for bit"
        cfg = O.make_cfg(pb, rb=[(pb, 8, 0.0, 1.0)])
        assert _featdef.column_names(lab.ndim, 3, [8], [], [8])[STUB] == "x0.b0.mean"
        o, s = O.Rag(lab, mask=mask).merge_order_bc(cfg, None, stub_index=STUB)
        _cache[name] = (lab, pb, mask, o, s)
    return _cache[name]


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", list(CASES))
def test_generate_and_check_agree_with_the_oracle(name):
    lab, pb, mask, o, s = _case(name)
    assert len(o) > 0
    go, gs = _loopdef.generate(lab, pb, mask)
    assert go.shape == o.shape and (go == o).all()
    assert (_bits(gs) == _bits(s)).all()
    assert _loopdef.check(lab, pb, o, s, mask, explain=True) == (-1, "")


def test_the_cases_are_what_they_are_meant_to_be():
    # few levels and a constant image: the insertion order decides (most of) the order
    _, _, _, o, s = _case("hub8_4levels")
    assert len(np.unique(s)) * 2 < len(o)
    _, _, _, o, s = _case("hub8_constant")
    assert len(o) == 128 and (s == 0.5).all()
    # the thin hub: only hub <-> left half is mutual, so half of the regions never merge
    lab, pb, _, o, _ = _case("thin_hub8")
    assert len(np.unique(lab)) == 129 and len(o) == 64
    st = _loopdef.stats(lab, pb, order=o)
    assert (st["live0"] + st["live1"] > st["tab0"] + st["tab1"]).all() and st["fragile"].max() >= 1
    # the fragile comb: every Y -> X_i is fragile and nothing else is; the hub takes the 40 X_i first, and W'-Y pops between the V_i,
    # on a chain of 40 of which a quarter to three quarters are alive.  Split in three: each part pops on a chain of 12, part dead
    lab, pb, _, o, s = _case("fragile_comb40")
    rp = _loopdef.Replay(lab, pb)
    assert len(np.unique(lab)) == 82 and len(o) == 81 and rp.fragile.sum() == 40
    assert {rp.pair_keys[i] for i in np.flatnonzero(rp.fragile)} == {(2, 3 + 2 * i) for i in range(40)}
    assert set(o[:40, 0].tolist()) | set(o[:40, 1].tolist()) >= {3 + 2 * i for i in range(40)}, "the X_i go first"
    step, n, alive = _loopdef.chain_at_pop(lab, pb, o, 2)
    print("fragile_comb40: W'-Y pops at step %d of %d, %d of its %d fragile pairs alive" % (step, len(o), alive, n))
    assert n == 40 and 10 <= alive <= 30 and step == 40 + (n - alive)
    assert _loopdef.stats(lab, pb, order=o)["fragile"].max() == 40
    lab, pb, _, o, s = _case("fragile_comb36_split3")
    assert len(np.unique(lab)) == 76 and len(o) == 75
    for y in (2, 3, 4):
        step, n, alive = _loopdef.chain_at_pop(lab, pb, o, y)
        print("fragile_comb36_split3: part %d pops at step %d, %d of %d alive" % (y, step, alive, n))
        assert n == 12 and 0 < alive < 12
    # the touching comb: 12 merges (hub <-> L) among 67 regions, the hub touches every tooth: total = regions + 1 - step
    lab, pb, _, o, _ = _case("touching_comb3x4")
    st = _loopdef.stats(lab, pb, order=o)
    assert len(np.unique(lab)) == 67 and len(o) == 12
    assert (st["len0"] + st["len1"] == 68 - np.arange(12)).all() and (st["new_records"] == 65 - np.arange(12)).all()
    assert st["fragile"].max() == 1 and (st["new_edges"] == 11 - np.arange(12)).all()
    # compact supervoxels: regions touch that are no table neighbours (the restriction to the table matters)
    lab, pb, _, o, _ = _case("synth64x64_S4")
    st = _loopdef.stats(lab, pb, order=o)
    assert (st["new_records"] > st["new_edges"]).any()


@pytest.mark.parametrize("name", ["hub8_4levels", "thin_hub8", "synth48x40_S4", "synth24x24x24_S6", "masked48x40_S4", "fragile_comb40",
                                  "fragile_comb36_split3"])
def test_flat_shared_boundary_rule_equals_get_boundary(name):
    """'alive pairs between the two regions whose target leaf has an alive pair left' against boundaryWith on TRegion objects, for the
    merged pair of every step and for the new region with (a sample of) the regions that touch it"""
    lab, pb, mask, o, _ = _case(name)
    g = _featdef.Geometry(lab, mask, o)
    rp = _loopdef.Replay(lab, pb, mask)
    compared = nonempty = 0
    for i, (a, b, c) in enumerate(o.tolist()):
        r0, r1 = rp.rid(a), rp.rid(b)
        assert rp.boundary_pairs(r0, r1) == set(_featdef.get_boundary(g.regions[a], g.regions[b]))
        r2 = rp.merge(r0, r1)
        _, touching = _loopdef._others(rp.t_lo, rp.t_hi, r2)
        every = name == "thin_hub8" and i % 8 == 0 or name.startswith("fragile_comb") and i % 4 == 0
        for rs in touching.tolist() if every else touching.tolist()[:4]:
            got = rp.boundary_pairs(r2, rs)
            assert got == set(_featdef.get_boundary(g.regions[c], g.regions[rp.key(rs)]))
            compared += 1
            nonempty += bool(got)
    assert compared > 100 and nonempty > 50


def _swap(o, s, i):
    """merges i and i + 1 trade places (the new keys stay where they are)"""
    o, s = o.copy(), s.copy()
    o[[i, i + 1], :2] = o[[i + 1, i], :2]
    s[[i, i + 1]] = s[[i + 1, i]]
    return o, s


def _independent(o, i):
    return o[i, 2] not in o[i + 1, :2]


@pytest.mark.parametrize("name", ["hub8", "thin_hub8", "synth72x72_S4", "synth24x24x24_S6", "masked48x40_S4", "fragile_comb40",
                                  "fragile_comb36_split3", "touching_comb3x4"])
def test_check_names_the_step_of_a_spoiled_order(name):
    lab, pb, mask, o, s = _case(name)
    n = len(o)
    # two adjacent merges swapped: the first of the two now has a smaller saliency than the table's best, or, where the second
    # merges the region the first creates (on the thin hub every merge does), names a region that does not exist yet
    hit = 0
    for i in range(n - 1):
        if _independent(o, i) and s[i] == s[i + 1]:
            continue
        step, why = _loopdef.check(lab, pb, *_swap(o, s, i), mask, explain=True)
        assert step == i and ("greater saliency" if _independent(o, i) else "no edge") in why, (i, step, why)
        hit += 1
        if hit == 8:
            break
    assert hit == 8
    # one saliency moved by one ulp
    for i in (0, n // 2, n - 1):
        for to in (0.0, 2.0):
            s2 = s.copy()
            s2[i] = np.nextafter(s[i], to)
            step, why = _loopdef.check(lab, pb, o, s2, mask, explain=True)
            assert step == i and "recomputed" in why
    # a wrong key, and an order that stops early
    o2 = o.copy()
    o2[n // 2:, 2] += 1
    assert _loopdef.check(lab, pb, o2, s, mask) == n // 2
    assert _loopdef.check(lab, pb, o[:n - 1], s[:n - 1], mask) == n - 1


def test_check_refuses_a_merge_of_regions_that_are_no_table_neighbours():
    # two blobs of different cells: they do not touch
    lab, pb, _, o, s = _case("hub8")
    o2 = o.copy()
    i = 3
    alive = sorted(set(np.unique(lab).tolist()) - set(o[:i, :2].ravel().tolist()) - {1})
    o2[i, :2] = (alive[0], alive[-1])
    step, why = _loopdef.check(lab, pb, o2, s, explain=True)
    assert step == i and "no edge" in why
    # the hub and a right half of the thin image: they touch (the hub points at the half) but the half never points back
    lab, pb, _, o, s = _case("thin_hub8")
    assert lab[1, 2] == 3 and lab[1, 3] == 1
    o2 = o.copy()
    o2[0, :2] = (1, 3)
    step, why = _loopdef.check(lab, pb, o2, s, explain=True)
    assert step == 0 and "no edge" in why
    # a region that was merged away
    o2 = o.copy()
    o2[5, :2] = o[2, :2]
    assert _loopdef.check(lab, pb, o2, s) == 5


def test_check_names_a_tie_taken_in_the_wrong_order():
    """the constant image: every saliency is 0.5, only the insertion order separates the edges -- any other edge of the table in
    place of the last inserted one is named"""
    lab, pb, _, o, s = _case("hub8_constant")
    rp = _loopdef.Replay(lab, pb)
    hit = 0
    for i, (a, b, _) in enumerate(o.tolist()):
        if i % 4 == 0 and len(rp.e_seq) > 1:
            for k in {0, int(np.argsort(rp.e_seq)[-2])}:          # the oldest edge and the runner-up
                assert (rp.e_lo[k], rp.e_hi[k]) != (rp.rid(a), rp.rid(b)) and rp.e_sal[k] == s[i]
                o2 = o.copy()
                o2[i, :2] = (rp.key(int(rp.e_lo[k])), rp.key(int(rp.e_hi[k])))
                step, why = _loopdef.check(lab, pb, o2, s, explain=True)
                assert step == i and "inserted later" in why, (i, step, why)
                hit += 1
        rp.merge(rp.rid(a), rp.rid(b))
    assert hit >= 20


def test_stump_forest_score_is_the_forest_walk():
    """F(mean) against the walk of _rf-style stumps: left (the predicted label) on x <= t"""
    thr = np.array([0.125, 0.25, 0.25, 0.5, 0.75])
    F = _loopdef.stump_forest_score(thr)
    x = np.array([0.0, 0.125, 0.2, 0.25, 0.3, 0.5, 0.75, 0.9])
    want = [sum(1 for t in thr if v <= t) / 5.0 for v in x]
    assert F(x).tolist() == want
    # as a scorer of the loop: saliencies are multiples of 1 / trees; check() accepts what generate() made and refuses it under
    # the stub's rule
    lab, pb, _, _, _ = _case("hub8")
    F = _loopdef.stump_forest_score(np.linspace(0.3, 0.7, 15))
    o, s = _loopdef.generate(lab, pb, F=F)
    assert np.abs(s * 15 - np.round(s * 15)).max() < 1e-12 and 3 < len(np.unique(s)) <= 16
    assert _loopdef.check(lab, pb, o, s, F=F) == -1
    assert _loopdef.check(lab, pb, o, s) == 0
