"""The host half of eval_ri / eval_vi (glia_hmt_overlap_scores, glia_amd/csrc/eval.cpp) against known answers and against the
plain-Python restatement of tests/_eval_cases.py.  Needs no GPU: the tables are built here."""
import ctypes as C
import math

import numpy as np
import pytest

import _eval_cases as E
from glia_amd import hmt


def _scores(cmaps, mode="reference"):
    return hmt.overlap_scores([E.entries(c) for c in cmaps], vi_mode=mode)


def test_known_answer_one_proposed_label():
    """(a): res = 1 everywhere, ref = 1 1 1 1 2 2 3 3.  Every quotient is a power of two, so both modes are exact."""
    cmap = E.contingency([1] * 8, [1, 1, 1, 1, 2, 2, 3, 3])
    assert cmap == {(1, 1): 4, (1, 2): 2, (1, 3): 2}
    for mode in ("reference", "exact"):
        s = _scores([cmap], mode)
        assert (s["TP"], s["TN"], s["FP"], s["FN"]) == (8, 0, 20, 0)
        assert s["precision"] == 8.0 / 28.0 and s["recall"] == 1.0
        assert s["f1"] == 2.0 * (8.0 / 28.0) * 1.0 / (8.0 / 28.0 + 1.0)
        assert abs((1.0 - s["f1"]) - 5.0 / 9.0) < 1e-15
        assert s["rand_index"] == 8.0 / 28.0
        assert s["false_split"] == 0.0 and s["false_merge"] == 1.5


def test_known_answer_integer_quotient():
    """(b): res = 1 1 1, ref = 1 1 2.  n_a / c = 3 / 2: the reference divides two uints (util/image_stats.hxx:153), so its term is log2 1."""
    cmap = E.contingency([1, 1, 1], [1, 1, 2])
    ref, exact = _scores([cmap], "reference"), _scores([cmap], "exact")
    assert E.close(ref["false_merge"], math.log2(3.0) / 3.0, 1e-15)
    assert E.close(exact["false_merge"], (2.0 * math.log2(1.5) + math.log2(3.0)) / 3.0, 1e-15)
    assert ref["false_merge"] < exact["false_merge"]
    assert ref["false_split"] == 0.0 and exact["false_split"] == 0.0
    assert all(ref[k] == exact[k] for k in ("TP", "TN", "FP", "FN", "precision", "recall", "f1", "rand_index"))


def test_known_answer_identical_volumes():
    """(c): error 0, Rand index 1, VI 0"""
    vol = np.random.default_rng(5).integers(1, 9, size=(7, 11, 13))
    for mode in ("reference", "exact"):
        s = _scores([E.contingency(vol, vol)], mode)
        assert s["TP"] > 0 and s["FP"] == 0 and s["FN"] == 0
        assert 1.0 - s["f1"] == 0.0 and s["rand_index"] == 1.0
        assert s["false_split"] == 0.0 and s["false_merge"] == 0.0


def test_empty_selection_is_what_the_reference_returns():
    """(d): no voxel selected -- 0 / 0 = NaN for the entropies and f1, 0 for precision and recall, 0 / FEPS = 0 for the Rand index"""
    for tables in ([np.empty(0, hmt.OVERLAP_ENTRY)], [np.empty(0, hmt.OVERLAP_ENTRY)] * 3):
        s = hmt.overlap_scores(tables)
        assert (s["TP"], s["TN"], s["FP"], s["FN"]) == (0, 0, 0, 0)
        assert math.isnan(s["false_split"]) and math.isnan(s["false_merge"]) and math.isnan(s["f1"])
        assert s["precision"] == 0.0 and s["recall"] == 0.0 and s["rand_index"] == 0.0
    E.check_against(hmt.overlap_scores([np.empty(0, hmt.OVERLAP_ENTRY)]), E.scores([{}]))


def test_counts_are_summed_before_the_ratios_and_entropies_averaged():
    """(e): two image pairs"""
    rng = np.random.default_rng(8)
    pairs = [(rng.integers(0, 5, size=300), rng.integers(0, 4, size=300)), (rng.integers(0, 3, size=(9, 8)), rng.integers(0, 9, size=(9, 8)))]
    cmaps = [E.contingency(p, r) for p, r in pairs]
    for mode in ("reference", "exact"):
        both, one, two = _scores(cmaps, mode), _scores(cmaps[:1], mode), _scores(cmaps[1:], mode)
        for k in ("TP", "TN", "FP", "FN"):
            assert both[k] == one[k] + two[k]
        assert both["precision"] == float(both["TP"]) / float(both["TP"] + both["FP"])
        assert both["precision"] != (one["precision"] + two["precision"]) / 2.0
        assert both["recall"] == float(both["TP"]) / float(both["TP"] + both["FN"])
        for k in ("false_split", "false_merge"):
            assert both[k] == (0.0 + one[k] + two[k]) / 2.0          # stats::mean: the sum starts from 0.0, in image order
        E.check_against(both, E.scores(cmaps, mode))


def test_pair_counts_beyond_64_bits():
    """(f): entries of 2^33 voxels -- c (c - 1) / 2 alone is about 2^65; the lo / hi words carry the 128-bit counts"""
    c = 2 ** 33
    cmaps = [{(1, 1): c, (2, 2): c, (1, 2): c}, {(7, 7): c}, {(1, 5): c, (2, 5): c + 3}]
    want = E.scores(cmaps)
    assert want["TP"] > 2 ** 64 and want["FP"] > 2 ** 64 and want["FN"] > 2 ** 64 and want["TN"] > 2 ** 64
    got = _scores(cmaps)
    E.check_against(got, want)
    tabs = [E.entries(m) for m in cmaps]
    raw = hmt.EvalResult()
    ptrs = (C.c_void_p * 3)(*[t.ctypes.data for t in tabs])
    lens = (C.c_int64 * 3)(*[len(t) for t in tabs])
    assert hmt.lib().glia_hmt_overlap_scores(ptrs, lens, C.c_int(3), C.c_int(0), C.byref(raw)) == 0
    for k in ("tp", "tn", "fp", "fn"):
        assert getattr(raw, k + "_hi") == want[k.upper()] >> 64 and getattr(raw, k + "_hi") > 0
        assert getattr(raw, k + "_lo") == want[k.upper()] & (2 ** 64 - 1)


def _random_cmap(rng, n_entries, n_a, n_b, max_count):
    cmap = {}
    while len(cmap) < n_entries:
        a, b = int(rng.integers(0, n_a)), int(rng.integers(1, n_b + 1))
        cmap[(a * 7919 % 2 ** 32, b * 104729 % 2 ** 32)] = int(rng.integers(1, max_count + 1))
    return cmap


@pytest.mark.parametrize("seed,n_entries,n_a,n_b,max_count", [
    (1, 1, 1, 1, 1), (2, 17, 5, 5, 3), (3, 300, 40, 25, 1000), (4, 4096, 3000, 2000, 50), (5, 4096, 80, 90, 2 ** 20),
    (6, 2000, 2000, 3, 7), (7, 2000, 3, 2000, 7), (8, 4096, 100, 100, 2 ** 31), (9, 1500, 60, 60, 2 ** 40),
])
def test_random_tables_against_the_restatement(seed, n_entries, n_a, n_b, max_count):
    rng = np.random.default_rng(seed)
    cmaps = [_random_cmap(rng, n_entries, n_a, n_b, max_count)] + ([_random_cmap(rng, max(n_entries // 3, 1), n_a, n_b, max_count)] if seed % 2 else [])
    for mode in ("reference", "exact"):
        E.check_against(_scores(cmaps, mode), E.scores(cmaps, mode))


def test_entries_are_taken_as_given_in_any_order():
    rng = np.random.default_rng(12)
    cmap = _random_cmap(rng, 500, 30, 30, 100)
    tab = E.entries(cmap)
    a, b = hmt.overlap_scores([tab]), hmt.overlap_scores([tab[rng.permutation(len(tab))]])
    for k in ("TP", "TN", "FP", "FN", "precision", "recall", "f1", "rand_index"):
        assert a[k] == b[k]
    assert E.close(a["false_split"], b["false_split"], 1e-12) and E.close(a["false_merge"], b["false_merge"], 1e-12)


def test_bad_arguments_are_status_codes_with_a_message():
    L = hmt.lib()
    tab = E.entries({(1, 1): 2})
    ptr, one, out = (C.c_void_p * 1)(tab.ctypes.data), (C.c_int64 * 1)(1), hmt.EvalResult()
    msg = lambda: L.glia_hmt_last_error().decode()
    assert L.glia_hmt_overlap_scores(ptr, one, C.c_int(1), C.c_int(2), C.byref(out)) == hmt.ERR_ARG and msg().startswith("eval: ")
    assert L.glia_hmt_overlap_scores(ptr, one, C.c_int(0), C.c_int(0), C.byref(out)) == hmt.ERR_ARG and msg().startswith("eval: ")
    assert L.glia_hmt_overlap_scores(None, one, C.c_int(1), C.c_int(0), C.byref(out)) == hmt.ERR_ARG and msg().startswith("eval: ")
    assert L.glia_hmt_overlap_scores(ptr, one, C.c_int(1), C.c_int(0), None) == hmt.ERR_ARG and msg().startswith("eval: ")
    assert L.glia_hmt_overlap_scores(ptr, (C.c_int64 * 1)(-1), C.c_int(1), C.c_int(0), C.byref(out)) == hmt.ERR_ARG and msg().startswith("eval: ")
    zero = E.entries({(1, 1): 2, (1, 2): 0})
    assert L.glia_hmt_overlap_scores((C.c_void_p * 1)(zero.ctypes.data), (C.c_int64 * 1)(2), C.c_int(1), C.c_int(0), C.byref(out)) == hmt.ERR_ARG
    assert msg().startswith("eval: ") and "count 0" in msg()
    # the device entry points refuse a NULL context before anything else, so without a GPU too
    n = C.c_int64(0)
    assert L.glia_hmt_label_overlap(None, None, None, None, C.c_int64(8), C.c_int(0), None, C.c_int64(0), C.byref(n)) == hmt.ERR_ARG
    assert msg().startswith("label_overlap: ")
    assert L.glia_hmt_eval(None, C.c_int(1), None, None, None, None, C.c_int(0), C.byref(out)) == hmt.ERR_ARG and msg().startswith("eval: ")
