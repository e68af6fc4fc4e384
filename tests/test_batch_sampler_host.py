"""The batch samplers of DESIGN 3.17 alone (glia_hmt_batch_plan: glia_amd/csrc/mlp_batch.hpp) against the second author
tests/_batchdef.py, index for index: the wrap into the head of the old permutation, the class sampler's reshuffle of one class, the
choice of sampler, the errors.  No GPU."""
import numpy as np
import pytest

import _batchdef as B


def _hmt():
    from glia_amd import hmt
    return hmt


def _both(labels, n_paths, k, **kw):
    """the library's and the second author's next k draws, asserted equal"""
    got = _hmt().batch_plan(labels, n_paths, k, **kw)
    want = B.plan(labels, n_paths, k, **kw)
    assert [a.tolist() for a in got[0]] == want[0]
    assert [a.tolist() for a in got[1]] == want[1]
    assert got[2] == want[2]
    return want


ONES = np.ones(10, np.int32)


def test_uniform_wraps_into_the_head_of_the_old_permutation():
    """N = 10, B = 3: the fourth batch is the last entry of permutation 0 and then its FIRST two; it ends the epoch; the fifth is from permutation 1"""
    sup, _, end = _both(ONES, 0, 6, sup_batch_size=3, seed=7)
    p0, p1 = B.perm(7, 1, 0, range(10)), B.perm(7, 1, 1, range(10))
    assert sup[0] + sup[1] + sup[2] == p0[:9]
    assert sup[3] == [p0[9], p0[0], p0[1]]
    assert end == [False, False, False, True, False, False]
    assert sup[4] == p1[:3] and sup[5] == p1[3:6]


def test_uniform_batch_of_everything_and_of_one():
    sup, _, end = _both(ONES, 0, 3, sup_batch_size=10, seed=1)
    assert end == [True] * 3 and [sorted(b) for b in sup] == [list(range(10))] * 3
    assert [sup[i] for i in range(3)] == [B.perm(1, 1, i, range(10)) for i in range(3)]
    sup, _, end = _both(ONES, 0, 21, sup_batch_size=1, seed=2)
    assert [i for i, e in enumerate(end) if e] == [9, 19]
    assert sorted(b[0] for b in sup[:10]) == list(range(10)) == sorted(b[0] for b in sup[10:20])


def test_paths_are_stream_0_and_rows_stream_1():
    sup, uns, end = _both(ONES, 12, 5, sup_batch_size=4, uns_batch_size=5, seed=3)
    assert uns[0] == B.perm(3, 0, 0, range(12))[:5] and sup[0] == B.perm(3, 1, 0, range(10))[:4]
    # either sampler ends the epoch: the rows after 3 draws (10 / 4), the paths after 3 (12 / 5)
    assert end[2] and not end[0] and not end[1]
    sup, uns, end = _both(ONES, 12, 4, uns_batch_size=6, seed=3)
    assert sup == [[]] * 4 and end == [False, True, False, True]


def test_class_sampler_reshuffles_one_class_alone():
    """7 positive and 13 negative rows, B = 6: three of each per batch.  The positive class wraps in batch 3 (index 2) and is reshuffled
    alone; the epoch ends when the negative class has wrapped too, in batch 5; then both start again"""
    labels = np.array([1, -1, -1] * 6 + [1, -1], np.int32)
    pos = [r for r in range(20) if labels[r] == 1]
    neg = [r for r in range(20) if labels[r] != 1]
    assert len(pos) == 7 and len(neg) == 13
    sup, _, end = _both(labels, 0, 7, sup_batch_size=6, balance_sup_batch=1, seed=4)
    pp = [B.perm(4, 2, s, pos) for s in range(4)]
    nn = [B.perm(4, 3, s, neg) for s in range(3)]
    assert [b[:3] for b in sup[:2]] == [pp[0][:3], pp[0][3:6]]
    assert sup[2][:3] == [pp[0][6], pp[0][0], pp[0][1]]            # the head of the OLD permutation
    # reshuffled alone after its share: permutation 1, read on from where the wrapped batch stopped (sampler.hxx:203-215 keeps curIndex)
    assert sup[3][:3] == pp[1][2:5] and sup[4][:3] == [pp[1][5], pp[1][6], pp[1][0]]
    assert [b[3:] for b in sup[:4]] == [nn[0][0:3], nn[0][3:6], nn[0][6:9], nn[0][9:12]]
    assert sup[4][3:] == [nn[0][12], nn[0][0], nn[0][1]]
    assert end == [False, False, False, False, True, False, False]
    # batch 5 wrapped both classes -- each reshuffled alone (positive: 2, negative: 1) -- and ended the epoch: the reset shuffles both
    # again and starts them at 0
    assert sup[5] == pp[3][:3] + nn[2][:3]


def test_balance_without_a_batch_size_takes_the_minority_from_both():
    labels = np.array([1, -1, -1] * 6 + [1, -1], np.int32)
    sup, _, end = _both(labels, 0, 3, balance_sup_batch=1, seed=5)
    assert all(len(b) == 14 for b in sup)
    # classes in ascending target: the positive target 0.05 first
    assert all(labels[r] == 1 for r in sup[0][:7]) and all(labels[r] == -1 for r in sup[0][7:])
    assert end[0] is False and end[1] is True                        # 13 negative rows: the second batch wraps them
    flipped, _, _ = _both(labels, 0, 3, balance_sup_batch=1, seed=5, pos_target=0.9, neg_target=0.1)
    assert all(labels[r] == -1 for r in flipped[0][:7]) and all(labels[r] == 1 for r in flipped[0][7:])
    # with a batch size the positive class comes first whatever the targets
    first, _, _ = _both(labels, 0, 1, sup_batch_size=5, balance_sup_batch=1, seed=5, pos_target=0.9, neg_target=0.1)
    assert [labels[r] for r in first[0]] == [1, 1, -1, -1, -1]


def test_permutations_and_seeds():
    for n in (1, 2, 3, 64, 65, 1000):
        for s in range(3):
            assert sorted(B.perm(9, 1, s, range(n))) == list(range(n))
    a, _, _ = _both(np.ones(50, np.int32), 0, 4, sup_batch_size=50, seed=1)
    b, _, _ = _both(np.ones(50, np.int32), 0, 4, sup_batch_size=50, seed=2)
    c, _, _ = _both(np.ones(50, np.int32), 0, 4, sup_batch_size=50, seed=1)
    assert a == c and a != b and all(sorted(x) == list(range(50)) for x in a + b)
    assert len({tuple(x) for x in a}) == 4                           # every reshuffle is another permutation
    _both(np.ones(50, np.int32), 0, 2, sup_batch_size=7, seed=(1 << 64) - 1)


@pytest.mark.parametrize("kw, n_paths, text", [
    (dict(sup_batch_size=11), 0, "Error: totalSize must be greater than batchSize"),
    (dict(uns_batch_size=5), 4, "Error: totalSize must be greater than batchSize"),
    (dict(sup_batch_size=4, balance_sup_batch=1), 0, "has no row"),
    (dict(balance_sup_batch=1), 0, "has no row"),
    (dict(balance_sup_batch=1, pos_target=0.5, neg_target=0.5), 0, "one class"),
])
def test_errors_are_arg_errors_with_a_message(kw, n_paths, text):
    hmt = _hmt()
    with pytest.raises(hmt.HmtError) as e:
        hmt.batch_plan(ONES, n_paths, 2, **kw)
    assert e.value.code == hmt.ERR_ARG and text in str(e.value)
    with pytest.raises(ValueError):
        B.plan(ONES, n_paths, 2, **kw)


def test_a_class_with_fewer_rows_than_its_share_is_refused():
    hmt = _hmt()
    labels = np.array([1, 1, -1, -1, -1, -1, -1, -1], np.int32)
    with pytest.raises(hmt.HmtError) as e:
        hmt.batch_plan(labels, 0, 1, sup_batch_size=6, balance_sup_batch=1)      # three of two positive rows
    assert e.value.code == hmt.ERR_ARG and "class 0 has 2 rows, fewer than its share" in str(e.value)
    with pytest.raises(ValueError):
        B.plan(labels, 0, 1, sup_batch_size=6, balance_sup_batch=1)
    _both(labels, 0, 3, sup_batch_size=4, balance_sup_batch=1)                   # two of two: every batch wraps the class
    with pytest.raises(hmt.HmtError) as e:
        hmt.batch_plan(np.array([1, 0], np.int32), 0, 1, sup_batch_size=1)
    assert "neither +1 nor -1" in str(e.value)
