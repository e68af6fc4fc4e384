"""-m gpu: Context.label_overlap (glia_hmt_label_overlap, glia_amd/csrc/label_overlap.hip) against np.unique on the stacked label
pairs -- exact entries in exact order -- and Context.evaluate (glia_hmt_eval) against the plain-Python restatement of
tests/_eval_cases.py with the tolerances of test_eval_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import _eval_cases as E
from test_gpu_bc_label import truth_cells

pytestmark = pytest.mark.gpu
FF = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    c.close()


def _dev(a, offset=0):
    """the array on the device; offset = 1: as a view one element into a larger buffer, so not 16-byte aligned"""
    import torch
    a = np.array(a, dtype=np.uint32, order="C")              # a copy: shared inputs stay as they are
    if not offset:
        return torch.from_numpy(a.view(np.int32)).cuda()
    buf = torch.zeros(a.size + offset, dtype=torch.int32, device="cuda")
    view = buf[offset:].view(a.shape)
    view.copy_(torch.from_numpy(a.view(np.int32)))
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def _expected(a, b, mask=None, drop_a=False, drop_b=False):
    from glia_amd import hmt
    a, b = np.asarray(a, np.uint32).reshape(-1), np.asarray(b, np.uint32).reshape(-1)
    keep = np.ones(a.size, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    if drop_a:
        keep &= a != 0
    if drop_b:
        keep &= b != 0
    out = np.empty(0, hmt.OVERLAP_ENTRY)
    if keep.any():
        u, c = np.unique(np.stack([a[keep], b[keep]], axis=1), axis=0, return_counts=True)      # rows ascend by (a, b)
        out = np.empty(len(u), hmt.OVERLAP_ENTRY)
        out["a"], out["b"], out["count"] = u[:, 0], u[:, 1], c
    return out


def _check(ctx, a, b, mask=None, drop_a=False, drop_b=False, offset=0):
    got = ctx.label_overlap(_dev(a, offset), _dev(b, offset), None if mask is None else _dev(mask, offset), drop_zero_a=drop_a, drop_zero_b=drop_b)
    want = _expected(a, b, mask, drop_a, drop_b)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes()
    return got


def _labels(rng, shape, n_a=6, n_b=5):
    return rng.integers(0, n_a, size=shape).astype(np.uint32), rng.integers(0, n_b, size=shape).astype(np.uint32)


# 1 .. 5: below, at and above one 16-byte word; 1023 .. 1025: around one step of a workgroup (1024 voxels); 4096 + 17: two groups
# of steps and a tail; 5 * 4096 + 17: two workgroups (16 steps each), the second with an odd number of steps
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 4096 + 17, 5 * 4096 + 17])
@pytest.mark.parametrize("offset", [0, 1])
def test_stream_lengths_aligned_and_not(ctx, n, offset):
    a, b = _labels(np.random.default_rng(n), n)
    m = (np.random.default_rng(n + 1).random(n) > 0.3).astype(np.uint32) * 5
    _check(ctx, a, b, offset=offset)
    _check(ctx, a, b, mask=m, offset=offset)


@pytest.mark.parametrize("shape", [(33, 31), (17, 19, 23)])
def test_2d_and_3d_are_the_same_call(ctx, shape):
    a, b = _labels(np.random.default_rng(len(shape)), shape, 40, 30)
    got = _check(ctx, a, b)
    assert got.tobytes() == ctx.label_overlap(_dev(a.reshape(-1)), _dev(b.reshape(-1))).tobytes()


def test_one_unaligned_pointer_is_enough_for_the_scalar_path(ctx):
    a, b = _labels(np.random.default_rng(3), 3000)
    want = _expected(a, b)
    assert ctx.label_overlap(_dev(a, 1), _dev(b)).tobytes() == want.tobytes()
    assert ctx.label_overlap(_dev(a), _dev(b, 1)).tobytes() == want.tobytes()
    m = np.ones(3000, np.uint32)
    assert ctx.label_overlap(_dev(a), _dev(b), _dev(m, 1)).tobytes() == want.tobytes()


@pytest.mark.parametrize("offset", [0, 1])
def test_label_ffffffff_on_both_sides_and_on_one(ctx, offset):
    """the key of (0xFFFFFFFF, 0xFFFFFFFF) is the tables' empty-slot marker: it is counted apart and sorts last"""
    rng = np.random.default_rng(9)
    a, b = _labels(rng, 5000)
    both = rng.random(5000) < 0.2
    a[both], b[both] = FF, FF
    only_a, only_b = rng.random(5000) < 0.1, rng.random(5000) < 0.1
    a[only_a & ~both] = FF
    b[only_b & ~both] = FF
    b[only_a & ~both & (b == FF)] = 1
    got = _check(ctx, a, b, offset=offset)
    assert (got["a"][-1], got["b"][-1], got["count"][-1]) == (FF, FF, int(both.sum()))
    assert ((got["a"] == FF) & (got["b"] != FF)).any() and ((got["a"] != FF) & (got["b"] == FF)).any()
    _check(ctx, np.full(777, FF, np.uint32), np.full(777, FF, np.uint32), offset=offset)       # nothing but the reserved pair
    _check(ctx, a, b, mask=(~both).astype(np.uint32), offset=offset)                         # ... and a mask that removes all of it


def test_all_pairs_distinct_overflow_the_lds_table_and_repeat_the_global_pass(ctx):
    from glia_amd import hmt
    n = 20000
    a = np.random.default_rng(4).permutation(n).astype(np.uint32) * np.uint32(211)
    b = np.arange(n, dtype=np.uint32) * np.uint32(3) + np.uint32(1)
    got = _check(ctx, a, b)
    assert len(got) == n and (got["count"] == 1).all()
    assert ctx.last_eval_timing()["repeats"] == 0 and ctx.last_eval_timing()["entries"] == n
    with hmt.options(GLIA_HMT_MINCAP=1):
        again = _check(ctx, a, b)
        assert ctx.last_eval_timing()["repeats"] >= 1          # 1024 slots cannot hold 20 000 keys: the pass was repeated
    assert again.tobytes() == got.tobytes()


def test_one_pair_for_the_whole_volume(ctx):
    n = 300000
    got = _check(ctx, np.full(n, 7, np.uint32), np.full(n, 9, np.uint32))
    assert len(got) == 1 and got["count"][0] == n


def test_masks_none_random_all_out(ctx):
    rng = np.random.default_rng(6)
    a, b = _labels(rng, (21, 20, 19), 50, 40)
    _check(ctx, a, b)
    _check(ctx, a, b, mask=rng.integers(0, 3, size=a.shape).astype(np.uint32))
    assert len(_check(ctx, a, b, mask=np.zeros(a.shape, np.uint32))) == 0


@pytest.mark.parametrize("drop_a", [False, True])
@pytest.mark.parametrize("drop_b", [False, True])
def test_drop_flags(ctx, drop_a, drop_b):
    rng = np.random.default_rng(7)
    a, b = _labels(rng, 6001, 4, 3)
    got = _check(ctx, a, b, drop_a=drop_a, drop_b=drop_b)
    assert (got["a"] == 0).any() != drop_a and (got["b"] == 0).any() != drop_b
    _check(ctx, a, b, mask=rng.integers(0, 2, size=6001).astype(np.uint32), drop_a=drop_a, drop_b=drop_b)
    assert len(_check(ctx, np.zeros(100, np.uint32), b[:100], drop_a=True)) == 0


@functools.lru_cache(maxsize=None)
def _cells64():
    t = truth_cells((64, 64, 64), 16)
    t.setflags(write=False)
    return t


def test_two_calls_return_identical_bytes_on_several_workgroups(ctx):
    labels, _ = ctx.synth((64, 64, 64), 8, 16)
    d_truth = _dev(_cells64())
    first = ctx.label_overlap(labels, d_truth)
    for _ in range(3):
        assert ctx.label_overlap(labels, d_truth).tobytes() == first.tobytes()
    assert first.tobytes() == _expected(labels.cpu().numpy().view(np.uint32), _cells64()).tobytes()


def test_capacity_one_short_reports_the_number_needed(ctx):
    from glia_amd import hmt
    a, b = _labels(np.random.default_rng(10), 4000, 9, 8)
    want = _expected(a, b)
    da, db = _dev(a), _dev(b)
    L, n = hmt.lib(), C.c_int64(-1)
    buf = np.zeros(len(want), hmt.OVERLAP_ENTRY)
    args = (ctx.h, C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()), None, C.c_int64(a.size), C.c_int(0), buf.ctypes.data_as(C.c_void_p))
    assert L.glia_hmt_label_overlap(*args, C.c_int64(len(want) - 1), C.byref(n)) == hmt.ERR_CAPACITY
    assert n.value == len(want) and not buf.view(np.uint8).any()              # the number needed; the buffer untouched
    assert L.glia_hmt_label_overlap(*args, C.c_int64(len(want)), C.byref(n)) == 0
    assert n.value == len(want) and buf.tobytes() == want.tobytes()
    # bad arguments are refused before the device is touched
    for bad in ((ctx.h, None, C.c_void_p(db.data_ptr()), None, C.c_int64(a.size), C.c_int(0), None, C.c_int64(0), C.byref(n)),
                (ctx.h, C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()), None, C.c_int64(0), C.c_int(0), None, C.c_int64(0), C.byref(n)),
                (ctx.h, C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()), None, C.c_int64(2 ** 32 - 1), C.c_int(0), None, C.c_int64(0), C.byref(n)),
                (ctx.h, C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()), None, C.c_int64(a.size), C.c_int(4), None, C.c_int64(0), C.byref(n)),
                (ctx.h, C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()), None, C.c_int64(a.size), C.c_int(0), None, C.c_int64(5), C.byref(n)),
                (ctx.h, C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()), None, C.c_int64(a.size), C.c_int(0), None, C.c_int64(0), None)):
        assert L.glia_hmt_label_overlap(*bad) == hmt.ERR_ARG and L.glia_hmt_last_error().decode().startswith("label_overlap: ")


# ---- Context.evaluate against the restatement ----
def _np32(t):
    return t.cpu().numpy().view(np.uint32)


def _same(x, y):
    return x.keys() == y.keys() and all(E.same_float(x[k], y[k]) if isinstance(x[k], float) else x[k] == y[k] for k in x)


def _check_eval(ctx, res, ref, masks=None):
    """res / ref / masks: lists of device tensors (masks may hold None)"""
    from glia_amd import hmt
    host = lambda ts: [None if t is None else _np32(t) for t in ts]
    cmaps = [E.contingency(p, r, m) for p, r, m in zip(host(res), host(ref), host(masks) if masks is not None else [None] * len(res))]
    assert all(len(c) <= 4096 for c in cmaps)                   # the entropy tolerance of _eval_cases.check_against is for E <= 4096
    for mode in ("reference", "exact"):
        got = ctx.evaluate(res, ref, masks, vi_mode=mode)
        assert all(type(got[k]) is int for k in ("TP", "TN", "FP", "FN"))
        E.check_against(got, E.scores(cmaps, mode))
        tables = [ctx.label_overlap(p, r, m, drop_zero_b=True) for p, r, m in zip(res, ref, masks if masks is not None else [None] * len(res))]
        assert _same(hmt.overlap_scores(tables, vi_mode=mode), got)     # evaluate = the tables with "drop b == 0", then the host half
    return got


def test_evaluate_synth_labels_against_truth_cells(ctx):
    labels, _ = ctx.synth((64, 64, 64), 8, 16)
    got = _check_eval(ctx, [labels], [_dev(_cells64())])
    assert got["TP"] > 0 and got["FP"] >= 0 and 0.0 < got["rand_index"] < 1.0
    single = ctx.evaluate(labels, _dev(_cells64()), vi_mode="exact")       # single volumes instead of lists
    assert _same(single, got)                                              # (got is the last mode _check_eval ran: "exact")


def test_evaluate_components_of_thresholded_pb_with_a_mask(ctx):
    import torch
    _, pb = ctx.synth((64, 64, 64), 8, 16)
    comp, n = ctx.label_components((pb > 0.5).to(torch.int32).contiguous(), mode="binary_inverted")
    assert n >= 1
    mask = _dev((np.random.default_rng(2).random((64, 64, 64)) > 0.2).astype(np.uint32) * 3)
    _check_eval(ctx, [comp], [_dev(_cells64())], [mask])
    _check_eval(ctx, [comp], [_dev(_cells64())])


def test_evaluate_three_2d_pairs(ctx):
    rng = np.random.default_rng(13)
    shapes = [(33, 31), (40, 17), (5, 64)]
    res = [_dev(rng.integers(0, 9, size=s)) for s in shapes]
    ref = [_dev(rng.integers(0, 7, size=s)) for s in shapes]
    masks = [None, _dev(rng.integers(0, 2, size=shapes[1])), None]
    _check_eval(ctx, res, ref, masks)
    _check_eval(ctx, res, ref)


def test_evaluate_bad_arguments(ctx):
    from glia_amd import hmt
    a = _dev(np.ones(10, np.uint32))
    with pytest.raises(KeyError):
        ctx.evaluate(a, a, vi_mode="textbook")
    L, out = hmt.lib(), hmt.EvalResult()
    ptr, nv = (C.c_void_p * 1)(a.data_ptr()), (C.c_int64 * 1)(10)
    for args in ((ctx.h, C.c_int(0), ptr, ptr, None, nv, C.c_int(0), C.byref(out)), (ctx.h, C.c_int(1), ptr, ptr, None, nv, C.c_int(7), C.byref(out)),
                 (ctx.h, C.c_int(1), ptr, None, None, nv, C.c_int(0), C.byref(out)), (ctx.h, C.c_int(1), ptr, ptr, None, (C.c_int64 * 1)(0), C.c_int(0), C.byref(out)),
                 (ctx.h, C.c_int(1), (C.c_void_p * 1)(None), ptr, None, nv, C.c_int(0), C.byref(out))):
        assert L.glia_hmt_eval(*args) == hmt.ERR_ARG and L.glia_hmt_last_error().decode().startswith("eval: ")
