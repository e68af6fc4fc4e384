"""The semi-supervised chain end to end on two 32^3 synthetic volumes, inputs built as tests/test_gpu_mlp_train_chain.py builds them:
merge_order_pb -> bc_feat_batch -> (the labelled volume: bc_label) -> rows_minmax over both -> train_sshmt with both terms (10 + 10,
vanilla with the adaptive step, 2 rounds of 5 iterations) -> model.mlp(ctx) -> RegionMap.merge_order_bc.  The trained classifier's order
passes check_merge_order, the trace's fx never rises, and the model is not the one train_mlp gives on the labelled volume alone."""
import numpy as np
import pytest

import _mlpdef


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    assert c.libm_exp() != 0, "host exp not pinned"
    yield c
    c.close()


def _dense(order, labels):
    """keys -> dense ids: leaf i = i-th label ascending, merged key maxKey + 1 + k -> R + k"""
    lab = np.unique(labels)
    R, top = len(lab), int(lab.max())
    o = order.astype(np.int64)
    return np.where(o > top, o - (top + 1) + R, np.searchsorted(lab, np.minimum(o, top))).astype(np.uint32), R


def _volume(ctx, seed):
    import torch
    from glia_amd import hmt
    from oracle import pyoracle as O
    labels, pb = O.synth((32,) * 3, 8, 16, seed=seed)
    d_lab, d_pb = torch.from_numpy(labels.view(np.int32)).cuda(), torch.from_numpy(pb).cuda()
    rm = hmt.RegionMap(ctx, d_lab, pb=d_pb, cfg=hmt.make_config(d_pb, rb=[(d_pb, 8, 0.0, 1.0)]))
    assert rm.num_regions == 64
    order, _ = rm.merge_order_pb(type=2)
    assert len(order) == 63
    return rm, labels, order, rm.bc_feat_batch(order)


@pytest.mark.gpu
def test_chain_from_pb_orders_to_a_semi_supervised_classifiers_order(ctx):
    import torch
    from glia_amd import hmt
    before = hmt.Context.internal_errors()
    rm, labels, order, rows = _volume(ctx, 0x9E3779B97F4A7C15)          # the labelled volume
    rm_u, labels_u, order_u, rows_u = _volume(ctx, 12345)                       # the unlabelled one
    assert not np.array_equal(rows, rows_u)
    z, y, x = np.meshgrid(*[np.arange(32)] * 3, indexing="ij")
    truth = ((z // 16) * 4 + (y // 16) * 2 + x // 16 + 1).astype(np.uint32)
    lab = rm.bc_label(torch.from_numpy(truth.view(np.int32)).cuda(), order)
    assert set(lab.tolist()) == {1, -1}
    mn, mx = hmt.rows_minmax([rows, rows_u])
    paths = hmt.merge_paths(order_u)
    assert len(paths) > 30 and all(2 <= len(p) <= 3 for p in paths)
    opts = dict(ws=1.0, wr=1e-4, sigma_s=0.5, optimizer=1, step=0.5, step_decay=0.5, max_iterations=5, n_sigma_updates=2)
    uopts = dict(opts, wu=1.0, sigma_u=0.5)
    model = hmt.train_sshmt(ctx, rows, lab, [(rows_u, order_u)], 10, 10, minmax=(mn, mx), **uopts)
    assert model.rounds == 2 and not model.stopped_nonfinite and model.n_used_rows == 63
    assert model.n_paths == len(paths) and model.n_uns_rows == 63
    it = model.trace[model.trace["kind"] == 0]
    assert len(it) == 10
    for rnd in (0, 1):      # the adaptive step accepts no higher energy: within a round fx never rises
        fx = model.trace["fx"][(model.trace["round"] == rnd) & (model.trace["kind"] <= 1)]
        assert len(fx) == 6 and (np.diff(fx) <= 0).all() and fx[-1] < fx[0]
    host = hmt.train_sshmt_host(rows, lab, [(rows_u, order_u)], 10, 10, minmax=(mn, mx), **uopts)
    assert model.trace.tobytes() == host.trace.tobytes() and model.weights().tobytes() == host.weights().tobytes()
    sup = hmt.train_mlp(ctx, rows, lab, 10, 10, minmax=(mn, mx), **opts)
    assert sup.weights().shape == model.weights().shape and not _mlpdef.same(sup.weights(), model.weights())
    clf = model.mlp(ctx)
    assert clf.dim == rm.feat_dim() == rows.shape[1]
    o, s, f = rm_u.merge_order_bc(clf, want_feats=True)
    assert len(o) == 63
    d, R = _dense(o, labels_u)
    assert R == 64 and hmt.check_merge_order(d, R) == -1
    pred, _ = hmt.mlp_predict_host(model.weights(), 10, 10, f, mn, mx)
    assert _mlpdef.same(s, pred)
    clf.close(); rm.close(); rm_u.close(); model.close(); host.close(); sup.close()
    assert hmt.Context.internal_errors() == before == 0
