"""The MLP chain end to end on a 32^3 synthetic volume, inputs built as tests/test_gpu_bc_mlp.py builds them:
merge_order_pb -> bc_feat_batch -> bc_label -> rows_minmax -> train_mlp (10 + 10, Adam, 2 rounds of 5 iterations) -> model.mlp(ctx) ->
RegionMap.merge_order_bc.  The trained classifier's order passes check_merge_order and its saliencies are the host predictor's values
of the rows the loop returns."""
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


@pytest.mark.gpu
def test_chain_from_a_pb_order_to_a_trained_classifiers_order(ctx):
    import torch
    from glia_amd import hmt
    from oracle import pyoracle as O
    labels, pb = O.synth((32,) * 3, 8, 16)
    d_lab, d_pb = torch.from_numpy(labels.view(np.int32)).cuda(), torch.from_numpy(pb).cuda()
    rm = hmt.RegionMap(ctx, d_lab, pb=d_pb, cfg=hmt.make_config(d_pb, rb=[(d_pb, 8, 0.0, 1.0)]))
    assert rm.num_regions == 64
    before = hmt.Context.internal_errors()
    order, _ = rm.merge_order_pb(type=2)
    assert len(order) == 63
    rows = rm.bc_feat_batch(order)
    # truth: the eight 16^3 octants
    z, y, x = np.meshgrid(*[np.arange(32)] * 3, indexing="ij")
    truth = ((z // 16) * 4 + (y // 16) * 2 + x // 16 + 1).astype(np.uint32)
    lab = rm.bc_label(torch.from_numpy(truth.view(np.int32)).cuda(), order)
    assert set(lab.tolist()) == {1, -1}
    mn, mx = hmt.rows_minmax([rows])
    opts = dict(ws=1.0, wr=1e-4, sigma_s=0.5, optimizer=2, step=0.01, max_iterations=5, n_sigma_updates=2)
    model = hmt.train_mlp(ctx, rows, lab, 10, 10, minmax=(mn, mx), **opts)
    assert model.rounds == 2 and not model.stopped_nonfinite and model.n_used_rows == 63
    assert int((model.trace["kind"] == 0).sum()) == 10
    fx = model.trace["fx"][model.trace["kind"] <= 1]
    assert fx[-1] < fx[0], "ten Adam steps lower the energy"
    host = hmt.train_mlp_host(rows, lab, 10, 10, minmax=(mn, mx), **opts)
    assert model.trace.tobytes() == host.trace.tobytes() and model.weights().tobytes() == host.weights().tobytes()
    clf = model.mlp(ctx)
    assert clf.dim == rm.feat_dim() == rows.shape[1]
    o, s, f = rm.merge_order_bc(clf, want_feats=True)
    assert len(o) == 63
    d, R = _dense(o, labels)
    assert R == 64 and hmt.check_merge_order(d, R) == -1
    pred, _ = hmt.mlp_predict_host(model.weights(), 10, 10, f, mn, mx)
    assert _mlpdef.same(s, pred)
    assert _mlpdef.same(s, _mlpdef.sigmoid(_mlpdef.logits(model.weights(), 10, 10, f, mn, mx)))
    assert len(np.unique(s)) > 8
    clf.close(); rm.close(); model.close(); host.close()
    assert hmt.Context.internal_errors() == before == 0
