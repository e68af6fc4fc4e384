"""train_mlp on the device (glia_amd/csrc/mlp_train.hip) against the definition on the host (glia_hmt_mlp_train_host, itself held to the
second author by tests/test_mlp_train_host.py): weights after every round, the trace and the sigmas bit for bit on every shared case
(tests/_mlptrain_cases.py) -- one row; a chunk short by one, exact and over by one; a last chunk of one row; one unit and 32 units; one
column and 104 columns; logsig; every optimiser and step rule; dropped rows; dead units; a saturated sigmoid; the divergent step.  Where
the context could not pin the host's exp (glia_hmt_ctx_libm_exp reports 0) the device's sigmoid is its own libm's and the comparison is
to 1e-9 relative instead."""
import numpy as np
import pytest

import _mlpdef
import _mlptrain_cases as K
import _mlptraindef as T


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    c.close()


def _train(ctx, kw, host=False):
    from glia_amd import hmt
    return hmt.train_mlp(None if host else ctx, kw["rows"], kw["labels"], kw["n1"], kw["n2"], kw["minmax"], kw["init"], **kw["opts"])


def _as_ref(m):
    f, i = K.model_trace_array(m)
    return dict(round_w=[m.weights(r) for r in range(m.rounds)], trace=[tuple(a) + tuple(b) for a, b in zip(f.tolist(), i.tolist())],
                sigma2=m.sigma2, sigma2_eval=m.sigma2_eval, stopped_nonfinite=m.stopped_nonfinite)


@pytest.mark.gpu
@pytest.mark.parametrize("name", K.IDS)
def test_device_equals_host_definition(ctx, name):
    from glia_amd import hmt
    kw = K.CASES[K.IDS.index(name)][1]
    host = _train(ctx, kw, host=True)
    dev = _train(ctx, kw)
    K.assert_same_as_reference(dev, _as_ref(host), exact=ctx.libm_exp() != 0)
    assert hmt.Context.internal_errors() == 0


@pytest.mark.gpu
def test_two_calls_return_identical_bytes_and_timing_is_reported(ctx):
    from glia_amd import hmt
    kw = K.CASES[K.IDS.index("shape_n192_d104_32_32")][1]
    a, b = _train(ctx, kw), _train(ctx, kw)
    assert a.rounds == b.rounds == 2
    for r in range(a.rounds):
        assert a.weights(r).tobytes() == b.weights(r).tobytes()
    assert a.trace.tobytes() == b.trace.tobytes() and len(a.trace) > 0
    t = hmt.last_mlp_train_timing(ctx)
    assert t["evals"] >= t["grad_evals"] >= t["iterations"] == int((a.trace["kind"] == 0).sum()) > 0
    assert t["ms_chunk"] > 0 and t["ms_fold"] > 0 and t["device_bytes"] > 192 * 105 * 8
    assert hmt.Context.internal_errors() == 0


@pytest.mark.gpu
def test_minmax_equals_training_on_rows_the_second_author_rescaled(ctx):
    from glia_amd import hmt
    kw = K.CASES[K.IDS.index("minmax")][1]
    mn, mx = kw["minmax"]
    a = _train(ctx, kw)
    b = hmt.train_mlp(ctx, _mlpdef.rescale(kw["rows"], mn, mx), kw["labels"], kw["n1"], kw["n2"], None, kw["init"], **kw["opts"])
    assert a.rounds == b.rounds == 2 and a.trace.tobytes() == b.trace.tobytes()
    for r in range(a.rounds):
        assert a.weights(r).tobytes() == b.weights(r).tobytes()
    # the classifier carries the table: it rescales raw rows itself
    clf = a.mlp(ctx)
    p = clf.predict(np.ascontiguousarray(kw["rows"]))
    assert _mlpdef.same(p, hmt.mlp_predict_host(a.weights(), kw["n1"], kw["n2"], kw["rows"], mn, mx)[0])
    clf.close()


@pytest.mark.gpu
def test_refusals_reach_the_device_entry_point_too(ctx):
    from glia_amd import hmt
    kw = K.CASES[K.IDS.index("ws_only")][1]
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_mlp(ctx, kw["rows"], kw["labels"], 33, 33, **kw["opts"])
    assert e.value.code == -3 and "32 units" in str(e.value)
    bad = np.array(kw["rows"])
    bad[5, 2] = np.inf
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_mlp(ctx, bad, kw["labels"], 3, 17, **kw["opts"])
    assert e.value.code == hmt.ERR_ARG and "not finite" in str(e.value)
    assert T.CHUNK == hmt.mlp_train_limits()["chunk_rows"]
