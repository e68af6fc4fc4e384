"""train_sshmt on the device (glia_amd/csrc/sshmt_train.hip) against the definition on the host (glia_hmt_sshmt_train_host, itself held
to the second author by tests/test_sshmt_host.py): weights after every round, the trace and both sigma series bit for bit on every
shared case (tests/_sshmt_cases.py) -- 1, 63, 64, 65 and 129 paths; 2, 63, 64, 65 and 130 unlabelled rows; paths of 1 to 8 rows;
caterpillars, balanced trees and forests; blocks; rows on no path; the term alone without labelled rows; skipped paths; one unit and 32
units; one column and 104 columns; logsig; every optimiser and step rule.  Where the context could not pin the host's exp
(glia_hmt_ctx_libm_exp reports 0) the device's sigmoid is its own libm's and the comparison is to 1e-9 relative instead."""
import numpy as np
import pytest

import _mlptrain_cases as MK
import _sshmt_cases as K


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
    return hmt.train_sshmt(None if host else ctx, kw["rows"], kw["labels"], kw["unlabelled"], kw["n1"], kw["n2"], kw["minmax"], kw["init"], **kw["opts"])


def _as_ref(m):
    f, i = MK.model_trace_array(m)
    return dict(round_w=[m.weights(r) for r in range(m.rounds)], trace=[tuple(a) + tuple(b) for a, b in zip(f.tolist(), i.tolist())],
                sigma2=m.sigma2, sigma2_eval=m.sigma2_eval, sigma_u2=m.sigma_u2, sigma_u2_eval=m.sigma_u2_eval, stopped_nonfinite=m.stopped_nonfinite,
                n_paths=m.n_paths, n_uns_rows=m.n_uns_rows)


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
    kw = K.CASES[K.IDS.index("shape_d104_32_32")][1]
    a, b = _train(ctx, kw), _train(ctx, kw)
    assert a.rounds == b.rounds == 2
    for r in range(a.rounds):
        assert a.weights(r).tobytes() == b.weights(r).tobytes()
    assert a.trace.tobytes() == b.trace.tobytes() and len(a.trace) > 0 and a.sigma_u2.tobytes() == b.sigma_u2.tobytes()
    t = hmt.last_sshmt_train_timing(ctx)
    assert t["n_paths"] == a.n_paths == 54 and t["n_uns_rows"] == a.n_uns_rows == 70
    assert t["u_evals"] >= t["u_grad_evals"] >= t["sup"]["iterations"] == int((a.trace["kind"] == 0).sum()) > 0
    assert t["u_evals"] == t["sup"]["evals"] and t["u_grad_evals"] == t["sup"]["grad_evals"]
    for k in ("ms_u_upload", "ms_u_weights", "ms_u_forward", "ms_u_paths", "ms_u_gather", "ms_u_chunk", "ms_u_fold", "ms_u_readback"):
        assert t[k] > 0, k
    assert t["sup"]["ms_chunk"] > 0 and t["sup"]["ms_total"] > 0 and t["u_device_bytes"] > 70 * 105 * 8 and t["sup"]["device_bytes"] > 65 * 105 * 8
    assert hmt.Context.internal_errors() == 0


@pytest.mark.gpu
def test_no_block_and_no_wu_is_the_supervised_trainer_byte_for_byte(ctx):
    """train_sshmt(ctx, ...) without blocks and train_mlp(ctx, ...) through the device entry points: 65 rows, 3 + 17 units -- the chunk
    kernel's <32> instantiation across a chunk boundary"""
    from glia_amd import hmt
    kw = MK.NO_TERM_CASES[0][1]
    assert (kw["rows"].shape[0], kw["n1"], kw["n2"]) == (65, 3, 17)
    a = hmt.train_mlp(ctx, kw["rows"], kw["labels"], kw["n1"], kw["n2"], kw["minmax"], kw["init"], **kw["opts"])
    b = hmt.train_sshmt(ctx, kw["rows"], kw["labels"], (), kw["n1"], kw["n2"], kw["minmax"], kw["init"], **dict(kw["opts"], wu=0.0))
    assert a.rounds == 2 and int((a.trace["kind"] == 0).sum()) > 0
    MK.assert_identical_models(a, b)
    assert b.n_paths == 0 and (b.sigma_u2 == 0.0).all()
    assert hmt.Context.internal_errors() == 0


@pytest.mark.gpu
def test_refusals_reach_the_device_entry_point_too(ctx):
    from glia_amd import hmt
    kw = K.CASES[K.IDS.index("wu_one")][1]
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_sshmt(ctx, kw["rows"], kw["labels"], kw["unlabelled"], 33, 33, **kw["opts"])
    assert e.value.code == -3 and "32 units" in str(e.value)
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_sshmt(ctx, kw["rows"], kw["labels"], kw["unlabelled"], 3, 17, **dict(kw["opts"], max_path_length=9))
    assert e.value.code == -3 and "above 8" in str(e.value)
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_sshmt(ctx, kw["rows"], kw["labels"], kw["unlabelled"], 3, 17, **dict(kw["opts"], uns_batch_size=16))
    assert e.value.code == -3 and "uns_batch_size" in str(e.value)
    bad = np.array(kw["unlabelled"][0][0])
    bad[5, 2] = np.inf
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_sshmt(ctx, kw["rows"], kw["labels"], [(bad, kw["unlabelled"][0][1])], 3, 17, **kw["opts"])
    assert e.value.code == hmt.ERR_ARG and "not finite" in str(e.value)
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_sshmt(ctx, kw["rows"], kw["labels"], [(kw["unlabelled"][0][0][:2], [[1, 2, 7], [1, 3, 8]])], 3, 17, **kw["opts"])
    assert e.value.code == hmt.ERR_ARG and "merge 1" in str(e.value)
    with pytest.raises(hmt.HmtError) as e:      # the supervised entry point keeps refusing the term
        hmt.train_mlp(ctx, kw["rows"], kw["labels"], 3, 17, **{k: v for k, v in kw["opts"].items() if k != "sigma_u"})
    assert e.value.code == -3 and "wu" in str(e.value)
    assert hmt.Context.internal_errors() == 0
