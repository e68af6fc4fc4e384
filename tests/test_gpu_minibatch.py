"""Mini-batch training on the device (glia_amd/csrc/mlp_batch.hip: the batches of a step back to back on the stream, k_batch_step, the
gathered instances of the chunk kernel) against the definition on the host (ctx None, itself held to the second author by
tests/test_minibatch_host.py): weights after every round, trace and both sigma series bit for bit, on the smallest shapes that reach
every branch (tests/_batch_cases.py: gpu_cases).  The cross-check route GLIA_HMT_BATCH = step gives the same bytes; the stream route
waits for the device once per mini-batch step.  Where the context could not pin the host's exp the comparison is to 1e-9 relative."""
import numpy as np
import pytest

import _batch_cases as BK
import _mlptrain_cases as MK
import _sshmt_cases as K
import _sshmtdef as S


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    c.close()


def _kw(name):
    return BK.GPU[BK.GPU_IDS.index(name)][1]


def _as_ref(m):
    f, i = MK.model_trace_array(m)
    return dict(round_w=[m.weights(r) for r in range(m.rounds)], trace=[tuple(a) + tuple(b) for a, b in zip(f.tolist(), i.tolist())],
                sigma2=m.sigma2, sigma2_eval=m.sigma2_eval, sigma_u2=m.sigma_u2, sigma_u2_eval=m.sigma_u2_eval, stopped_nonfinite=m.stopped_nonfinite,
                n_paths=m.n_paths, n_uns_rows=m.n_uns_rows)


@pytest.mark.gpu
@pytest.mark.parametrize("name", BK.GPU_IDS)
def test_device_equals_host_definition(ctx, name):
    from glia_amd import hmt
    kw = _kw(name)
    host = BK.train(hmt, None, kw)
    dev = BK.train(hmt, ctx, kw)
    K.assert_same_as_reference(dev, _as_ref(host), exact=ctx.libm_exp() != 0)
    t = hmt.last_batch_timing(ctx)
    assert t["route"] == 0 and t["steps"] > 0 and t["batches"] >= t["steps"]
    assert t["syncs"] == t["steps"], "the stream route waits once per mini-batch step"
    assert t["ms_steps"] > 0 and t["ms_plan"] > 0 and t["plan_bytes"] > 0
    assert hmt.Context.internal_errors() == 0


def test_cases_reach_what_they_are_for():
    """from the second author's sampler and paths alone (no GPU): the path batches name more than 64 rows; a batch holds a row that two
    of its paths name and that a path outside it names too; the roll-back case rolls back"""
    import _batchdef as B
    kw = _kw("paths_b65")
    paths = []
    row0 = 0
    for rows, order in kw["unlabelled"]:
        paths += [[row0 + i for i in p] for p in S.merge_paths(order, 3, 2)]
        row0 += len(rows)
    assert len(paths) == 76
    _, uns, _ = B.plan([], len(paths), 1, uns_batch_size=65, seed=kw["batch"]["seed"])
    inside = set(uns[0])
    assert len({r for p in inside for r in paths[p]}) > 64
    shared = [r for r in range(row0) if sum(r in paths[p] for p in inside) >= 2 and any(r in paths[p] for p in range(76) if p not in inside)]
    assert shared
    kw = _kw("rollback")
    r = B.train(kw["rows"], kw["labels"], kw["unlabelled"], kw["n1"], kw["n2"], None, None, kw["batch"], **kw["opts"])
    assert sum(t[8] for t in r["trace"] if t[7] == 0) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sup_b65_17_17", "sup_logsig_epoch", "paths_b65", "both_samplers", "rollback"])
def test_step_route_gives_the_bytes_of_the_stream_route(ctx, name):
    from glia_amd import hmt
    kw = _kw(name)
    a = BK.train(hmt, ctx, kw)
    ta = hmt.last_batch_timing(ctx)
    with hmt.options(GLIA_HMT_BATCH="step"):
        b = BK.train(hmt, ctx, kw)
        tb = hmt.last_batch_timing(ctx)
    MK.assert_identical_models(a, b)
    assert a.sigma_u2.tobytes() == b.sigma_u2.tobytes()
    assert (ta["route"], tb["route"]) == (0, 1) and ta["steps"] == tb["steps"] and ta["batches"] == tb["batches"]
    assert tb["syncs"] >= tb["batches"] > ta["syncs"] == ta["steps"]
    if name == "rollback":
        assert int(a.trace["rollbacks"][a.trace["kind"] == 0].sum()) >= 1
    with pytest.raises(hmt.HmtError):
        with hmt.options(GLIA_HMT_BATCH="neither"):
            BK.train(hmt, ctx, kw)
    assert hmt.Context.internal_errors() == 0


@pytest.mark.gpu
def test_without_a_sampler_the_device_entry_point_is_the_old_one(ctx):
    from glia_amd import hmt
    kw = _kw("both_samplers")
    o = dict(kw["opts"], sup_batch_size=-1, uns_batch_size=-1)
    a = hmt.train_sshmt_batches(ctx, kw["rows"], kw["labels"], kw["unlabelled"], 16, 16, batch=dict(seed=3), **o)
    b = hmt.train_sshmt(ctx, kw["rows"], kw["labels"], kw["unlabelled"], 16, 16, **o)
    MK.assert_identical_models(a, b)
    assert hmt.last_batch_timing(ctx)["steps"] == 0
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_sshmt(ctx, kw["rows"], kw["labels"], kw["unlabelled"], 16, 16, **kw["opts"])
    assert "--bss" in str(e.value)
