"""Mini-batch training on the host (glia_hmt_mlp_train_batches / glia_hmt_sshmt_train_batches with ctx NULL: glia_amd/csrc/mlp_batch.hpp,
the definition of DESIGN 3.17) against the second author tests/_batchdef.py: weights after every round, trace and both sigma series bit
for bit.  150 labelled rows of 5 columns in batches of 70 (a 64-row and a 6-row chunk), 3 + 3 MLP and logsig, the three optimisers,
the fixed and the adaptive step, epochs and batch counts, the path term with a sampler on either term or both.  No GPU."""
import numpy as np
import pytest

import _batch_cases as BK
import _batchdef as B
import _mlptrain_cases as MK
import _sshmt_cases as K


def _hmt():
    from glia_amd import hmt
    return hmt


@pytest.mark.parametrize("name", BK.HOST_IDS)
def test_host_equals_second_author(name):
    m = BK.train(_hmt(), None, BK.host_kw(name))
    K.assert_same_as_reference(m, BK.reference(name))
    m.close()


def test_cases_reach_what_they_are_for():
    """read from the second author's results"""
    # three draws an epoch over 150 rows in batches of 70; 3 iterations, 2 rounds
    r = BK.reference("mlp_fixed_opt1")
    assert (r["steps"], r["batches"]) == (6, 18)
    assert BK.reference("mlp_te2")["batches"] == 36 and BK.reference("logsig_tb3")["batches"] == 18
    # the roll-back runs the step again, on new batches: more steps than iterations
    r = BK.reference("mlp_rollback")
    rb = sum(t[8] for t in r["trace"] if t[7] == 0)
    assert rb >= 1 and r["steps"] == sum(1 for t in r["trace"] if t[7] == 0) + rb and r["batches"] == 3 * r["steps"]
    # 76 paths in batches of 70: two draws an epoch, also when the rows' sampler would take three
    r = BK.reference("paths_only_sampler")
    assert r["n_paths"] == 76 and r["batches"] == 2 * r["steps"]
    # both: the paths end the first epoch after two draws; the rows, which nobody reset, end the next after ONE (their third draw)
    r = BK.reference("both_samplers")
    assert r["steps"] >= 6 and r["batches"] in (3 * r["steps"] // 2, (3 * r["steps"] + 1) // 2)
    assert BK.reference("rows_only_sampler")["batches"] == 3 * BK.reference("rows_only_sampler")["steps"]
    # the batches change the answer, and so does the sampler's seed
    kw = BK.host_kw("mlp_fixed_opt1")
    full = B.train(kw["rows"], kw["labels"], None, 3, 3, None, None, None, **dict(kw["opts"], sup_batch_size=-1))
    other = B.train(kw["rows"], kw["labels"], None, 3, 3, None, None, dict(seed=99), **kw["opts"])
    w = BK.reference("mlp_fixed_opt1")["round_w"][-1]
    assert full["batches"] == 0 and not np.array_equal(full["round_w"][-1], w) and not np.array_equal(other["round_w"][-1], w)


def test_rollback_count_of_the_library():
    m = BK.train(_hmt(), None, BK.host_kw("mlp_rollback"))
    assert int(m.trace["rollbacks"][m.trace["kind"] == 0].sum()) >= 1
    m.close()


@pytest.mark.parametrize("sshmt", [False, True])
def test_without_a_sampler_the_new_entry_point_is_the_old_one(sshmt):
    hmt = _hmt()
    kw = BK.host_kw("both_samplers" if sshmt else "mlp_fixed_opt2")
    o = dict(kw["opts"], sup_batch_size=-1, uns_batch_size=-1)
    batch = dict(seed=5, epochs_per_iteration=3, batches_per_iteration=7)
    if sshmt:
        a = hmt.train_sshmt_batches(None, kw["rows"], kw["labels"], kw["unlabelled"], 3, 3, batch=batch, **o)
        b = hmt.train_sshmt_host(kw["rows"], kw["labels"], kw["unlabelled"], 3, 3, **o)
    else:
        a = hmt.train_mlp_batches(None, kw["rows"], kw["labels"], 3, 3, batch=batch, **o)
        b = hmt.train_mlp_host(kw["rows"], kw["labels"], 3, 3, **o)
    MK.assert_identical_models(a, b)
    assert a.sigma_u2.tobytes() == b.sigma_u2.tobytes()


def test_the_existing_entry_points_still_refuse():
    hmt = _hmt()
    kw = BK.host_kw("both_samplers")
    for field, flag in (("sup_batch_size", "--bss"), ("uns_batch_size", "--bsu"), ("balance_sup_batch", "--bb")):
        o = dict(kw["opts"], sup_batch_size=-1, uns_batch_size=-1)
        o[field] = 1 if field == "balance_sup_batch" else 16
        for call in (lambda: hmt.train_mlp_host(kw["rows"], kw["labels"], 3, 3, **{k: v for k, v in o.items() if k not in ("wu", "sigma_u")}),
                     lambda: hmt.train_sshmt_host(kw["rows"], kw["labels"], kw["unlabelled"], 3, 3, **o)):
            with pytest.raises(hmt.HmtError) as e:
                call()
            assert flag in str(e.value)
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_mlp_batches(None, kw["rows"], kw["labels"], 3, 3, ws=1.0, sigma_s=0.5, sup_batch_size=8, alt_su=1)
    assert "alt_su" in str(e.value)


def test_errors_of_the_trainers():
    hmt = _hmt()
    kw = BK.host_kw("both_samplers")
    base = dict(ws=1.0, sigma_s=0.5, step=0.05, max_iterations=1, n_sigma_updates=1)
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_mlp_batches(None, kw["rows"], kw["labels"], 3, 3, sup_batch_size=151, **base)
    assert e.value.code == hmt.ERR_ARG and "Error: totalSize must be greater than batchSize" in str(e.value)
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_sshmt_batches(None, kw["rows"], kw["labels"], kw["unlabelled"], 3, 3, uns_batch_size=77, wu=0.5, sigma_u=0.7, **base)
    assert e.value.code == hmt.ERR_ARG and "Error: totalSize must be greater than batchSize" in str(e.value)
    with pytest.raises(hmt.HmtError) as e:                                     # a path sampler while the path term is off
        hmt.train_sshmt_batches(None, kw["rows"], kw["labels"], kw["unlabelled"], 3, 3, uns_batch_size=8, **base)
    assert e.value.code == hmt.ERR_ARG and "a term that is off" in str(e.value)
    with pytest.raises(hmt.HmtError) as e:
        hmt.train_mlp_batches(None, kw["rows"], np.ones(150, np.int32), 3, 3, sup_batch_size=8, balance_sup_batch=1, **base)
    assert e.value.code == hmt.ERR_ARG and "has no row" in str(e.value)


def test_adam_in_batches_of_32_lowers_the_full_data_energy():
    """linearly separable rows: after one round of Adam in batches of 32 the energy over ALL rows is below the initial one"""
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((200, 4))
    rows[:, 0] += np.where(rows[:, 0] > 0.0, 1.0, -1.0)
    labels = np.where(rows[:, 0] > 0.0, 1, -1)
    m = _hmt().train_mlp_batches(None, rows, labels, 3, 3, batch=dict(seed=1), ws=1.0, sigma_s=0.5, optimizer=2, step=0.01, max_iterations=5,
                                 n_sigma_updates=1, sup_batch_size=32, seed=3)
    tr = m.trace
    assert tr["kind"][0] == 0 and tr["kind"][-1] == 1 and tr["fx"][-1] < tr["fx"][0]
    m.close()
