"""train_mlp and train_sshmt_mlp with --bseed over files: the written models are the library call's on the same rows, load into
pred_mlp, and without --bseed the batch flags stay refused by name."""
import os
import subprocess

import numpy as np
import pytest

import _mlpdef
import _sshmt_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cli")


def _run(tool, *args, ok=True):
    r = subprocess.run([os.path.join(CLI, tool)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert (r.returncode == 0) == ok, (tool, r.stderr)
    return r


def _read(path):
    return np.array([[float(v) for v in line.split()] for line in open(path) if line.strip()])


@pytest.mark.gpu
def test_batch_flags_end_to_end(tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    rng = np.random.default_rng(21)
    rows = rng.standard_normal((150, 6))
    labels = np.where(rows[:, 0] + rows[:, 3] / 4.0 > 0.1, 1, -1)
    fr, fl = tmp_path / "rows.txt", tmp_path / "labels.txt"
    _mlpdef.write_rows(fr, rows)
    fl.write_text("".join("%d\n" % v for v in labels))
    rows = _read(fr)                                                  # the 8 digits the file holds
    flags = ["--ws", "1", "--wr", "0.001", "--ss", "0.5", "--topt", "2", "--lr", "0.02", "--tw", "3", "--ts", "2", "--seed", "9", "--v", "0"]
    opts = dict(ws=1.0, wr=0.001, sigma_s=0.5, optimizer=2, step=0.02, max_iterations=3, n_sigma_updates=2, seed=9)
    ctx = hmt.Context(0)
    # ---- train_mlp --bss 64 --bseed 7 ----
    _run("train_mlp", "--sl", fl, "--sf", fr, "--nn1", "6", "--nn2", "4", "--omp", tmp_path / "m%d.txt", "--bss", "64", "--bseed", "7", *flags)
    model = hmt.train_mlp_batches(ctx, rows, labels, 6, 4, batch=dict(seed=7), sup_batch_size=64, **opts)
    assert _mlpdef.same(hmt.mlp_file_parse(tmp_path / "m1.txt"), model.weights())
    full = hmt.train_mlp(ctx, rows, labels, 6, 4, **opts)
    assert not _mlpdef.same(model.weights(), full.weights())
    pa = tmp_path / "pa.txt"
    _run("pred_mlp", "--m", tmp_path / "m1.txt", "--f", fr, "--nn1", "6", "--nn2", "4", "--p", pa)
    clf = model.mlp(ctx)
    assert pa.read_text() == "".join("%g\n" % v for v in clf.predict(np.ascontiguousarray(rows)))
    clf.close()
    # --bb, --te 0 --tb 2
    _run("train_mlp", "--sl", fl, "--sf", fr, "--nn1", "6", "--nn2", "4", "--omp", tmp_path / "b%d.txt", "--bss", "33", "--bb", "1", "--te", "0", "--tb", "2",
         "--bseed", "8", *flags)
    mb = hmt.train_mlp_batches(ctx, rows, labels, 6, 4, batch=dict(seed=8, epochs_per_iteration=0, batches_per_iteration=2), sup_batch_size=33,
                               balance_sup_batch=1, **opts)
    assert _mlpdef.same(hmt.mlp_file_parse(tmp_path / "b1.txt"), mb.weights())
    # ---- train_sshmt_mlp --bsu ----
    urows, order = K._block(K.caterpillar(40), 6, 3)
    fu, fo = tmp_path / "urows.txt", tmp_path / "order.txt"
    _mlpdef.write_rows(fu, urows)
    fo.write_text("".join("%d %d %d\n" % tuple(m) for m in order))
    urows = _read(fu)
    _run("train_sshmt_mlp", "--sl", fl, "--sf", fr, "--uo", fo, "--uf", fu, "--wu", "0.5", "--su", "0.7", "--nn1", "6", "--nn2", "4", "--omp",
         tmp_path / "u%d.txt", "--bsu", "20", "--bss", "64", "--bseed", "7", *flags)
    mu = hmt.train_sshmt_batches(ctx, rows, labels, [(urows, order)], 6, 4, batch=dict(seed=7), sup_batch_size=64, uns_batch_size=20, wu=0.5,
                                 sigma_u=0.7, **opts)
    assert _mlpdef.same(hmt.mlp_file_parse(tmp_path / "u1.txt"), mu.weights()) and not _mlpdef.same(mu.weights(), model.weights())
    # ---- without --bseed the refusals stand ----
    r = _run("train_mlp", "--sl", fl, "--sf", fr, "--omp", tmp_path / "x%d.txt", "--bss", "64", *flags, ok=False)
    assert "--bss" in r.stderr and "not supported" in r.stderr
    r = _run("train_sshmt_mlp", "--sl", fl, "--sf", fr, "--omp", tmp_path / "x%d.txt", "--bsu", "20", *flags, ok=False)
    assert "--bsu" in r.stderr
    r = _run("train_mlp", "--sl", fl, "--sf", fr, "--omp", tmp_path / "x%d.txt", "--bss", "151", "--bseed", "1", *flags, ok=False)
    assert "totalSize must be greater than batchSize" in r.stderr
    for m in (model, full, mb, mu):
        m.close()
    assert hmt.Context.internal_errors() == 0
    ctx.close()
