"""normalize_sample, train_mlp / train_logsig and pred_mlp / pred_logsig over files, end to end: the written models equal the library's
on the same (8-digit) rows, --fmm equals normalising first up to the rows' 8 digits, and --v 1 prints the reference's "gd:" and "learn-"
lines (alg/gd.hxx:185-186, main_train_sshmt_mlp.cxx:140-142)."""
import os
import re
import subprocess

import numpy as np
import pytest

import _mlpdef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cli")
GD = re.compile(r"^\tgd: (\d+) +fx = (\S+) +\|x\| = (\S+) +\|g\| = (\S+) +step = (\S+)$")
LEARN = re.compile(r"^\tlearn-(\d+): su = 0 \(0\), ss = (\S+) \((\S+)\)$")


def _run(tool, *args):
    r = subprocess.run([os.path.join(CLI, tool)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (tool, r.stderr)
    return r.stdout


def _read(path):
    return np.array([[float(v) for v in line.split()] for line in open(path) if line.strip()])


@pytest.mark.gpu
def test_files_end_to_end(tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    rng = np.random.default_rng(12)
    rows = rng.standard_normal((150, 9)) * np.arange(1, 10) + 3.0
    labels = np.where(rows[:, 0] + rows[:, 3] / 4.0 > 3.5, 1, -1)
    labels[::11] = 0
    fa, fb, la, lb = (tmp_path / n for n in ("a.txt", "b.txt", "la.txt", "lb.txt"))
    _mlpdef.write_rows(fa, rows[:100]); _mlpdef.write_rows(fb, rows[100:])
    la.write_text("".join("%d\n" % v for v in labels[:100])); lb.write_text("".join("%d\n" % v for v in labels[100:]))
    na, nb, mm = tmp_path / "na.txt", tmp_path / "nb.txt", tmp_path / "mm.txt"
    _run("normalize_sample", "--i", fa, fb, "--o", na, nb, "--om", mm)
    nrows = np.concatenate([_read(na), _read(nb)])
    assert nrows.shape == rows.shape and nrows.min() == -1.0 and abs(nrows.max() - 1.0) < 1e-7
    flags = ["--ws", "1", "--wr", "0.001", "--ss", "0.5", "--topt", "2", "--lr", "0.02", "--tw", "5", "--ts", "3", "--seed", "9"]
    opts = dict(ws=1.0, wr=0.001, sigma_s=0.5, optimizer=2, step=0.02, max_iterations=5, n_sigma_updates=3, seed=9)
    ctx = hmt.Context(0)
    # ---- train_mlp on the normalised files; a model every round ----
    out = _run("train_mlp", "--sl", la, lb, "--sf", na, nb, "--nn1", "6", "--nn2", "4", "--omp", tmp_path / "m%d.txt", "--si", "1", *flags)
    model = hmt.train_mlp(ctx, nrows, labels, 6, 4, **opts)
    for rnd in range(3):
        assert _mlpdef.same(hmt.mlp_file_parse(tmp_path / ("m%d.txt" % rnd)), model.weights(rnd))
    lines = out.split("\n")
    gd = [GD.match(x) for x in lines if x.startswith("\tgd:")]
    learn = [LEARN.match(x) for x in lines if x.startswith("\tlearn-")]
    assert len(gd) == 3 * 6 and all(gd) and len(learn) == 4 and all(learn)
    assert [int(m.group(1)) for m in gd] == list(range(6)) * 3 and [int(m.group(1)) for m in learn] == [0, 1, 2, 3]
    tr = model.trace
    assert [m.group(2) for m in gd] == ["%g" % v for v in tr["fx"]] and [m.group(5) for m in gd] == ["%g" % v for v in tr["step"]]
    assert lines[lines.index(learn[0].group(0)) + 1] == "\tgd: %-6d fx = %-12g |x| = %-12g |g| = %-12g step = %g" % (0, tr["fx"][0], tr["xnorm"][0], tr["gnorm"][0], tr["step"][0])
    assert "Use %d supervised samples." % int((labels != 0).sum()) in lines
    # without --si only the last round is written; --v 0 prints nothing
    out = _run("train_mlp", "--sl", la, lb, "--sf", na, nb, "--nn1", "6", "--nn2", "4", "--omp", tmp_path / "q%d.txt", "--v", "0", *flags)
    assert out == "" and not (tmp_path / "q0.txt").exists() and _mlpdef.same(hmt.mlp_file_parse(tmp_path / "q2.txt"), model.weights(2))
    # ---- pred_mlp with the written model: the library's predictions of the same rows, at the 6 digits the tool writes ----
    pa = tmp_path / "pa.txt"
    _run("pred_mlp", "--m", tmp_path / "m2.txt", "--f", na, "--nn1", "6", "--nn2", "4", "--p", pa)
    clf = model.mlp(ctx)
    assert pa.read_text() == "".join("%g\n" % v for v in clf.predict(np.ascontiguousarray(nrows[:100])))
    clf.close()
    # ---- --fmm rescales inside: the library with minmax = the table the file holds ----
    _run("train_mlp", "--sl", la, lb, "--sf", fa, fb, "--fmm", mm, "--nn1", "6", "--nn2", "4", "--omp", tmp_path / "f%d.txt", "--v", "0", *flags)
    t = _read(mm)
    m2 = hmt.train_mlp(ctx, rows, labels, 6, 4, minmax=(t[0], t[1]), **opts)
    assert _mlpdef.same(hmt.mlp_file_parse(tmp_path / "f2.txt"), m2.weights())
    pf = tmp_path / "pf.txt"
    _run("pred_mlp", "--m", tmp_path / "f2.txt", "--fmm", mm, "--f", fb, "--nn1", "6", "--nn2", "4", "--p", pf)
    clf = m2.mlp(ctx)
    assert pf.read_text() == "".join("%g\n" % v for v in clf.predict(np.ascontiguousarray(rows[100:])))
    clf.close()
    # ---- train_logsig, continued from its own model with --im ----
    _run("train_logsig", "--sl", la, lb, "--sf", na, nb, "--omp", tmp_path / "g%d.txt", "--v", "0", "--lrd", "0.5", *flags)
    lg = hmt.train_mlp(ctx, nrows, labels, 0, 0, step_decay=0.5, **opts)
    assert _mlpdef.same(hmt.mlp_file_parse(tmp_path / "g2.txt"), lg.weights())
    _run("train_logsig", "--sl", la, lb, "--sf", na, nb, "--im", tmp_path / "g2.txt", "--omp", tmp_path / "h%d.txt", "--v", "0", *flags)
    lg2 = hmt.train_mlp(ctx, nrows, labels, 0, 0, init=lg.weights(), **opts)
    assert _mlpdef.same(hmt.mlp_file_parse(tmp_path / "h2.txt"), lg2.weights()) and not _mlpdef.same(lg.weights(), lg2.weights())
    pl = tmp_path / "pl.txt"
    _run("pred_logsig", "--m", tmp_path / "h2.txt", "--f", na, "--p", pl)
    assert len(pl.read_text().splitlines()) == 100
    for m in (model, m2, lg, lg2):
        m.close()
    assert hmt.Context.internal_errors() == 0
    ctx.close()
