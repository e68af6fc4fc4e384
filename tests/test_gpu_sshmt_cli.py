"""train_sshmt_mlp / train_sshmt_logsig over files, end to end: labelled rows and labels, two (--uo, --uf) pairs of different sizes, the
written models equal the library's on the same rows, --fmm equals the library's minmax, --v 1 prints the "learn-" lines with both sigmas
and the counts of supervised and unsupervised samples, the term alone runs without --sl / --sf, and pred_mlp accepts the model."""
import os
import re
import subprocess

import numpy as np
import pytest

import _mlpdef
import _sshmt_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cli")
LEARN = re.compile(r"^\tlearn-(\d+): su = (\S+) \((\S+)\), ss = (\S+) \((\S+)\)$")


def _run(tool, *args):
    r = subprocess.run([os.path.join(CLI, tool)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (tool, r.stderr)
    return r.stdout


@pytest.mark.gpu
def test_files_end_to_end(tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    rng = np.random.default_rng(21)
    rows = rng.standard_normal((90, 6)) * np.arange(1, 7) + 2.0
    labels = np.where(rows[:, 0] + rows[:, 2] / 3.0 > 2.5, 1, -1)
    labels[::13] = 0
    orders = [K.forest(70, 90, 4) + 1, K.caterpillar(33, key0=5)]
    urows = [rng.standard_normal((len(o), 6)) * np.arange(1, 7) + 2.0 for o in orders]
    sf, sl, mm = tmp_path / "s.txt", tmp_path / "l.txt", tmp_path / "mm.txt"
    _mlpdef.write_rows(sf, rows)
    sl.write_text("".join("%d\n" % v for v in labels))
    uo, uf = [tmp_path / ("o%d.txt" % i) for i in range(2)], [tmp_path / ("u%d.txt" % i) for i in range(2)]
    for i in range(2):
        uo[i].write_text("".join("%d %d %d\n" % tuple(m) for m in orders[i].tolist()))
        _mlpdef.write_rows(uf[i], urows[i])
    mn, mx = hmt.rows_minmax([rows] + urows)
    _mlpdef.write_rows(mm, [mn, mx])
    unl = list(zip(urows, orders))
    flags = ["--ws", "1", "--wu", "0.5", "--wr", "0.001", "--ss", "0.5", "--su", "0.6", "--usu", "1", "--topt", "2", "--lr", "0.02", "--tw", "4", "--ts", "3",
             "--seed", "9", "--fmm", mm]
    opts = dict(ws=1.0, wu=0.5, wr=0.001, sigma_s=0.5, sigma_u=0.6, update_sigma_u=1, optimizer=2, step=0.02, max_iterations=4, n_sigma_updates=3, seed=9)
    ctx = hmt.Context(0)
    # ---- train_sshmt_mlp; a model every round ----
    out = _run("train_sshmt_mlp", "--sl", sl, "--sf", sf, "--uo", uo[0], uo[1], "--uf", uf[0], uf[1], "--nn1", "6", "--nn2", "4", "--omp", tmp_path / "m%d.txt",
               "--si", "1", *flags)
    model = hmt.train_sshmt(ctx, rows, labels, unl, 6, 4, minmax=(mn, mx), **opts)
    assert model.n_paths == sum(len(hmt.merge_paths(o)) for o in orders) > 64 and model.n_uns_rows == 103
    for rnd in range(3):
        assert _mlpdef.same(hmt.mlp_file_parse(tmp_path / ("m%d.txt" % rnd)), model.weights(rnd))
    lines = out.split("\n")
    learn = [LEARN.match(x) for x in lines if x.startswith("\tlearn-")]
    assert len(learn) == 4 and all(learn) and len([x for x in lines if x.startswith("\tgd:")]) == 3 * 5
    assert [m.group(2) for m in learn] == ["%g" % np.sqrt(v) for v in model.sigma_u2] and [m.group(4) for m in learn] == ["%g" % 0.5] * 4
    assert len(set(m.group(2) for m in learn)) > 1, "--usu 1 moves sigma_u"
    assert "Use %d supervised samples." % int((labels != 0).sum()) in lines and "Use %d unsupervised samples." % model.n_paths in lines
    # ---- the model differs from the supervised tool's, and pred_mlp takes it ----
    sflags = ["--ws", "1", "--wr", "0.001", "--ss", "0.5", "--topt", "2", "--lr", "0.02", "--tw", "4", "--ts", "3", "--seed", "9", "--fmm", mm]
    _run("train_mlp", "--sl", sl, "--sf", sf, "--nn1", "6", "--nn2", "4", "--omp", tmp_path / "s%d.txt", "--v", "0", *sflags)
    assert not _mlpdef.same(hmt.mlp_file_parse(tmp_path / "s2.txt"), model.weights(2))
    pa = tmp_path / "pa.txt"
    _run("pred_mlp", "--m", tmp_path / "m2.txt", "--fmm", mm, "--f", uf[1], "--nn1", "6", "--nn2", "4", "--p", pa)
    clf = model.mlp(ctx)
    assert pa.read_text() == "".join("%g\n" % v for v in clf.predict(np.ascontiguousarray(urows[1])))
    clf.close()
    # ---- the term alone: no --sl / --sf; --v 0 prints nothing, only the last round is written ----
    out = _run("train_sshmt_mlp", "--uo", uo[0], "--uf", uf[0], "--nn1", "6", "--nn2", "4", "--omp", tmp_path / "q%d.txt", "--v", "0", "--wu", "1", "--su", "0.6",
               "--wr", "0.001", "--lr", "0.05", "--lrd", "0.5", "--tw", "3", "--ts", "2", "--fmm", mm)
    m2 = hmt.train_sshmt(ctx, None, None, unl[:1], 6, 4, minmax=(mn, mx), wu=1.0, sigma_u=0.6, wr=0.001, step=0.05, step_decay=0.5, max_iterations=3,
                         n_sigma_updates=2)
    assert out == "" and not (tmp_path / "q0.txt").exists() and _mlpdef.same(hmt.mlp_file_parse(tmp_path / "q1.txt"), m2.weights(1))
    # ---- train_sshmt_logsig, continued from its own model with --im ----
    _run("train_sshmt_logsig", "--sl", sl, "--sf", sf, "--uo", uo[1], "--uf", uf[1], "--omp", tmp_path / "g%d.txt", "--v", "0", *flags)
    lg = hmt.train_sshmt(ctx, rows, labels, unl[1:], 0, 0, minmax=(mn, mx), **opts)
    assert _mlpdef.same(hmt.mlp_file_parse(tmp_path / "g2.txt"), lg.weights())
    _run("train_sshmt_logsig", "--sl", sl, "--sf", sf, "--uo", uo[1], "--uf", uf[1], "--im", tmp_path / "g2.txt", "--omp", tmp_path / "h%d.txt", "--v", "0", *flags)
    lg2 = hmt.train_sshmt(ctx, rows, labels, unl[1:], 0, 0, minmax=(mn, mx), init=lg.weights(), **opts)
    assert _mlpdef.same(hmt.mlp_file_parse(tmp_path / "h2.txt"), lg2.weights()) and not _mlpdef.same(lg.weights(), lg2.weights())
    # ---- a row count that is not the order's ----
    r = subprocess.run([os.path.join(CLI, "train_sshmt_mlp"), "--uo", str(uo[0]), "--uf", str(uf[1]), "--omp", "x", "--wu", "1", "--su", "1"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "33 rows" in r.stderr and "70 merges" in r.stderr
    for m in (model, m2, lg, lg2):
        m.close()
    assert hmt.Context.internal_errors() == 0
    ctx.close()


def _write_mha(path, a):
    et = {np.dtype(np.uint32): "MET_UINT", np.dtype(np.float32): "MET_FLOAT"}[a.dtype]
    with open(path, "wb") as f:
        f.write(("ObjectType = Image\nNDims = %d\nBinaryData = True\nBinaryDataByteOrderMSB = False\nDimSize = %s\nElementType = %s\n"
                 "ElementDataFile = LOCAL\n" % (a.ndim, " ".join(str(v) for v in a.shape[::-1]), et)).encode())
        f.write(np.ascontiguousarray(a).tobytes())


def _rows(path):
    return np.array([[float(x) for x in ln.split()] for ln in open(path).read().split("\n") if ln.strip()])


@pytest.mark.gpu
def test_the_tools_chain_from_images_to_a_classifiers_order(tmp_path):
    """two synth 32^3 volumes, one with truth: merge_order_pb -> bc_feat -> (bc_label_ri) -> normalize_sample -> train_sshmt_mlp; the model
    is the library's on the files' rows, and pred_mlp and merge_order_bc --bct 2 accept it"""
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    from oracle import pyoracle as O
    p = lambda n: str(tmp_path / n)
    feat = ["--rbb", "8", "--rbl", "0", "--rbu", "1", "--bt", "0.2", "0.5", "0.8"]
    for tag, seed in (("l", 0x9E3779B97F4A7C15), ("u", 12345)):
        labels, pb = O.synth((32, 32, 32), 8, 16, seed=seed)
        _write_mha(p("seg_%s.mha" % tag), labels)
        _write_mha(p("pb_%s.mha" % tag), pb)
        _run("merge_order_pb", "-s", p("seg_%s.mha" % tag), "-p", p("pb_%s.mha" % tag), "-t", "2", "-o", p("order_%s.txt" % tag))
        _run("bc_feat", "-s", p("seg_%s.mha" % tag), "-o", p("order_%s.txt" % tag), "--pb", p("pb_%s.mha" % tag), "--rbi", p("pb_%s.mha" % tag), *feat,
             "-b", p("feats_%s.txt" % tag))
    z, y, x = np.meshgrid(*[np.arange(32) // 12] * 3, indexing="ij")
    _write_mha(p("truth.mha"), ((z * 3 + y) * 3 + x + 1).astype(np.uint32))
    _run("bc_label_ri", "-s", p("seg_l.mha"), "-o", p("order_l.txt"), "-t", p("truth.mha"), "-l", p("labels.txt"))
    _run("normalize_sample", "--i", p("feats_l.txt"), p("feats_u.txt"), "--o", p("n_l.txt"), p("n_u.txt"), "--om", p("mm.txt"))
    flags = ["--ws", "1", "--wu", "1", "--wr", "0.0001", "--ss", "0.5", "--su", "0.5", "--lr", "0.5", "--lrd", "0.5", "--tw", "4", "--ts", "2"]
    out = _run("train_sshmt_mlp", "--sl", p("labels.txt"), "--sf", p("n_l.txt"), "--uo", p("order_u.txt"), "--uf", p("n_u.txt"), "--omp", p("m%d.txt"), *flags)
    order_u = np.loadtxt(p("order_u.txt"), dtype=np.int64).reshape(-1, 3)
    lab = _rows(p("labels.txt"))[:, 0].astype(np.int32)
    assert len(order_u) == 63 == len(lab) and set(lab.tolist()) == {1, -1}
    n_paths = len(hmt.merge_paths(order_u))
    assert n_paths > 30 and "Use 63 supervised samples." in out and "Use %d unsupervised samples." % n_paths in out
    ctx = hmt.Context(0)
    model = hmt.train_sshmt(ctx, _rows(p("n_l.txt")), lab, [(_rows(p("n_u.txt")), order_u)], 10, 10, ws=1.0, wu=1.0, wr=0.0001, sigma_s=0.5, sigma_u=0.5,
                            step=0.5, step_decay=0.5, max_iterations=4, n_sigma_updates=2)
    assert _mlpdef.same(hmt.mlp_file_parse(p("m1.txt")), model.weights()) and not model.stopped_nonfinite
    _run("pred_mlp", "--m", p("m1.txt"), "--f", p("n_u.txt"), "--nn1", "10", "--nn2", "10", "--p", p("pred.txt"))
    pred = _rows(p("pred.txt"))
    assert pred.shape == (63, 1) and (pred >= 0).all() and (pred <= 1).all()
    _run("merge_order_bc", "--bct", "2", "--bcm", p("m1.txt"), "--bcfmm", p("mm.txt"), "-s", p("seg_u.mha"), "--pb", p("pb_u.mha"), "--rbi", p("pb_u.mha"), *feat,
         "-n", "0", "-l", "0", "-o", p("order_bc.txt"), "--sal", p("sal_bc.txt"))
    assert np.loadtxt(p("order_bc.txt"), dtype=np.int64).reshape(-1, 3).shape == (63, 3) and len(_rows(p("sal_bc.txt"))) == 63
    model.close()
    assert hmt.Context.internal_errors() == 0
    ctx.close()
