"""The tools around the MLP / logsig trainer, without a GPU: cli/normalize_sample against a plain-Python restatement of
stats::rescale (util/stats.hxx:264-318), cli/mlp_train_check's digests against the second author (tests/_mlptraindef.py), the usage
and refusals of cli/train_mlp and cli/train_logsig, and a model file written by MLPModel.write read back bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import _mlpdef
import _mlptraindef as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cli")
FEPS = 2.22e-16
DBL_MAX, DBL_MIN = 1.7976931348623157e308, 2.2250738585072014e-308


def _run(tool, *args):
    return subprocess.run([os.path.join(CLI, tool)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def _write_rows(path, rows, fmt="%.17g"):
    with open(path, "w") as f:
        for r in rows:
            f.write(" ".join(fmt % v for v in r) + "\n")


def _normalize(blocks, table=None, lo=-1.0, hi=1.0):
    """stats::rescale over several blocks as loops over Python floats: (rescaled blocks, minima, maxima)"""
    dim = len(blocks[0][0])
    if table is None:
        mn, mx = [DBL_MAX] * dim, [DBL_MIN] * dim          # FVAL_MAX, FVAL_MIN (glia_base.hxx:46-47)
        for b in blocks:
            for row in b:
                for j, f in enumerate(row):
                    if f < mn[j]:
                        mn[j] = f
                    if f > mx[j]:
                        mx[j] = f
    else:
        mn, mx = table
    diff = hi - lo
    out = [[[diff * (f - mn[j]) / (mx[j] - mn[j] + FEPS) + lo for j, f in enumerate(row)] for row in b] for b in blocks]
    return out, mn, mx


def _text(rows):
    return "".join("".join("%.8g " % v for v in r) + "\n" for r in rows)


def test_normalize_sample(tmp_path):
    rng = np.random.default_rng(3)
    a = (rng.standard_normal((7, 5)) * 3.0).tolist()
    b = (rng.standard_normal((4, 5)) * 3.0 + 1.0).tolist()
    for row in a + b:
        row[2] = 0.75                                      # a constant column: the denominator is FEPS
        row[4] = -abs(row[4])                              # no positive value: the maximum stays at DBL_MIN
    fa, fb = tmp_path / "a.txt", tmp_path / "b.txt"
    _write_rows(fa, a); _write_rows(fb, b)
    oa, ob, om = tmp_path / "oa.txt", tmp_path / "ob.txt", tmp_path / "mm.txt"
    r = _run("normalize_sample", "--i", fa, fb, "--o", oa, ob, "--om", om)
    assert r.returncode == 0, r.stderr
    (wa, wb), mn, mx = _normalize([a, b])
    assert mn[2] == mx[2] == 0.75 and mx[4] == DBL_MIN and all(v == -1.0 for v in np.array(wa)[:, 2])
    assert oa.read_text() == _text(wa) and ob.read_text() == _text(wb)
    assert om.read_text() == _text([mn, mx])
    assert len(oa.read_text().split()[0].lstrip("-").replace(".", "")) <= 8 + 4          # 8 significant digits (and an exponent at most)
    # the library's table is the tool's
    from glia_amd import hmt
    lmn, lmx = hmt.rows_minmax([np.array(a), np.array(b)])
    assert lmn.tolist() == mn and lmx.tolist() == mx
    # --im: the table is read (as written: 8 digits), none is written; another output range
    o2, om2 = tmp_path / "o2.txt", tmp_path / "mm2.txt"
    r = _run("normalize_sample", "--i", fb, "--im", om, "--o", o2, "--om", om2, "--min", "0", "--max", "10")
    assert r.returncode == 0, r.stderr
    t = [[float(v) for v in line.split()] for line in om.read_text().splitlines()]
    (w2,), _, _ = _normalize([b], (t[0], t[1]), 0.0, 10.0)
    assert o2.read_text() == _text(w2) and not om2.exists()
    # what it writes is what the predictors' parser reads
    from glia_amd import hmt as H
    m = H.MLP.from_arrays(None, np.zeros(6), 0, 0, np.array(t[0]), np.array(t[1]))
    m.close()
    assert _run("normalize_sample", "--o", oa).returncode == 1
    assert _run("normalize_sample", "--i", tmp_path / "missing.txt").returncode == 1


def _fnv(h, data):
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & ((1 << 64) - 1)
    return h


CHECK_CASES = [("mlp_3_5_vanilla_fixed", 70, 4, 3, 5, 1, 0.05, 1.0, 0), ("mlp_3_5_adam_adaptive", 70, 4, 3, 5, 2, 0.5, 0.5, 1),
               ("mlp_1_1_momentum", 130, 1, 1, 1, 3, 0.05, 1.0, 0), ("logsig_vanilla_adaptive", 65, 6, 0, 0, 1, 100.0, 0.25, 0),
               ("mlp_32_32_adam", 9, 12, 32, 32, 2, 0.01, 1.0, 1)]


def test_mlp_train_check_digests():
    """the stand-alone host program trains fixed cases by the header alone; its digests are the second author's"""
    r = _run("mlp_train_check")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert lines[-2] == "mlp_train_check: OK"
    got = dict(line.split()[1:3] for line in lines if line.count(" ") == 2)
    assert sorted(got) == sorted(c[0] for c in CHECK_CASES)
    for name, n, dim, n1, n2, opt, step, decay, uss in CHECK_CASES:
        rows = np.array([[((7 * r + 13 * j) % 17 - 8) / 8.0 for j in range(dim)] for r in range(n)])
        labels = np.array([1 if (5 * r) % 7 < 3 else (-1 if (5 * r) % 7 < 6 else 0) for r in range(n)])
        ref = T.train(rows, labels, n1, n2, wr=0.01, ws=1.0, sigma_s=0.5, update_sigma_s=uss, optimizer=opt, step=step, step_decay=decay,
                      max_iterations=4, n_sigma_updates=2, seed=3, fixed_step_decay_iterations=2)
        h = 0xCBF29CE484222325
        for w in ref["round_w"]:
            h = _fnv(h, np.asarray(w, np.float64).tobytes())
        for rec in ref["trace"]:
            h = _fnv(h, np.array(rec[:5], np.float64).tobytes())
        assert got[name] == "%016x" % h, name


REFUSED = [(["--uo", "o.txt"], "--uo"), (["--uf", "f.txt"], "--uf"), (["--wu", "0.5"], "--wu"), (["--bsu", "8"], "--bsu"), (["--bss", "8"], "--bss"),
           (["--bb", "1"], "--bb"), (["--usu", "1"], "--usu")]


@pytest.mark.parametrize("tool", ["train_mlp", "train_logsig"])
def test_usage_and_refused_flags(tool, tmp_path):
    r = _run(tool, "--help")
    assert r.returncode == 1 and r.stderr.startswith("Usage: " + tool) and "--omp" in r.stderr
    assert ("--nn1" in r.stderr) == (tool == "train_mlp")
    base = ["--sl", tmp_path / "l.txt", "--sf", tmp_path / "f.txt", "--omp", tmp_path / "m%d.txt", "--ws", "1", "--ss", "1"]
    for extra, flag in REFUSED:
        r = _run(tool, *(base + extra))
        assert r.returncode == 1 and flag + " is not supported" in r.stderr and tool in r.stderr, (extra, r.stderr)
    # the values at which those flags ask for nothing are taken: the run then fails on the missing files, not on the flag
    r = _run(tool, *(base + ["--wu", "0", "--bss", "-1", "--bb", "0", "--usu", "0"]))
    assert r.returncode == 1 and "cannot open file" in r.stderr and "not supported" not in r.stderr
    r = _run(tool, "--sf", tmp_path / "f.txt", "--omp", "x")
    assert r.returncode == 1 and "'--sl' is required" in r.stderr
    assert _run(tool, "--frobnicate", "1").returncode == 1


def test_a_written_model_parses_back_bit_for_bit(tmp_path):
    from glia_amd import hmt
    rng = np.random.default_rng(6)
    rows = rng.standard_normal((40, 3)) * 1e3
    labels = np.where(rows[:, 1] > 0, 1, -1)
    for n1, n2 in ((4, 3), (0, 0)):
        m = hmt.train_mlp_host(rows, labels, n1, n2, ws=1.0, wr=1e-3, sigma_s=0.3, optimizer=2, step=0.1, max_iterations=3, n_sigma_updates=3,
                               init=rng.standard_normal(_mlpdef.n_weights(3, n1, n2)) * 1e-3)
        assert m.rounds == 3
        for rnd in (0, 1, 2, -1):
            path = tmp_path / ("m_%d_%d.txt" % (n1, rnd))
            m.write(path, rnd)
            assert _mlpdef.same(hmt.mlp_file_parse(path), m.weights(rnd))
            assert len(path.read_text().splitlines()) == m.n_weights
        assert not _mlpdef.same(m.weights(0), m.weights(2))
        # the reference's own form (the stream's default precision, 6 digits) is read too
        p6 = tmp_path / "six.txt"
        p6.write_text("".join("%g\n" % v for v in m.weights()))
        assert np.allclose(hmt.mlp_file_parse(p6), m.weights(), rtol=1e-5, atol=0.0)
        with pytest.raises(hmt.HmtError):
            m.write(tmp_path / "nope" / "m.txt")
        m.close()
