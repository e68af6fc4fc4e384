"""-m gpu: the drop-in tools cli/pred_mlp and cli/pred_logsig (sshmt/main_pred_mlp.cxx, sshmt/main_pred_logsig.cxx) on written feature
files.  Every output line is '%g' of the probability the second author computes (tests/_mlpdef.py): writeData without a precision
argument writes 6 significant digits."""
import os
import subprocess

import numpy as np
import pytest

import _mlpdef as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cli")


def _run(tool, *args):
    return subprocess.run([os.path.join(CLI, tool)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def _lines(path):
    with open(path) as f:
        return f.read().split("\n")


def _expect(p):
    return ["%g" % v for v in p] + [""]         # every value is followed by the delimiter


def test_pred_mlp(tmp_path):
    w, rows, mn, mx = D.random_case(104, 10, 10, n_rows=300)
    model, fmm = tmp_path / "model.txt", tmp_path / "minmax.txt"
    D.write_values(model, w)
    D.write_rows(fmm, [mn, mx])
    f1, f2, f3 = tmp_path / "a.txt", tmp_path / "b.txt", tmp_path / "empty.txt"
    D.write_rows(f1, rows[:200])
    D.write_rows(f2, rows[200:])
    f3.write_text("")
    p1, p2, p3 = tmp_path / "pa.txt", tmp_path / "pb.txt", tmp_path / "pe.txt"
    # two files and an empty one in one call, no rescale
    r = _run("pred_mlp", "--m", model, "--f", f1, f2, f3, "--nn1", 10, "--nn2", 10, "--p", p1, p2, p3)
    assert r.returncode == 0, r.stderr
    want = D.sigmoid(D.logits(w, 10, 10, rows))
    assert _lines(p1) == _expect(want[:200]) and _lines(p2) == _expect(want[200:]) and _lines(p3) == [""]
    assert len(set(_lines(p1))) > 100
    # --fmm
    r = _run("pred_mlp", "--m", model, "--fmm", fmm, "--f", f1, "--nn1", 10, "--nn2", 10, "--p", p1)
    assert r.returncode == 0, r.stderr
    assert _lines(p1) == _expect(D.sigmoid(D.logits(w, 10, 10, rows[:200], mn, mx)))


def test_pred_mlp_three_models(tmp_path):
    ws, rows, mn, mx = D.random_case(7, 3, 17, n_rows=120, n_models=3)
    models = []
    for i, w in enumerate(ws):
        models.append(tmp_path / ("model%d.txt" % i))
        D.write_values(models[-1], w)
    fmm, feats, preds = tmp_path / "minmax.txt", tmp_path / "f.txt", tmp_path / "p.txt"
    D.write_rows(fmm, [mn, mx])
    D.write_rows(feats, rows)
    for mm, opt in (((None, None), []), ((mn, mx), ["--fmm", fmm])):
        lg, picks = D.logits(ws, 3, 17, rows, *mm, dist=D.DIST, want_pick=True)
        assert np.bincount(picks, minlength=3).min() >= 5
        r = _run("pred_mlp", "--m", *models, "--md", *D.DIST, *opt, "--f", feats, "--nn1", 3, "--nn2", 17, "--p", preds)
        assert r.returncode == 0, r.stderr
        assert _lines(preds) == _expect(D.sigmoid(lg))
    # a negative threshold is a value, not an option
    r = _run("pred_mlp", "--m", *models, "--md", 3, 1, -0.5, "--f", feats, "--nn1", 3, "--nn2", 17, "--p", preds)
    assert r.returncode == 0, r.stderr
    assert _lines(preds) == _expect(D.sigmoid(D.logits(ws, 3, 17, rows, dist=(3, 1, -0.5))))


def test_pred_logsig(tmp_path):
    w, rows, _, _ = D.random_case(104, 0, 0, n_rows=150)
    model = tmp_path / "model.txt"
    D.write_values(model, w)
    f1, f2, f3 = tmp_path / "a.txt", tmp_path / "b.txt", tmp_path / "empty.txt"
    D.write_rows(f1, rows[:100])
    D.write_rows(f2, rows[100:])
    f3.write_text("")
    p1, p2, p3 = tmp_path / "pa.txt", tmp_path / "pb.txt", tmp_path / "pe.txt"
    r = _run("pred_logsig", "--m", model, "--f", f1, f2, f3, "--p", p1, p2, p3)
    assert r.returncode == 0, r.stderr
    want = D.sigmoid(D.logits(w, 0, 0, rows))
    assert _lines(p1) == _expect(want[:100]) and _lines(p2) == _expect(want[100:]) and _lines(p3) == [""]


def test_usage_errors(tmp_path):
    w, rows, _, _ = D.random_case(7, 3, 17, n_rows=5)
    model, feats, preds = tmp_path / "model.txt", tmp_path / "f.txt", tmp_path / "p.txt"
    D.write_values(model, w)
    D.write_rows(feats, rows)
    full = {"--m": [model], "--f": [feats], "--nn1": [3], "--nn2": [17], "--p": [preds]}
    for missing in full:
        args = [x for k, v in full.items() if k != missing for x in [k] + v]
        r = _run("pred_mlp", *args)
        assert r.returncode == 1 and "required but missing" in r.stderr and "Usage: pred_mlp" in r.stderr, (missing, r.stderr)
    for md in ([], ["--md", 3, 1]):
        r = _run("pred_mlp", "--m", model, model, model, *md, "--f", feats, "--nn1", 3, "--nn2", 17, "--p", preds)
        assert r.returncode == 1 and "Error: model distributor needs 3 arguments..." in r.stderr
    r = _run("pred_mlp", "--m", model, "--f", feats, "--nn1", 4, "--nn2", 17, "--p", preds)        # no whole D: refused, not truncated
    assert r.returncode == 1 and "do not fit" in r.stderr
    r = _run("pred_mlp", "--m", model, "--f", feats, feats, "--nn1", 3, "--nn2", 17, "--p", preds)
    assert r.returncode == 1 and "fewer prediction files" in r.stderr
    full = {"--m": [model], "--f": [feats], "--p": [preds]}
    for missing in full:
        args = [x for k, v in full.items() if k != missing for x in [k] + v]
        r = _run("pred_logsig", *args)
        assert r.returncode == 1 and "required but missing" in r.stderr and "Usage: pred_logsig" in r.stderr, (missing, r.stderr)
    r = _run("pred_logsig", "--m", model, "--f", feats, "--p", preds)                              # rows of 7 columns, a model for more
    assert r.returncode == 1 and "columns" in r.stderr
