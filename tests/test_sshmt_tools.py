"""The tools around the merge-path term, without a GPU: cli/sshmt_check's digests against the second author (tests/_sshmtdef.py), and
the usage and refusals of cli/train_sshmt_mlp and cli/train_sshmt_logsig.  (The tools have no host switch, as train_mlp has none: their
runs on files are tests/test_gpu_sshmt_cli.py's.)"""
import os
import subprocess

import numpy as np
import pytest

import _sshmt_cases as K
import _sshmtdef as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cli")


def _run(tool, *args):
    return subprocess.run([os.path.join(CLI, tool)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def _fnv(h, data):
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & ((1 << 64) - 1)
    return h


# name, labelled rows, columns, n1, n2, optimizer, step, decay, update_sigma_u, tree (0: caterpillar of 67, else balanced levels), max, min, ws
CHECK_CASES = [("mlp_3_5_vanilla_fixed_cat", 70, 4, 3, 5, 1, 0.05, 1.0, 0, 0, 3, 2, 1.0), ("mlp_3_5_adam_adaptive_bal", 70, 4, 3, 5, 2, 0.5, 0.5, 1, 5, 3, 2, 1.0),
               ("mlp_1_1_momentum_len8", 130, 1, 1, 1, 3, 0.05, 1.0, 0, 0, 8, 2, 1.0), ("logsig_vanilla_adaptive_len1", 65, 6, 0, 0, 1, 100.0, 0.25, 0, 4, 1, 1, 1.0),
               ("mlp_32_32_adam_wu_alone", 9, 12, 32, 32, 2, 0.01, 1.0, 1, 6, 2, 1, 0.0)]


def test_sshmt_check_digests():
    """the stand-alone host program trains fixed cases by the header alone; its digests are the second author's"""
    r = _run("sshmt_check")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert lines[-2] == "sshmt_check: OK"
    got = dict(line.split()[1:3] for line in lines if line.count(" ") == 2)
    assert sorted(got) == sorted(c[0] for c in CHECK_CASES)
    for name, n, dim, n1, n2, opt, step, decay, usu, tree, mx, mn, ws in CHECK_CASES:
        rows = np.array([[((7 * r + 13 * j) % 17 - 8) / 8.0 for j in range(dim)] for r in range(n)])
        labels = np.array([1 if (5 * r) % 7 < 3 else (-1 if (5 * r) % 7 < 6 else 0) for r in range(n)])
        order = K.balanced(tree) if tree else K.caterpillar(67)
        urows = np.array([[((5 * r + 11 * j) % 19 - 9) / 9.0 for j in range(dim)] for r in range(len(order))])
        ref = S.train(rows, labels, [(urows, order)], n1, n2, wr=0.01, ws=ws, wu=0.5, sigma_s=0.5, sigma_u=0.7, update_sigma_u=usu, optimizer=opt,
                      step=step, step_decay=decay, max_iterations=4, n_sigma_updates=2, seed=3, fixed_step_decay_iterations=2,
                      max_path_length=mx, min_path_length=mn)
        h = 0xCBF29CE484222325
        for w in ref["round_w"]:
            h = _fnv(h, np.asarray(w, np.float64).tobytes())
        for rec in ref["trace"]:
            h = _fnv(h, np.array(rec[:5], np.float64).tobytes())
        h = _fnv(h, np.array(ref["sigma_u2"], np.float64).tobytes())
        h = _fnv(h, np.array(ref["sigma_u2_eval"], np.float64).tobytes())
        assert got[name] == "%016x" % h, name


REFUSED = [(["--bsu", "8"], "--bsu"), (["--bss", "8"], "--bss"), (["--bb", "1"], "--bb"), (["--te", "2"], "--te"), (["--tb", "4"], "--tb")]


@pytest.mark.parametrize("tool", ["train_sshmt_mlp", "train_sshmt_logsig"])
def test_usage_and_refused_flags(tool, tmp_path):
    r = _run(tool, "--help")
    assert r.returncode == 1 and r.stderr.startswith("Usage: " + tool) and "--omp" in r.stderr and "--uo" in r.stderr and "--wu" in r.stderr
    assert ("--nn1" in r.stderr) == (tool == "train_sshmt_mlp")
    base = ["--sl", tmp_path / "l.txt", "--sf", tmp_path / "f.txt", "--uo", tmp_path / "o.txt", "--uf", tmp_path / "u.txt", "--omp", tmp_path / "m%d.txt",
            "--ws", "1", "--ss", "1", "--wu", "1", "--su", "1"]
    for extra, flag in REFUSED:
        r = _run(tool, *(base + extra))
        assert r.returncode == 1 and flag + " is not supported" in r.stderr and tool in r.stderr, (extra, r.stderr)
    # the values at which those flags ask for nothing are taken: the run then fails on the missing files, not on the flag
    r = _run(tool, *(base + ["--bsu", "-1", "--bss", "-1", "--bb", "0", "--te", "1", "--tb", "1", "--usu", "1"]))
    assert r.returncode == 1 and "not supported" not in r.stderr and ("cannot open file" in r.stderr or "invalid data file" in r.stderr), r.stderr
    r = _run(tool, "--uo", tmp_path / "o.txt", "--omp", "x", "--wu", "1", "--su", "1")
    assert r.returncode == 1 and "--uo and --uf must come in equal numbers (1 and 0)" in r.stderr
    r = _run(tool, "--uo", tmp_path / "o.txt", "--uf", tmp_path / "u.txt", "--omp", "x", "--ws", "1", "--ss", "1")
    assert r.returncode == 1 and "--sl and --sf are required unless --ws is 0" in r.stderr
    r = _run(tool, "--uo", tmp_path / "o.txt", "--uf", tmp_path / "u.txt")
    assert r.returncode == 1 and "'--omp' is required" in r.stderr
    assert _run(tool, "--frobnicate", "1").returncode == 1
