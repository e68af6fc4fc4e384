"""-m gpu: the drop-in tools eval_ri (gadget/main_eval_ri.cxx: -p -r -m -a) and eval_vi (gadget/main_eval_vi.cxx: -p -r -m, plus
--exact) on MetaImage files: stdout token by token against the restatement of tests/_eval_cases.py formatted as std::ostream
prints a double by default (%g), and the error exits."""
import os
import subprocess

import numpy as np
import pytest

import _cc_cases as K
import _eval_cases as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cli")


@pytest.fixture(scope="module")
def tools():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    subprocess.check_call(["make", "-C", CLI])
    return CLI


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    """three image pairs (two 3D of one shape, one 2D) with masks, written once: {"res" | "ref" | "mask": [(file, array)]}"""
    d = tmp_path_factory.mktemp("eval_cli")
    rng = np.random.default_rng(21)
    out = {"res": [], "ref": [], "mask": []}
    for i, shape in enumerate([(12, 18, 20), (12, 18, 20), (33, 31)]):
        ref = rng.integers(0, 6, size=shape).astype(np.uint32)
        res = np.where(rng.random(shape) < 0.7, ref * 3, rng.integers(0, 9, size=shape)).astype(np.uint32)      # mostly agrees with ref
        mask = (rng.random(shape) > 0.25).astype(np.uint32) * 2
        for kind, arr in (("res", res), ("ref", ref), ("mask", mask)):
            path = str(d / ("%s%d.mha" % (kind, i)))
            K.write_mha(path, arr, compress=(i == 1))
            out[kind].append((path, arr))
    return out


def _run(tools, name, images, idx, n_masks=0, flags=()):
    args = [os.path.join(tools, name), "-p"] + [images["res"][i][0] for i in idx] + ["-r"] + [images["ref"][i][0] for i in idx]
    if n_masks:
        args += ["-m"] + [images["mask"][i][0] for i in idx[:n_masks]]
    r = subprocess.run(args + list(flags), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    masks = [images["mask"][i][1] if k < n_masks else None for k, i in enumerate(idx)]
    return r.stdout.split(), ([images["res"][i][1] for i in idx], [images["ref"][i][1] for i in idx], masks)


@pytest.mark.parametrize("idx,n_masks,flags", [((0,), 0, ()), ((0,), 0, ("-a", "0")), ((0,), 1, ("-a", "1")), ((0, 1, 2), 0, ("-a", "0")),
                                               ((0, 1, 2), 2, ()), ((0, 1, 2), 3, ("-a", "0"))])
def test_eval_ri(tools, images, idx, n_masks, flags):
    """one and several image pairs; fewer masks than images are allowed (main_eval_ri.cxx:34); -a 1 is the default"""
    got, vols = _run(tools, "eval_ri", images, idx, n_masks, flags)
    want = E.evaluate(*vols)
    if flags == ("-a", "0"):
        assert got == [E.fmt(want["rand_index"])]
    else:
        assert got == [E.fmt(want["precision"]), E.fmt(want["recall"]), E.fmt(1.0 - want["f1"])]


@pytest.mark.parametrize("idx,n_masks,mode", [((0,), 0, "reference"), ((2,), 1, "exact"), ((0, 1, 2), 0, "exact"), ((0, 1, 2), 3, "reference"),
                                              ((0, 1, 2), 3, "exact")])
def test_eval_vi(tools, images, idx, n_masks, mode):
    got, vols = _run(tools, "eval_vi", images, idx, n_masks, ("--exact", "1") if mode == "exact" else ())
    want = E.evaluate(*vols, mode=mode)
    fs, fm = want["false_split"], want["false_merge"]
    assert got == [E.fmt(fs), E.fmt(fm), E.fmt(fs + fm)]
    other = E.evaluate(*vols, mode="exact" if mode == "reference" else "reference")
    assert E.fmt(other["false_merge"]) != E.fmt(fm)                    # the printed numbers tell the two modes apart


def test_error_exits(tools, images):
    p, r, m = ([f for f, _ in images[k]] for k in ("res", "ref", "mask"))
    for name in ("eval_ri", "eval_vi"):
        exe = os.path.join(tools, name)
        # images of different sizes
        q = subprocess.run([exe, "-p", p[0], "-r", r[2]], capture_output=True, text=True)
        assert q.returncode == 1 and "sizes do not match" in q.stderr and q.stdout == ""
        q = subprocess.run([exe, "-p", p[0], "-r", r[0], "-m", m[2]], capture_output=True, text=True)
        assert q.returncode == 1 and "sizes do not match" in q.stderr and q.stdout == ""
        # different numbers of -p and -r
        q = subprocess.run([exe, "-p", p[0], p[1], "-r", r[0]], capture_output=True, text=True)
        assert q.returncode == 1 and "numbers of proposed and reference images" in q.stderr and q.stdout == ""
        # a required option is missing
        q = subprocess.run([exe, "-p", p[0]], capture_output=True, text=True)
        assert q.returncode == 1 and "refImage" in q.stderr
    # eval_vi reads maskImageFiles[i] for every image once one mask is given (main_eval_vi.cxx:20): another number is refused
    q = subprocess.run([os.path.join(tools, "eval_vi"), "-p", p[0], p[1], "-r", r[0], r[1], "-m", m[0]], capture_output=True, text=True)
    assert q.returncode == 1 and "one mask per image" in q.stderr and q.stdout == ""
