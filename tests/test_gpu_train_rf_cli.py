"""-m gpu: cli/train_rf (ml/rf/main_train_rf.cxx) end to end through the tools on synth 32^3 at S = 8:
merge_order_pb -> bc_feat -> bc_label_ri -> train_rf --nt 5 -> pred_rf with the written model, against train_forest / RandomForest.predict
on the same rows in memory; and the tool's error paths."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cli")


def _write_mha(path, a):
    et = {np.dtype(np.uint32): "MET_UINT", np.dtype(np.float32): "MET_FLOAT"}[a.dtype]
    with open(path, "wb") as f:
        f.write(("ObjectType = Image\nNDims = %d\nBinaryData = True\nBinaryDataByteOrderMSB = False\nDimSize = %s\nElementType = %s\n"
                 "ElementDataFile = LOCAL\n" % (a.ndim, " ".join(str(v) for v in a.shape[::-1]), et)).encode())
        f.write(np.ascontiguousarray(a).tobytes())


def _rows(path):
    return np.array([[float(x) for x in ln.split()] for ln in open(path).read().split("\n") if ln.strip()])


@pytest.fixture(scope="module")
def pipeline(tmp_path_factory):
    """the files of the tools up to bc_label_ri, made once"""
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from oracle import pyoracle as O
    subprocess.check_call(["make", "-C", CLI], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("train_rf")
    p = lambda n: str(d / n)
    shape = (32, 32, 32)
    labels, pb = O.synth(shape, 8, 16)
    z, y, x = np.meshgrid(*[np.arange(n) // 12 for n in shape], indexing="ij")
    truth = ((z * 3 + y) * 3 + x + 1).astype(np.uint32)                     # 12-cubes: a supervoxel of side 8 meets one to a few of them
    _write_mha(p("seg.mha"), labels)
    _write_mha(p("pb.mha"), pb)
    _write_mha(p("truth.mha"), truth)
    run = lambda *argv: subprocess.run([os.path.join(CLI, argv[0])] + list(argv[1:]), capture_output=True, text=True, timeout=120)
    r = run("merge_order_pb", "-s", p("seg.mha"), "-p", p("pb.mha"), "-t", "2", "-o", p("order.txt"))
    assert r.returncode == 0, r.stderr
    r = run("bc_feat", "-s", p("seg.mha"), "-o", p("order.txt"), "--pb", p("pb.mha"), "--rbi", p("pb.mha"), "--rbb", "8", "--rbl", "0", "--rbu", "1",
            "--bt", "0.2", "0.5", "0.8", "-b", p("feats.txt"))
    assert r.returncode == 0, r.stderr
    r = run("bc_label_ri", "-s", p("seg.mha"), "-o", p("order.txt"), "-t", p("truth.mha"), "-l", p("labels.txt"))
    assert r.returncode == 0, r.stderr
    X, y = _rows(p("feats.txt")), _rows(p("labels.txt"))
    assert X.shape[0] == y.shape[0] > 40 and y.shape[1] == 1 and set(y[:, 0]) == {-1.0, 1.0}
    return dict(p=p, run=run, X=X, y=y[:, 0].astype(np.int32))


def test_tools_end_to_end(pipeline):
    from glia_amd import hmt
    p, run, X, y = (pipeline[k] for k in ("p", "run", "X", "y"))
    r = run("train_rf", "--f", p("feats.txt"), "--l", p("labels.txt"), "--nt", "5", "--m", p("model.bin"))
    assert r.returncode == 0, r.stderr
    # --bal defaults to true: the per-class lines of main_train_rf.cxx:57-58
    n_merge, n_split = int((y == -1).sum()), int((y == 1).sum())
    big = max(n_merge, n_split)
    want = ["Class -1: %d [w = %s]" % (n_merge, "%.6g" % (big / n_merge)), "Class 1: %d [w = %s]" % (n_split, "%.6g" % (big / n_split))]
    assert [ln for ln in r.stderr.split("\n") if ln.startswith("Class")] == want
    r = run("pred_rf", "--m", p("model.bin"), "--f", p("feats.txt"), "--l", "-1", "--p", p("pred.txt"))
    assert r.returncode == 0, r.stderr
    ctx = hmt.Context(0)
    model = hmt.train_forest(ctx, X, y, ntree=5)
    pred = model.forest(-1).predict(X)
    assert open(p("pred.txt")).read() == "".join("%.8g\n" % v for v in pred)            # FLT_PREC
    assert len(set(pred.tolist())) > 2 and set(np.round(pred * 5).astype(int).tolist()) <= set(range(6))
    model.write(p("model_py.bin"))
    assert open(p("model_py.bin"), "rb").read() == open(p("model.bin"), "rb").read()
    # the options reach the trainer; files given one by one and through --ff / --ll are concatenated in order
    half = len(X) // 2
    for name, a, b in (("f0.txt", 0, half), ("f1.txt", half, len(X))):
        with open(p(name), "w") as f:
            f.write("\n".join(open(p("feats.txt")).read().split("\n")[a:b]) + "\n")
        with open(p("l" + name[1:]), "w") as f:
            f.write("\n".join(open(p("labels.txt")).read().split("\n")[a:b]) + "\n")
    open(p("ff.txt"), "w").write(p("f1.txt") + "\n")
    open(p("ll.txt"), "w").write(p("l1.txt") + "\n")
    r = run("train_rf", "--f", p("f0.txt"), "--l", p("l0.txt"), "--ff", p("ff.txt"), "--ll", p("ll.txt"), "--nt", "3", "--mt", "4", "--sr", "0.5",
            "--ns", "3", "--bal", "0", "--seed", "77", "--maxdepth", "4", "--m", p("model2.bin"))
    assert r.returncode == 0 and "Class" not in r.stderr, r.stderr
    hmt.train_forest(ctx, X, y, ntree=3, mtry=4, sample_ratio=0.5, nodesize=3, balance=0, seed=77, max_depth=4).write(p("model2_py.bin"))
    assert open(p("model2_py.bin"), "rb").read() == open(p("model2.bin"), "rb").read()
    ctx.close()


def test_error_paths(pipeline):
    p, run = pipeline["p"], pipeline["run"]
    lines = open(p("labels.txt")).read().split("\n")
    open(p("short.txt"), "w").write("\n".join(lines[:-2]) + "\n")
    r = run("train_rf", "--f", p("feats.txt"), "--l", p("short.txt"), "--m", p("bad.bin"))
    assert r.returncode == 1 and "Error: incorrect matrices dimension..." in r.stderr and not os.path.exists(p("bad.bin"))
    open(p("wide.txt"), "w").write("".join(ln + " 1\n" for ln in lines if ln.strip()))
    r = run("train_rf", "--f", p("feats.txt"), "--l", p("wide.txt"), "--m", p("bad.bin"))
    assert r.returncode == 1 and "Error: incorrect matrices dimension..." in r.stderr
    feats = open(p("feats.txt")).read().split("\n")
    row = feats[3].split(" ")
    row[5] = "nan"
    open(p("nan.txt"), "w").write("\n".join(feats[:3] + [" ".join(row)] + feats[4:]))
    r = run("train_rf", "--f", p("nan.txt"), "--l", p("labels.txt"), "--nt", "2", "--m", p("bad.bin"))
    assert r.returncode == 1 and "non-finite value in row 3, column 5" in r.stderr and not os.path.exists(p("bad.bin"))
    r = run("train_rf", "--f", p("feats.txt"), "--l", p("labels.txt"))
    assert r.returncode == 1 and "'--m' is required" in r.stderr
