"""-m gpu: merge_order_bc --bct 2 (hmt/main_merge_order_bc.cxx:111-139) writes the order, saliency and -b files the library call
gives, with one model and with three; its refusals carry the reference's messages."""
import os
import subprocess

import numpy as np
import pytest

import _mlpdef
from test_gpu_cli import _g, write_mha

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cli")
COMMON = ["--rbb", "8", "--rbl", "0.0", "--rbu", "1.0", "--bt", "0.2", "0.5", "0.8", "-n", "0", "-l", "0"]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """a 32^3 synth volume as files and on the device, the rows of the stub scorer's run, and a context"""
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    from oracle import pyoracle as O
    subprocess.check_call(["make", "-C", CLI], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("bc_mlp_cli")
    labels, pb = O.synth((32, 32, 32), 8, 16)
    seg, pbf = str(d / "seg.mha"), str(d / "pb.mha")
    write_mha(seg, labels)
    write_mha(pbf, pb)
    ctx = hmt.Context(0)
    d_lab, d_pb = torch.from_numpy(labels.view(np.int32)).cuda(), torch.from_numpy(pb).cuda()
    rm = hmt.RegionMap(ctx, d_lab, pb=d_pb, cfg=hmt.make_config(d_pb, rb=[(d_pb, 8, 0.0, 1.0)]))
    _, _, f0 = rm.merge_order_bc(hmt.FeatureStubClassifier(ctx, 31), want_feats=True)
    yield dict(dir=d, seg=seg, pb=pbf, ctx=ctx, rm=rm, f0=f0, dim=rm.feat_dim())
    rm.close()
    ctx.close()


def _run(case, extra, check=True):
    order_f, sal_f, feat_f = (str(case["dir"] / n) for n in ("order.txt", "sal.txt", "bfeat.txt"))
    cmd = [os.path.join(CLI, "merge_order_bc")] + extra + ["-s", case["seg"], "--pb", case["pb"], "--rbi", case["pb"]] + COMMON + \
          ["-o", order_f, "--sal", sal_f, "-b", feat_f]
    r = subprocess.run(cmd, capture_output=True, timeout=120)
    if check:
        assert r.returncode == 0, r.stderr.decode()
    return r, order_f, sal_f, feat_f


def _files_are(order_f, sal_f, feat_f, o, s, f):
    assert (np.loadtxt(order_f, dtype=np.int64).reshape(-1, 3) == o).all()
    assert open(sal_f).read().split("\n")[:-1] == [_g(v) for v in s]
    rows = [ln.split(" ") for ln in open(feat_f).read().split("\n")[:-1]]
    assert len(rows) == len(f) and all(r[-1] == "" and len(r) == f.shape[1] + 1 for r in rows)
    got = np.array([[float(x) for x in r[:-1]] for r in rows])
    assert np.allclose(got, f, rtol=6e-8, atol=1e-12)            # FLT_PREC = 8 significant digits


def _minmax(case):
    f0 = case["f0"]
    mn, mx = f0.min(0) - 0.25, f0.max(0) + 0.25
    path = str(case["dir"] / "minmax.txt")
    _mlpdef.write_rows(path, [mn, mx])
    return path, mn, mx


def test_one_model(case):
    from glia_amd import hmt
    rng = np.random.default_rng(71)
    w = rng.standard_normal(_mlpdef.n_weights(case["dim"], 10, 10)) * 0.4
    model = str(case["dir"] / "mlp.txt")
    _mlpdef.write_values(model, w)
    fmm, mn, mx = _minmax(case)
    # --nn1 / --nn2 default to 10 and 10
    _, order_f, sal_f, feat_f = _run(case, ["--bct", "2", "--bcm", model, "--bcfmm", fmm])
    clf = hmt.MLP(case["ctx"], model, 10, 10, minmax=fmm)
    o, s, f = case["rm"].merge_order_bc(clf, want_feats=True)
    clf.close()
    assert len(o) == 63 and len(np.unique(s)) > 8
    _files_are(order_f, sal_f, feat_f, o, s, f)
    # without the min/max file the rows are not rescaled: another order file, the library's again
    _, order_f, sal_f, feat_f = _run(case, ["--bct", "2", "--nn1", "10", "--nn2", "10", "--bcm", model])
    clf = hmt.MLP(case["ctx"], model, 10, 10)
    o2, s2, f2 = case["rm"].merge_order_bc(clf, want_feats=True)
    clf.close()
    _files_are(order_f, sal_f, feat_f, o2, s2, f2)
    assert s2.tobytes() != s.tobytes()


def test_three_models(case):
    from glia_amd import hmt
    rng = np.random.default_rng(73)
    fmm, mn, mx = _minmax(case)
    models = []
    for k in range(3):
        models.append(str(case["dir"] / ("mlp%d.txt" % k)))
        _mlpdef.write_values(models[-1], rng.standard_normal(_mlpdef.n_weights(case["dim"], 7, 12)) * 0.4)
    x = _mlpdef.prepare(case["f0"], mn, mx)
    dim0, dim1 = 31, 26
    thr = float(np.median(np.concatenate([x[:, dim0], x[:, dim1]])))
    args = ["--bct", "2", "--nn1", "7", "--nn2", "12", "--bcm", models[0], "--bcm", models[1], "--bcm", models[2], "--bcfmm", fmm]
    _, order_f, sal_f, feat_f = _run(case, args + ["--bcmd", str(dim0), "--bcmd", str(dim1), "--bcmd", repr(thr)])
    clf = hmt.MLP(case["ctx"], models, 7, 12, minmax=fmm, distributor_args=(dim0, dim1, thr))
    o, s, f = case["rm"].merge_order_bc(clf, want_feats=True)
    clf.close()
    _files_are(order_f, sal_f, feat_f, o, s, f)
    # three models, or two, without the distributor arguments: the reference's message (:117-118) and exit code
    r, _, _, _ = _run(case, args, check=False)
    assert r.returncode == 1 and b"model distributor needs 3 arguments" in r.stderr
    r, _, _, _ = _run(case, ["--bct", "2", "--bcm", models[0], "--bcm", models[1]], check=False)
    assert r.returncode == 1 and b"model distributor needs 3 arguments" in r.stderr


def test_other_classifier_types_keep_their_message(case):
    r, _, _, _ = _run(case, ["--bct", "3", "--bcm", "nothing"], check=False)
    assert r.returncode == 1 and b"unsupported classifier type" in r.stderr
