"""-m gpu: cli/segment_ccm (hmt/main_segment_ccm.cxx) on the 32^3 golden volume: pb-mean merge order -> bc_feat -> forest predictions ->
tree inference -> final label image (-f) and boundary-confidence image (-b).  The tree functions themselves are pinned against the
reference by tests/test_tree_ccm.py; here their results are carried to the volume with NumPy and compared with what the tool writes."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_cli import read_mha, write_mha

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cli")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """volume, order and predicted merge probabilities, their files, and the library's own tree results (full and partial order)"""
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    import _rf
    from glia_amd import hmt
    subprocess.check_call(["make", "-C", CLI])
    tmp = tmp_path_factory.mktemp("ccm")
    g = np.load(os.path.join(ROOT, "tests", "golden", "vol_32.npz"))
    labels = g["labels"].astype(np.uint32)
    pb = (g["pb_q8"].astype(np.float32) / np.float32(256.0)).astype(np.float32)
    ctx = hmt.Context(0)
    d_lab, d_pb = torch.from_numpy(labels.view(np.int32)).cuda(), torch.from_numpy(pb).cuda()
    rm = hmt.RegionMap(ctx, d_lab, pb=d_pb, cfg=hmt.make_config(d_pb, rb=[(d_pb, 8, 0.0, 1.0)]))
    order, _ = rm.merge_order_pb(type=2)
    assert (order == g["pb_mean_order"]).all()
    rows = rm.bc_feat(order)
    model = str(tmp / "model.bin")
    _rf.write_model(model, _rf.random_forest(np.random.default_rng(21), 31, 6, rows))
    clf = hmt.RandomForest(ctx, model)
    probs = clf.predict(rows)
    assert len(np.unique(probs)) > 5
    clf.close()
    rm.close()                                  # a map must not outlive its context
    s = dict(ctx=ctx, labels=labels, tmp=tmp, seg=str(tmp / "seg.mha"))
    write_mha(s["seg"], labels)
    for name, n in (("full", len(order)), ("partial", 40)):
        of, pf = str(tmp / (name + "_order.txt")), str(tmp / (name + "_probs.txt"))
        with open(of, "w") as f:
            for r in order[:n]:
                f.write("%d %d %d\n" % tuple(r))
        with open(pf, "w") as f:
            for v in probs[:n]:
                f.write("%.17g\n" % v)
        lab, par, c0, c1, em, es, Em, Es = hmt.tree_energies(order[:n], probs[:n])
        s[name] = dict(order_f=of, probs_f=pf, lab=lab, par=par, c0=c0, c1=c1, picks=hmt.resolve_tree_ccm(c0, c1, Em, Es),
                       conf=hmt.tree_ccm_confidence(par, c0, c1, es, Em, Es)[2])
    assert 1 < len(s["full"]["picks"]) < 64, "the probabilities should give a segmentation between the trivial ones"
    yield s
    ctx.close()


def _leaves_below(t, i):
    out, stack = [], [int(i)]
    while stack:
        x = stack.pop()
        if t["c0"][x] < 0:
            out.append(int(t["lab"][x]))
        else:
            stack += [int(t["c0"][x]), int(t["c1"][x])]
    return out


def _final(labels, t, ignore=True, mask=None):
    """genFinalSegmentation by hand: the supervoxels below pick k become 1 + k; the others 0 (ignore) or stay; masked-out voxels stay"""
    lut = np.zeros(int(labels.max()) + 1, np.uint32) if ignore else np.arange(int(labels.max()) + 1, dtype=np.uint32)
    for k, p in enumerate(t["picks"]):
        lut[_leaves_below(t, p)] = 1 + k
    out = lut[labels]
    if mask is not None:
        out[mask == 0] = labels[mask == 0]
    return out


def _run(s, which, *extra):
    t = s[which]
    subprocess.check_call([os.path.join(CLI, "segment_ccm"), "-s", s["seg"], "-o", t["order_f"], "-p", t["probs_f"]] + list(extra))


def test_final_segmentation(setup):
    out = str(setup["tmp"] / "final.mha")
    _run(setup, "full", "-f", out)
    got = read_mha(out)
    assert got.dtype == np.uint32 and (got == _final(setup["labels"], setup["full"])).all()
    assert len(np.unique(got)) == len(setup["full"]["picks"])


def test_partial_order_ignore_flag(setup):
    """a partial order's tree is a forest and the resolution starts at its last node: the supervoxels beside it are missing regions"""
    t = setup["partial"]
    covered = sum(len(_leaves_below(t, p)) for p in t["picks"])
    assert 0 < covered < 64
    out = str(setup["tmp"] / "partial.mha")
    _run(setup, "partial", "-f", out)                       # default: -i true
    assert (read_mha(out) == _final(setup["labels"], t, ignore=True)).all() and (read_mha(out) == 0).any()
    _run(setup, "partial", "-i", "0", "-f", out)
    assert (read_mha(out) == _final(setup["labels"], t, ignore=False)).all()


def test_relabel_write16_and_mask(setup):
    from oracle import pyoracle as O
    labels = setup["labels"]
    out = str(setup["tmp"] / "relabel.mha")
    _run(setup, "full", "-r", "1", "-u", "1", "-z", "1", "-f", out)
    ref, _ = O.relabel_image(_final(labels, setup["full"]))
    got = read_mha(out)
    assert got.dtype == np.uint16 and (got == ref).all()
    mask = np.ones(labels.shape, np.uint32)
    mask[:, 5:20, :11] = 0
    maskf = str(setup["tmp"] / "mask.mha")
    write_mha(maskf, mask)
    _run(setup, "full", "-m", maskf, "-f", out)
    assert (read_mha(out) == _final(labels, setup["full"], mask=mask)).all()


def _first_other_neighbour(labels):
    """per voxel the first face neighbour with another label, in the order -x, +x, -y, +y, -z, +z (numpy axes z, y, x); own label if none"""
    nb = labels.copy()
    done = np.zeros(labels.shape, bool)
    for axis, step in ((2, -1), (2, 1), (1, -1), (1, 1), (0, -1), (0, 1)):
        q = np.roll(labels, -step, axis=axis)
        valid = np.ones(labels.shape, bool)
        idx = [slice(None)] * 3
        idx[axis] = 0 if step < 0 else -1
        valid[tuple(idx)] = False
        take = valid & ~done & (q != labels)
        nb[take] = q[take]
        done |= take
    return nb


def test_boundary_confidence_image(setup):
    import torch
    from glia_amd import hmt
    labels, t = setup["labels"], setup["full"]
    out = str(setup["tmp"] / "bc.mha")
    _run(setup, "full", "-b", out)
    got = read_mha(out)
    assert got.dtype == np.float32 and (got > 0).any() and (got[1:-1, 1:-1, 1:-1] == 0).any()
    # the library entry fed the confidence array as the potential
    d_lab = torch.from_numpy(labels.view(np.int32)).cuda()
    rm = hmt.RegionMap(setup["ctx"], d_lab, pb=torch.zeros(labels.shape, dtype=torch.float32, device="cuda"), only_contour=True)
    lib_img = rm.boundary_confidence([(t["lab"], t["par"], t["c0"], t["c1"], t["conf"])]).cpu().numpy()
    assert (got == lib_img).all()
    # brute force (genBoundaryConfidenceMap, hmt/tree_segment.hxx:66-143): a voxel belongs to the directed pair (its label, its first
    # other neighbour).  A region still holds the entry a -> b while a is inside it and b is not -- the nodes from a up to below the lowest
    # common ancestor -- and, if no voxel of b has a for its first other neighbour, b -> a does not exist, nothing cancels a -> b and every
    # ancestor of a holds it.  The pair's value, shared by both directions, is the largest float confidence over those nodes.
    leaf = {int(t["lab"][i]): i for i in range(len(t["lab"])) if t["c0"][i] < 0}
    conf32 = t["conf"].astype(np.float32)

    def path(i):
        p = [i]
        while t["par"][p[-1]] >= 0:
            p.append(int(t["par"][p[-1]]))
        return p

    def value(a, b, mutual):
        pa_, pb_ = path(leaf[a]), path(leaf[b])
        common = set(pa_) & set(pb_)
        v = max(conf32[x] for x in pa_ + pb_ if x not in common) if mutual else max(conf32[x] for x in pa_)
        return v if v > 0 else np.float32(0)

    nb = _first_other_neighbour(labels)
    want = np.zeros(labels.shape, np.float32)
    pairs = np.unique(np.stack([labels[nb != labels], nb[nb != labels]], axis=1), axis=0)
    directed = set(map(tuple, pairs.tolist()))
    assert any((b, a) not in directed for a, b in directed) and any((b, a) in directed for a, b in directed)
    for a, b in directed:
        want[(labels == a) & (nb == b)] = value(a, b, (b, a) in directed)
    assert (got == want).all()


def test_usage_errors(setup):
    r = subprocess.run([os.path.join(CLI, "segment_ccm"), "-s", setup["seg"], "-o", setup["full"]["order_f"], "-f", "x.mha"], capture_output=True)
    assert r.returncode == 1 and b"'--mergeProbs' is required" in r.stderr
    short = str(setup["tmp"] / "short.txt")
    with open(short, "w") as f:
        f.write("0.5\n")
    r = subprocess.run([os.path.join(CLI, "segment_ccm"), "-s", setup["seg"], "-o", setup["full"]["order_f"], "-p", short, "-f", "x.mha"],
                       capture_output=True)
    assert r.returncode == 1 and b"too few merge probabilities" in r.stderr
