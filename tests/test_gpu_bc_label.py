"""-m gpu: RegionMap.bc_label / cli bc_label_ri, bc_label_vi (hmt/main_bc_label_ri.cxx, main_bc_label_vi.cxx) against a
brute-force NumPy restatement.  The restatement builds the contingency table of every listed region from the voxel arrays, one
merge at a time (stats::pairStats / pairF1 / randIndex / vi, util/image_stats.hxx:69-110,173-245, util/stats.hxx:189-261), so
it checks the per-node reduction of the library as well as the rules.  The reference's tools cannot be built here (int512_t
needs Boost.Multiprecision): parity rests on this restatement, not on recorded reference runs."""
import os
import subprocess
import tempfile
from collections import deque

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEPS = 2.22e-16
MERGE, SPLIT = -1, 1
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    yield c
    c.close()


# ---- the synth truth cells (glia_amd/csrc/synth.hip, CellGrid with the truth salt), restated in NumPy ----
def _splitmix(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15)) & np.uint64(M64)
    z = x
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def truth_cells(shape, G, seed=0x9E3779B97F4A7C15):
    with np.errstate(over="ignore"):
        D = len(shape)
        n = list(shape[::-1]) + ([1] if D == 2 else [])
        nc = [(v + G - 1) // G for v in n]
        if D == 2:
            nc[2] = 1
        z, y, x = np.meshgrid(*[np.arange(v, dtype=np.int64) for v in n[::-1]], indexing="ij")
        cx, cy, cz = x // G, y // G, (z // G if D == 3 else np.zeros_like(z))
        best = np.full(x.shape, np.iinfo(np.int64).max, np.int64)
        bid = np.zeros(x.shape, np.uint32)
        salt = np.uint64(seed) ^ np.uint64(0x54525554)
        for dz in ((-1, 0, 1) if D == 3 else (0,)):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ex, ey, ez = cx + dx, cy + dy, cz + dz
                    ok = (ex >= 0) & (ey >= 0) & (ez >= 0) & (ex < nc[0]) & (ey < nc[1]) & (ez < nc[2])
                    lin = (ex + nc[0] * (ey + nc[1] * ez)).astype(np.uint64)
                    h = _splitmix(salt ^ _splitmix(lin))
                    q0 = ex * G + ((h & np.uint64(0xFFFF)) % np.uint64(G)).astype(np.int64)
                    q1 = ey * G + (((h >> np.uint64(16)) & np.uint64(0xFFFF)) % np.uint64(G)).astype(np.int64)
                    q2 = ez * G + (((h >> np.uint64(32)) & np.uint64(0xFFFF)) % np.uint64(G)).astype(np.int64) if D == 3 else 0
                    d = (q0 - x) ** 2 + (q1 - y) ** 2 + (q2 - z) ** 2
                    idv = (ex + nc[0] * (ey + nc[1] * ez)).astype(np.uint32)
                    better = ok & ((d < best) | ((d == best) & (idv < bid)))
                    best = np.where(better, d, best)
                    bid = np.where(better, idv, bid)
        return bid.reshape(shape)


# ---- brute-force restatement ----
def _cmap(regions, truth):
    """{(list index, truth label): count} of the listed voxel sets, truth 0 excluded"""
    out = {}
    for i, vox in enumerate(regions):
        t = truth[vox]
        t = t[t != 0]
        u, c = np.unique(t, return_counts=True)
        for a, b in zip(u.tolist(), c.tolist()):
            out[(i, a)] = b
    return out


def pair_stats(regions, truth):
    cm = _cmap(regions, truth)
    n = sum(cm.values())
    tp = sum(c * (c - 1) // 2 for c in cm.values())
    k0, k1 = {}, {}
    for (i, t), c in cm.items():
        k0[i] = k0.get(i, 0) + c
        k1[t] = k1.get(t, 0) + c
    p0 = sum(v * (v - 1) // 2 for v in k0.values())
    p1 = sum(v * (v - 1) // 2 for v in k1.values())
    npair = n * (n - 1) // 2
    return tp, npair - p1 + tp - p0, p0 - tp, p1 - tp


def _div(num, den):
    return num / (den if not abs(den - 0.0) < FEPS else den + FEPS)


def pair_f1(regions, truth):
    tp, tn, fp, fn = pair_stats(regions, truth)
    prec = _div(float(tp), float(tp + fp))
    rec = _div(float(tp), float(tp + fn))
    f = 2.0 * prec * rec / (prec + rec) if prec + rec != 0 else float("nan")     # 0 / 0 = NaN in C++
    return f, prec, rec


def rand_index(regions, truth):
    tp, tn, fp, fn = pair_stats(regions, truth)
    num = float(tp + tn)
    den = float(fp + fn)
    den += num
    return _div(num, den)


def vi(regions, truth):
    npoint = sum(len(v) for v in regions)
    cm = _cmap(regions, truth)
    ncount = [0] * len(regions)
    tcount = {}
    for (i, t), c in cm.items():
        ncount[i] += c
        tcount[t] = tcount.get(t, 0) + c
    ret = 0.0
    for (i, t), c in sorted(cm.items()):
        ret += c * (np.log2(float(tcount[t])) + np.log2(float(ncount[i])) - 2.0 * np.log2(float(c)))
    return ret / npoint


def majority(x):
    pos = sum(1 for v in x if v == SPLIT)
    if 2 * pos == len(x):
        return -x[0]
    return SPLIT if 2 * pos > len(x) else MERGE


class Ref:
    """voxel index arrays of every key of RegionMap(seg, mask, order, false), built merge by merge"""

    def __init__(self, labels, order, mask=None):
        flat = labels.reshape(-1)
        keep = np.ones(flat.shape, bool) if mask is None else (mask.reshape(-1) != 0)
        idx = np.nonzero(keep)[0]
        lab = flat[idx]
        o = np.argsort(lab, kind="stable")
        u, first = np.unique(lab[o], return_index=True)
        bounds = list(first) + [len(o)]
        self.vox = {int(k): idx[o[bounds[j]:bounds[j + 1]]] for j, k in enumerate(u.tolist())}
        self.order = [tuple(int(v) for v in r) for r in np.asarray(order).reshape(-1, 3)]
        for x0, x1, x2 in self.order:
            self.vox[x2] = np.concatenate([self.vox[x0], self.vox[x1]])

    def regions(self, keys):
        return [self.vox[k] for k in keys]

    def labels(self, truths, metric="f1", tweak=False, mpd=1.0, opt_split=False, opt=0, gaps=None):
        truths = [t.reshape(-1) for t in truths]
        T = truths[0]
        n = len(self.order)
        if opt == 0 and metric == "vi":
            out = []
            for x0, x1, x2 in self.order:
                tmp = []
                for t in truths:
                    m, s = vi(self.regions([x2]), t), vi(self.regions([x0, x1]), t)
                    if gaps is not None:
                        gaps.append((m, s, _nonempty(self.regions([x0, x1]), t) <= 1))
                    tmp.append(MERGE if m < s else SPLIT)
                out.append(majority(tmp))
            return out
        if opt == 0 and metric == "ri":
            return [MERGE if rand_index(self.regions([x2]), T) > rand_index(self.regions([x0, x1]), T) else SPLIT
                    for x0, x1, x2 in self.order]
        if opt == 0:
            out, mf1 = [], []
            for x0, x1, x2 in self.order:
                sf, sp, sr = pair_f1(self.regions([x0, x1]), T)
                mf, mp, mr = pair_f1(self.regions([x2]), T)
                mf1.append(mf)
                if mpd < 1.0 and sp - mp > mpd:
                    out.append(SPLIT)
                elif tweak:
                    out.append(MERGE if (mf > sf or (sp < FEPS and sr < FEPS and mp < FEPS and mr < FEPS) or
                                         (sf == mf and sp > 0.9 and mp > 0.9)) else SPLIT)
                else:
                    out.append(MERGE if mf > sf else SPLIT)
            if opt_split:
                smap = {}
                for i, (x0, x1, x2) in enumerate(self.order):
                    split = smap.get(x0, [x0]) + smap.get(x1, [x1])
                    if out[i] == SPLIT:
                        smap[x2] = split
                    elif mf1[i] > pair_f1(self.regions(split), T)[0]:
                        smap[x2] = [x2]
                    else:
                        out[i] = SPLIT
                        smap[x2] = split
            return out
        # genTree: leaves on first sight, then the merge node (hmt/tree_build.hxx:12-38)
        nodes, node_of = [], {}
        for x0, x1, x2 in self.order:
            for k in (x0, x1):
                if k not in node_of:
                    node_of[k] = len(nodes)
                    nodes.append({"key": k, "ch": [], "par": -1})
            me = len(nodes)
            nodes.append({"key": x2, "ch": [node_of[x0], node_of[x1]], "par": -1})
            nodes[node_of[x0]]["par"] = nodes[node_of[x1]]["par"] = me
            node_of[x2] = me
        for i, nd in enumerate(nodes):
            if not nd["ch"]:
                nd["lab"], nd["best"] = MERGE, [i]
                continue
            split = [j for c in nd["ch"] for j in nodes[c]["best"]]
            sreg = self.regions([nodes[j]["key"] for j in split])
            mreg = self.regions([nd["key"]])
            if metric == "vi":
                tmp = []
                for t in truths:
                    m, s = vi(mreg, t), vi(sreg, t)
                    if gaps is not None:
                        gaps.append((m, s, _nonempty(sreg, t) <= 1))
                    tmp.append(MERGE if m < s else SPLIT)
                merge = majority(tmp) == MERGE
            else:
                merge = pair_f1(mreg, T)[0] > pair_f1(sreg, T)[0]
            nd["lab"], nd["best"] = (MERGE, [i]) if merge else (SPLIT, split)
        if opt == 1 and nodes:
            q = deque([len(nodes) - 1])
            while q:
                i = q.popleft()
                if nodes[i]["lab"] == MERGE:
                    st = [i]
                    while st:
                        j = st.pop()
                        nodes[j]["lab"] = MERGE
                        st.extend(nodes[j]["ch"])
                else:
                    q.extend(nodes[i]["ch"])
        elif opt == 2:
            for nd in nodes:
                if nd["lab"] == SPLIT:
                    p = nd["par"]
                    while p >= 0:
                        nodes[p]["lab"] = SPLIT
                        p = nodes[p]["par"]
        out = [nd["lab"] for nd in nodes if nd["ch"]]
        assert len(out) == n
        return out


def _nonempty(regions, truth):
    return sum(1 for v in regions if (truth[v] != 0).any())


def _no_near_ties(gaps):
    """VI values are sums in another order than the reference's hash order: only labels can be exact, so no compared pair may
    lie within 1e-12 of a tie -- except the structural ties where at most one listed region meets a truth label: the split list
    then has the merged region's contingency table, both sides evaluate the same terms and compare equal (label SPLIT)"""
    for m, s, structural in gaps:
        if structural:
            assert m == s, (m, s)
            continue
        assert abs(m - s) > 1e-12 * max(abs(m), abs(s)), (m, s)


# ---- volumes ----
def _case(ctx, shape, S, G, erase=False, mask=False, seed=0x9E3779B97F4A7C15):
    import torch
    from glia_amd import hmt
    from oracle import pyoracle as O
    labels, pb = O.synth(shape, S, G, seed=seed)
    truth = truth_cells(shape, G, seed=seed).astype(np.uint32) + 1
    rng = np.random.default_rng(7)
    if erase:
        truth = truth.copy()
        truth[rng.random(shape) < 0.3] = 0
        truth[tuple(slice(0, v // 3) for v in shape)] = 0
    m = None
    if mask:
        m = (rng.random(shape) > 0.1).astype(np.uint32)
        m[tuple(slice(v // 2, v // 2 + 2) for v in shape)] = 0
    d_lab = torch.from_numpy(labels.view(np.int32)).cuda()
    d_pb = torch.from_numpy(pb).cuda()
    d_m = None if m is None else torch.from_numpy(m.view(np.int32)).cuda()
    rm = hmt.RegionMap(ctx, d_lab, pb=d_pb, mask=d_m)
    rm._bcl_keep = (d_lab, d_pb, d_m)
    return rm, labels, pb, truth, m


def _dt(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


VOLS = [((28, 26, 24), 4, 10, False, False), ((96, 88), 4, 20, False, False), ((28, 26, 24), 4, 10, True, False),
        ((26, 24, 22), 4, 9, False, True), ((80, 72), 4, 16, True, True)]
VARIANTS = [dict(metric="f1"), dict(metric="f1", tweak=True), dict(metric="f1", mpd=0.05), dict(metric="f1", tweak=True, mpd=0.2),
            dict(metric="f1", opt_split=True), dict(metric="ri"), dict(metric="vi"),
            dict(metric="f1", opt=1), dict(metric="f1", opt=2), dict(metric="ri", opt=1), dict(metric="vi", opt=1), dict(metric="vi", opt=2)]


@pytest.mark.parametrize("shape,S,G,erase,mask", VOLS)
def test_labels_match_restatement(ctx, shape, S, G, erase, mask):
    from glia_amd import hmt
    rm, labels, pb, truth, m = _case(ctx, shape, S, G, erase=erase, mask=mask)
    dt = _dt(truth)
    for typ in (1, 2):
        order, _ = rm.merge_order_pb(type=typ)
        assert len(order) > 20
        ref = Ref(labels, order, m)
        for kw in VARIANTS:
            gaps = [] if kw["metric"] == "vi" else None
            want = ref.labels([truth], gaps=gaps, **kw)
            got = rm.bc_label(dt, order, **kw)
            assert got.tolist() == want, (typ, kw)
            if gaps is not None:
                _no_near_ties(gaps)
        # a prefix of the order, and no merge at all
        k = len(order) // 3
        assert rm.bc_label(dt, order[:k]).tolist() == ref.labels([truth])[:k]
        assert rm.bc_label(dt, order[:0]).shape == (0,)
        assert rm.bc_label(dt, order[:k], metric="vi", opt=2).tolist() == Ref(labels, order[:k], m).labels([truth], metric="vi", opt=2)
    assert hmt.Context.internal_errors() == 0


def test_labels_of_classifier_order(ctx):
    import torch
    from glia_amd import hmt
    from oracle import pyoracle as O
    shape, S, G = (28, 26, 24), 4, 10
    labels, pb = O.synth(shape, S, G)
    d_lab = torch.from_numpy(labels.view(np.int32)).cuda()
    d_pb = torch.from_numpy(pb).cuda()
    cfg = hmt.make_config(d_pb, rb=[(d_pb, 8, 0.0, 1.0)], thresholds=(0.2, 0.5, 0.8))
    rm = hmt.RegionMap(ctx, d_lab, pb=d_pb, cfg=cfg)
    order, _ = rm.merge_order_bc(hmt.FeatureStubClassifier(ctx, 11 + 4 * 3 + 7 + 1))
    truth = truth_cells(shape, G).astype(np.uint32) + 1
    ref = Ref(labels, order)
    dt = _dt(truth)
    for kw in VARIANTS:
        assert rm.bc_label(dt, order, **kw).tolist() == ref.labels([truth], **kw), kw


@pytest.mark.parametrize("nt", [2, 3])
def test_vi_majority_over_truths(ctx, nt):
    rm, labels, pb, truth, m = _case(ctx, (28, 26, 24), 4, 10)
    t2 = truth_cells((28, 26, 24), 7, seed=12345).astype(np.uint32) + 1
    t3 = truth.copy()
    t3[np.random.default_rng(3).random(truth.shape) < 0.4] = 0
    truths = [truth, t2, t3][:nt]
    dts = [_dt(t) for t in truths]
    for typ in (1, 2):
        order, _ = rm.merge_order_pb(type=typ)
        ref = Ref(labels, order, m)
        for opt in (0, 1, 2):
            gaps = []
            want = ref.labels(truths, metric="vi", opt=opt, gaps=gaps)
            assert rm.bc_label(dts, order, metric="vi", opt=opt).tolist() == want, (typ, opt)
            _no_near_ties(gaps)
    if nt == 2:                            # an even count ties somewhere: the tie goes to the label of the second truth
        order, _ = rm.merge_order_pb(type=1)
        per = [Ref(labels, order, m).labels([t], metric="vi") for t in truths]
        assert any(a != b for a, b in zip(*per))


def test_errors(ctx):
    from glia_amd import hmt
    rm, labels, pb, truth, m = _case(ctx, (20, 18, 16), 4, 8)
    dt = _dt(truth)
    order, _ = rm.merge_order_pb(type=1)
    order = np.asarray(order, np.uint32)
    bad = []
    o = order.copy(); o[0, 0] = 0xFFFFFFF0; bad.append(o)                              # unknown region
    o = order.copy(); o[1, 0] = o[0, 0]; bad.append(o)                                 # already merged
    o = order.copy(); o[1, 2] = o[0, 2]; bad.append(o)                                 # reused key
    o = order.copy(); o[0, 2] = o[5, 1]; bad.append(o)                                 # new key = an existing region
    for o in bad:
        with pytest.raises(hmt.HmtError) as e:
            rm.bc_label(dt, o)
        assert e.value.code == hmt.ERR_ARG
    for kw in (dict(opt=3), dict(opt=-1), dict(metric="vi", tweak=True), dict(metric="vi", opt_split=True), dict(metric="vi", mpd=0.5)):
        with pytest.raises(hmt.HmtError) as e:
            rm.bc_label(dt, order, **kw)
        assert e.value.code == hmt.ERR_ARG, kw
    for metric in ("f1", "ri"):
        with pytest.raises(hmt.HmtError) as e:
            rm.bc_label([dt, dt], order, metric=metric)
        assert e.value.code == hmt.ERR_ARG
    copy = hmt.RegionMap.from_tensors(ctx, rm, rm.to_tensors())                       # no volumes behind it
    with pytest.raises(hmt.HmtError) as e:
        copy.bc_label(dt, order)
    assert e.value.code == -3
    assert hmt.Context.internal_errors() == 0


def test_growth_path_same_labels(ctx):
    """GLIA_HMT_MINCAP: the contingency table starts at 1024 slots and is doubled until it fits"""
    from glia_amd import hmt
    rm, labels, pb, truth, m = _case(ctx, (40, 36, 28), 4, 6, erase=True)
    order, _ = rm.merge_order_pb(type=2)
    dt = _dt(truth)
    a = rm.bc_label(dt, order, metric="vi", opt=1)
    with hmt.options(GLIA_HMT_MINCAP="1"):
        b = rm.bc_label(dt, order, metric="vi", opt=1)
    assert (a == b).all()
    assert a.tolist() == Ref(labels, order).labels([truth], metric="vi", opt=1)


def test_unaligned_truth(ctx):
    """a truth view that is not 16-byte aligned takes the scalar loads of the counting pass"""
    import torch
    rm, labels, pb, truth, m = _case(ctx, (24, 22, 20), 4, 8)
    order, _ = rm.merge_order_pb(type=1)
    base = torch.from_numpy(np.concatenate([[0], truth.reshape(-1)]).astype(np.uint32).view(np.int32)).cuda()
    dt = base[1:].view(truth.shape)
    assert dt.data_ptr() % 16 != 0
    assert rm.bc_label(dt, order, metric="ri").tolist() == Ref(labels, order).labels([truth], metric="ri")


def _write_mha(path, a, etype="MET_UINT"):
    dims = " ".join(str(v) for v in a.shape[::-1])
    with open(path, "wb") as f:
        f.write(("ObjectType = Image\nNDims = %d\nBinaryData = True\nBinaryDataByteOrderMSB = False\nDimSize = %s\n"
                 "ElementType = %s\nElementDataFile = LOCAL\n" % (a.ndim, dims, etype)).encode())
        f.write(np.ascontiguousarray(a).tobytes())


def test_cli_matches_python(ctx):
    rm, labels, pb, truth, m = _case(ctx, (26, 24, 22), 4, 9, mask=True)
    order, _ = rm.merge_order_pb(type=2)
    t2 = truth_cells((26, 24, 22), 6, seed=99).astype(np.uint32) + 1
    env = dict(os.environ)
    with tempfile.TemporaryDirectory() as d:
        p = lambda n: os.path.join(d, n)
        _write_mha(p("seg.mha"), labels)
        _write_mha(p("truth.mha"), truth)
        _write_mha(p("truth2.mha"), t2)
        _write_mha(p("mask.mha"), m)
        np.savetxt(p("order.txt"), np.asarray(order), fmt="%d")
        runs = [(["bc_label_ri", "-s", p("seg.mha"), "-o", p("order.txt"), "-t", p("truth.mha"), "-n", p("mask.mha"), "-l", p("a.txt")],
                 dict(metric="f1"), [truth]),
                (["bc_label_ri", "-s", p("seg.mha"), "-o", p("order.txt"), "-t", p("truth.mha"), "-n", p("mask.mha"), "--f1", "false",
                  "-l", p("a.txt")], dict(metric="ri"), [truth]),
                (["bc_label_ri", "-s", p("seg.mha"), "-o", p("order.txt"), "-t", p("truth.mha"), "-n", p("mask.mha"), "-p", "true", "-w", "true",
                  "-d", "0.3", "-l", p("a.txt")], dict(metric="f1", opt_split=True, tweak=True, mpd=0.3), [truth]),
                (["bc_label_ri", "-s", p("seg.mha"), "-o", p("order.txt"), "-t", p("truth.mha"), "-n", p("mask.mha"), "-g", "2", "-l", p("a.txt")],
                 dict(metric="f1", opt=2), [truth]),
                (["bc_label_vi", "-s", p("seg.mha"), "-o", p("order.txt"), "-t", p("truth.mha"), p("truth2.mha"), "-m", p("mask.mha"), "-g", "1",
                  "-l", p("a.txt")], dict(metric="vi", opt=1), [truth, t2]),
                (["bc_label_vi", "-s", p("seg.mha"), "-o", p("order.txt"), "-t", p("truth.mha"), "-m", p("mask.mha"), "-l", p("a.txt")],
                 dict(metric="vi"), [truth])]
        for argv, kw, truths in runs:
            argv = [os.path.join(ROOT, "cli", argv[0])] + argv[1:]
            r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
            got = np.loadtxt(p("a.txt"), dtype=np.int64).reshape(-1).tolist()
            assert got == rm.bc_label([_dt(t) for t in truths], order, **kw).tolist(), argv
            assert got == Ref(labels, order, m).labels(truths, **kw), argv


def test_large_256(ctx):
    """256^3, S = 16: GPU labels against the restatement run on the CPU"""
    shape, S, G = (256, 256, 256), 16, 40
    rm, labels, pb, truth, m = _case(ctx, shape, S, G, erase=True)
    order, _ = rm.merge_order_pb(type=1)
    dt = _dt(truth)
    ref = Ref(labels, order)
    for kw in (dict(metric="f1"), dict(metric="vi")):
        gaps = [] if kw["metric"] == "vi" else None
        assert rm.bc_label(dt, order, **kw).tolist() == ref.labels([truth], gaps=gaps, **kw), kw
        if gaps is not None:
            _no_near_ties(gaps)


# ---- the contingency table behind the labels: glia_hmt_label_overlap on (labels, truth), its labels mapped to leaves on the host ----
def _table_entries(labels, truths, m):
    """distinct (label, truth) pairs over the kept voxels, truth 0 included, summed over the truths"""
    keep = np.ones(labels.size, bool) if m is None else m.reshape(-1) != 0
    lab = labels.reshape(-1)[keep].astype(np.uint64) << np.uint64(32)
    return sum(len(np.unique(lab | t.reshape(-1)[keep].astype(np.uint64))) for t in truths)


# voxel counts: 19575 = 4 * 4893 + 3 (the scalar tail of the stream; two workgroups of 16 Ki voxels), 961 (less than one workgroup
# step of 1024), 40320 (three workgroups).  The truth cells are small, so that the table has more than 768 entries everywhere: in
# the 2D case every voxel has a truth label of its own and none is erased.
TABLE_VOLS = [((29, 27, 25), 3, 4, True, dict(metric="f1")), ((31, 31), 2, 1, False, dict(metric="ri")),
              ((40, 36, 28), 4, 6, True, dict(metric="vi", opt=1))]


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("shape,S,G,erase,kw", TABLE_VOLS)
def test_table_entries(ctx, shape, S, G, erase, kw, mask):
    """last_bc_label_timing()["entries"] is the number of distinct (label, truth) pairs NumPy finds, also when the counting pass is
    repeated: under GLIA_HMT_MINCAP the table starts at 1024 slots, of which a pass may fill 768"""
    from glia_amd import hmt
    rm, labels, pb, truth, m = _case(ctx, shape, S, G, erase=erase, mask=mask)
    assert labels.size == int(np.prod(shape)) and (m is None) == (not mask)
    truths = [truth]
    if kw["metric"] == "vi":                                                   # several truths: the entries of all their tables
        truths.append(truth_cells(shape, 5, seed=4321).astype(np.uint32) + 1)
    want_entries = _table_entries(labels, truths, m)
    assert min(_table_entries(labels, [t], m) for t in truths) > 768           # every MINCAP pass below is certain to be repeated
    order, _ = rm.merge_order_pb(type=1)
    assert len(order) > 20
    want = Ref(labels, order, m).labels(truths, **kw)
    dts = [_dt(t) for t in truths]
    assert rm.bc_label(dts, order, **kw).tolist() == want
    assert rm.last_bc_label_timing()["entries"] == want_entries
    with hmt.options(GLIA_HMT_MINCAP="1"):
        assert rm.bc_label(dts, order, **kw).tolist() == want
    assert rm.last_bc_label_timing()["entries"] == want_entries
    assert hmt.Context.internal_errors() == 0


def test_reserved_pair(ctx):
    """truth 0xFFFFFFFF on masked-out voxels is the pair (0xFFFFFFFF, 0xFFFFFFFF) of the folded labels, which label_overlap keeps out
    of its hash table and appends last; it belongs to no region, while 0xFFFFFFFF on kept voxels is a truth label like any other"""
    shape = (26, 24, 22)
    rm, labels, pb, truth, m = _case(ctx, shape, 4, 9, mask=True)
    truth = truth.copy()
    a = tuple(slice(v // 2 - 4, v // 2 + 5) for v in shape)                    # around the masked-out block in the middle
    b = tuple(slice(0, v // 3) for v in shape)
    truth[a] = 0xFFFFFFFF
    truth[b] = 0xFFFFFFFE
    assert (m[a] == 0).any() and (m[a] != 0).any() and (m[b] == 0).any() and (m[b] != 0).any()
    assert len(np.unique(labels[a][m[a] != 0])) > 1 and len(np.unique(labels[b][m[b] != 0])) > 1
    order, _ = rm.merge_order_pb(type=1)
    ref = Ref(labels, order, m)
    dt = _dt(truth)
    for metric in ("f1", "ri", "vi"):
        gaps = [] if metric == "vi" else None
        assert rm.bc_label(dt, order, metric=metric).tolist() == ref.labels([truth], metric=metric, gaps=gaps), metric
        assert rm.last_bc_label_timing()["entries"] == _table_entries(labels, [truth], m)
        if gaps is not None:
            _no_near_ties(gaps)
