"""Generates tests/golden/headline/reference_<case>.npz: merge orders of volumes of 13 824 to 32 768 regions computed by the REFERENCE'S OWN
engine (oracle/_ref/ref_engine: TBoundaryTable / TRegionMap / genMergeOrderGreedy compiled in place) and, on the same region map, by the
oracle, which must agree (same order; saliencies within 1e-12, and equal for these Q8 volumes) or the generator stops.  Sibling of
gen_headline256.py, which anchors the 256^3 pb-mean and classifier orders in the oracle alone.

Per case: the volume is O.synth's (bit-identical to glia_hmt_synth), the mask (where there is one) is mask_for's; the region map is
dumped in the compact form (only voxels some list names) and fed to ref_engine on stdin, while the oracle runs merge_order_pb / pre_merge
on a region map of its own.  The median x min-size linkage (type 3) has no caller in the reference and no path in the driver: its answer
is the oracle's alone, and the fixture says so (`answer_from`).  Each case also records a reduced twin (same code, 128^3, S = 8, 4 096
regions) that tests/test_golden_reference_orders.py recomputes live with the oracle, so the oracle cannot drift away from the recorded
reference unnoticed.

What a case must fulfil besides oracle = reference (asserted here):
  * the rule of glia_hmt_check_merge_order holds for the recorded order (replay in numpy);
  * pre_merge: 0.1 R < merges < 0.9 (R - 1), and with two size thresholds at least 1 % of the merges join regions whose smaller side has
    reached size_thresholds[0], i.e. they passed by the second rule alone;
  * masked: the mask removes at least one whole supervoxel and more than 10 000 regions stay.

usage (repository root, CPU only, after `make -C oracle && make -C oracle ref`):
    python tests/golden/gen_reference_orders.py [case ...]        # all cases by default; cases are independent and may run side by side
Measured with the reference engine and the oracle of a case side by side on a core each (seconds; ref_engine whole / its engine alone):
    case               regions  merges  synth  rag  dump (bytes)   ref_engine   oracle
    pb512               32 768  32 767   91.8  5.3  20.9 (703 MB)  309.5 / 298.2  406.9
    median256s8         32 768  32 767   12.4  1.2   5.3 (156 MB)  417.5 / 414.2  363.6
    median192s8_upd     13 824  13 823    4.7  0.5   3.1 (156 MB)   54.1 /  51.2   39.4
    premerge256s8       32 768  10 093   12.7  1.7   8.8 (383 MB)  265.0 / 259.8  244.2   (87 % of the merges by the second rule)
    premerge192s8_one   13 824   9 586    5.8  0.7   4.3 (156 MB)   39.6 /  37.2   29.2
    minsize192s8        13 824  13 823    4.7                                      32.7   (oracle only)
    pb_masked192s8      13 785  13 784    4.1  0.5   3.1 (105 MB)   32.4 /  30.8   26.7   type 2
                                                0.5   2.5            47.0 /  45.2   31.7   type 1
The median linkage finished at the full 32 768 regions in seven minutes, so no case was shrunk.  The engine alone took 1.46 s at 4 096
regions (256^3, S = 16) and 298 s at 32 768: about R^2.6, which puts 262 144 regions (1024^3) at most of a day -- PB_1024 stays a
digest the device recorded.  The compact dump was checked once against the full one at 256^3 (84 MB against 207 MB): ref_engine wrote
the same bytes.
"""
import hashlib, json, os, subprocess, sys, tempfile, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from oracle import pyoracle as O

REF_ENGINE = os.path.join(ROOT, "oracle", "_ref", "ref_engine")
OUT_DIR = os.path.join(ROOT, "tests", "golden", "headline")
TWIN = dict(size=128, S=8, G=64)                       # 4 096 regions: the oracle's loops take a second or two

# run = (name, kind, type): kind "pb" -> merge_order_pb(type), "pre_merge" -> pre_merge(sizes, rpb)
CASES = {
    "pb512":             dict(size=512, S=16, G=128, only_contour=True, runs=[("type2", "pb", 2)]),
    "median256s8":       dict(size=256, S=8, G=64, only_contour=True, runs=[("type1", "pb", 1)]),
    "median192s8_upd":   dict(size=192, S=8, G=64, only_contour=False, update_region=True, runs=[("type1", "pb", 1)]),
    "premerge256s8":     dict(size=256, S=8, G=64, only_contour=False, sizes=[300, 1500], rpb=0.3, runs=[("pre_merge", "pre_merge", 2)]),
    "premerge192s8_one": dict(size=192, S=8, G=64, only_contour=False, sizes=[700], rpb=0.0, runs=[("pre_merge", "pre_merge", 2)]),
    "minsize192s8":      dict(size=192, S=8, G=64, only_contour=False, update_region=True, oracle_only=True, runs=[("type3", "pb", 3)]),
    "pb_masked192s8":    dict(size=192, S=8, G=64, only_contour=True, mask=True, runs=[("type2", "pb", 2), ("type1", "pb", 1)]),
}


def fixture_path(case):
    return os.path.join(OUT_DIR, "reference_%s.npz" % case)


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def mask_for(shape, seed=3):
    """the mask of tests/test_gpu_rag.py::_mask_for: holes, a masked face, a masked block several supervoxels wide"""
    rng = np.random.default_rng(seed)
    m = (rng.random(shape) > 0.15).astype(np.uint32) * 5
    m[..., :2] = 0
    sl = tuple(slice(s // 3, s // 3 + max(2, s // 5)) for s in shape)
    m[sl] = 0
    return m


def twin_of(p):
    return dict(p, **TWIN)


def make_volume(p):
    shape = (p["size"],) * 3
    lab, pb = O.synth(shape, p["S"], p["G"])
    return lab, pb, (mask_for(shape) if p.get("mask") else None)


def initial_sizes(lab, mask):
    """voxels per label (masked voxels belong to no region); index = label"""
    l = lab.ravel() if mask is None else lab.ravel()[mask.ravel() != 0]
    return np.bincount(l)


def oracle_run(p, run, lab, pb, mask):
    """the oracle's answer on a region map of its own (update_region folds merged regions into the map)"""
    rag = O.Rag(lab, mask=mask, only_contour=p["only_contour"])
    if run[1] == "pre_merge":
        return rag.pre_merge(pb, p["sizes"], p["rpb"])
    return rag.merge_order_pb(pb, type=run[2], update_region=bool(p.get("update_region")))


def reference_run(p, run, lab, pb, mask, compact=True):
    """ref_engine's answer: (order, sal, seconds of rag / dump / whole process / engine alone)"""
    t = {}
    t0 = time.perf_counter()
    rag = O.Rag(lab, mask=mask, only_contour=p["only_contour"])
    t["rag"] = time.perf_counter() - t0
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "dump.txt")
        t0 = time.perf_counter()
        rag.dump(pb, run[2], bool(p.get("update_region")) or run[1] == "pre_merge", path, compact=compact)
        if run[1] == "pre_merge":
            with open(path, "a") as f:
                f.write("%d %s %r\n" % (len(p["sizes"]), " ".join(str(int(s)) for s in p["sizes"]), float(p["rpb"])))
        t["dump"] = time.perf_counter() - t0
        t["dump_bytes"] = os.path.getsize(path)
        del rag
        t0 = time.perf_counter()
        with open(path, "rb") as f:
            r = subprocess.run([REF_ENGINE], stdin=f, capture_output=True, check=True)
        t["ref_engine"] = time.perf_counter() - t0
    t["engine_only"] = float(r.stderr.decode().split("engine_seconds")[1].split()[0])
    rows = [l.split() for l in r.stdout.decode().split("\n") if l and l[0] != "K"]
    order = np.array([[int(x) for x in r[:3]] for r in rows], dtype=np.uint32).reshape(-1, 3)
    sal = np.array([float(r[3]) for r in rows], dtype=np.float64)
    return order, sal, t


def replay(order, present, first_new):
    """glia_hmt_check_merge_order's rule on keys: merge k joins two regions that exist and creates first_new + k"""
    o = order.astype(np.int64)
    n = len(o)
    assert (o[:, 2] == first_new + np.arange(n)).all()
    assert (o[:, 0] != o[:, 1]).all()
    used = np.concatenate([o[:, 0], o[:, 1]])
    assert len(np.unique(used)) == 2 * n                                     # nothing is merged twice
    k = np.concatenate([np.arange(n), np.arange(n)])
    old = used < first_new
    assert np.isin(used[old], present).all()                                 # a supervoxel of the volume
    assert (used[~old] - first_new < k[~old]).all()                          # or a region an earlier merge created


def second_rule_share(order, sizes0, thr0):
    """share of the merges whose smaller side holds >= thr0 voxels (they passed main_pre_merge's second rule only)"""
    n = len(order)
    first_new = int(order[0, 2])
    size = np.zeros(first_new + n, np.int64)
    size[:len(sizes0)] = sizes0
    late = 0
    for x0, x1, x2 in order.astype(np.int64):
        late += min(size[x0], size[x1]) >= thr0
        size[x2] = size[x0] + size[x1]
    return late / float(n)


def compute(p, reference=True):
    """one volume, all its runs: dict of arrays / digests (fixture keys without prefix) and times.  reference=False: the oracle alone
    answers (the fixture tests recompute the reduced twins that way, where oracle/_ref need not exist)"""
    out, times = {}, {}
    t0 = time.perf_counter()
    lab, pb, mask = make_volume(p)
    times["synth"] = time.perf_counter() - t0
    out["labels_sha1"], out["pb_sha1"] = sha(lab), sha(pb)
    out["mask_sha1"] = sha(mask) if mask is not None else ""
    sizes0 = initial_sizes(lab, mask)
    present = np.nonzero(sizes0)[0]
    present = present[present != 0]
    R = len(present)
    first_new = int(present.max()) + 1
    out["regions"] = R
    if mask is not None:
        assert R < int(lab.max()), "the mask removes no whole supervoxel"
        out["absent_labels"] = np.setdiff1d(np.arange(1, first_new), present).astype(np.uint32)    # supervoxels the mask removed whole
    reference = reference and not p.get("oracle_only")
    for run in p["runs"]:
        name = run[0]
        res = {}
        th = threading.Thread(target=lambda: res.update(orc=(time.perf_counter(), oracle_run(p, run, lab, pb, mask), time.perf_counter())))
        th.start()                                                           # beside the reference's engine, on a core of its own
        tt = {}
        if reference:
            order, sal, tt = reference_run(p, run, lab, pb, mask)
        th.join()
        oo, os_ = res["orc"][1]
        tt["oracle"] = res["orc"][2] - res["orc"][0]
        if reference:
            assert oo.shape == order.shape and (oo == order).all(), "%s: the oracle's order is not the reference's" % name
            assert np.allclose(os_, sal, rtol=0, atol=1e-12) and (os_ == sal).all(), "%s: saliencies differ (Q8 pb: must be equal)" % name
        else:
            order, sal = oo, os_
        n = len(order)
        assert n > 0 and (order[:, 2] == first_new + np.arange(n)).all()
        replay(order, present, first_new)
        if run[1] == "pre_merge":
            assert 0.1 * R < n < 0.9 * (R - 1), "pre_merge: %d merges of %d regions: the condition decides too little" % (n, R)
            if len(p["sizes"]) > 1:
                share = second_rule_share(order, sizes0, p["sizes"][0])
                tt["second_rule_share"] = share
                assert share >= 0.01, "pre_merge: only %.4f of the merges pass by the second rule" % share
        elif mask is None and p["only_contour"]:
            assert n == R - 1                                                # connected graph of mutual edges
        if run[2] == 2 and run[1] == "pb":
            assert (np.diff(sal) <= 1e-12).all()                             # mean linkage is reducible
        out[name + "_x0"], out[name + "_x1"], out[name + "_first_new"] = order[:, 0].copy(), order[:, 1].copy(), first_new
        out[name + "_sal"] = sal
        out[name + "_order_sha1"], out[name + "_sal_sha1"] = sha(order), sha(sal)
        times[name] = tt
    return out, times


def generate(case):
    p = CASES[case]
    big, tb = compute(p)
    assert big["regions"] > 10000
    twin, tw = compute(twin_of(p))
    params = dict((k, v) for k, v in p.items() if k != "runs")
    params.update(runs=[list(r) for r in p["runs"]], answer_from="oracle only: the reference has no caller of this linkage" if p.get("oracle_only")
                  else "oracle/_ref/ref_engine (the reference's own engine), equal to the oracle's", twin=TWIN)
    arrays = {"params": np.array(json.dumps(params, sort_keys=True)), "seconds": np.array(json.dumps(tb, sort_keys=True))}
    for prefix, d in (("", big), ("twin_", twin)):
        for k, v in d.items():
            arrays[prefix + k] = np.asarray(v)
    os.makedirs(OUT_DIR, exist_ok=True)
    np.savez_compressed(fixture_path(case), **arrays)
    for r in p["runs"]:
        print("%s %s: %d regions, %d merges, order sha1 %s, sal sha1 %s" % (case, r[0], big["regions"], len(big[r[0] + "_x0"]),
                                                                         big[r[0] + "_order_sha1"], big[r[0] + "_sal_sha1"]), flush=True)
    print("%s seconds: %s" % (case, json.dumps(tb, sort_keys=True)), flush=True)
    print("%s twin seconds: %s" % (case, json.dumps(tw, sort_keys=True)), flush=True)
    print("%s written: %d bytes" % (case, os.path.getsize(fixture_path(case))), flush=True)


if __name__ == "__main__":
    for case in (sys.argv[1:] or list(CASES)):
        generate(case)
