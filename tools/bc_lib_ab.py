"""A/B of the classifier loop between builds of the library: five rounds of alternating child processes, each timing the forest loop
(255 trees, helpers) and the stub loop of the 512^3, S = 16 synth volume; medians at the end.
usage: bc_lib_ab.py <tag> <libglia_hmt.so> <tag> <libglia_hmt.so> ...   (e.g. parent /path/to/the/parent/build new glia_amd/libglia_hmt.so)"""
import os, subprocess, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
libs = dict(zip(sys.argv[1::2], (os.path.abspath(p) for p in sys.argv[2::2])))
child = r'''
import sys, os, tempfile
sys.path.insert(0, %r)
from glia_amd import hmt
from glia_amd.synth_forest import synthetic_forest, write_model
ctx = hmt.Context(0)
labels, pb = ctx.synth((512,) * 3, 16, 128)
rm = hmt.RegionMap(ctx, labels, pb=pb, cfg=hmt.make_config(pb, rb=[(pb, 8, 0.0, 1.0)]))
with tempfile.TemporaryDirectory() as d:
    p = os.path.join(d, "m.bin"); write_model(p, synthetic_forest(ntree=255, dim=3)); forest = hmt.RandomForest(ctx, p, predict_label=-1)
stub = hmt.FeatureStubClassifier(ctx, 31)
for name, clf in (("warm", forest), ("forest", forest), ("stub", stub)):
    rm.merge_order_bc(clf); tm = rm.last_merge_timing()
    if name != "warm": print("RES", name, tm["ms_loop"], tm["ms_init"])
''' % ROOT
res = {}
for rep in range(5):
    for tag, lib in libs.items():
        out = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, GLIA_HMT_LIB=lib), capture_output=True, text=True, timeout=170)
        if out.returncode != 0:
            print("child failed", tag, out.returncode, out.stderr[-400:]); sys.exit(1)
        for ln in out.stdout.splitlines():
            if ln.startswith("RES"):
                _, name, loop, init = ln.split()
                res.setdefault((tag, name), []).append((float(loop), float(init)))
                print("rep %d %-7s %-7s loop %.2f ms init %.2f ms" % (rep, tag, name, float(loop), float(init)), flush=True)
for k, v in sorted(res.items()):
    l = [a for a, _ in v]; i = [b for _, b in v]
    print("%-7s %-7s loop median %.2f (min %.2f max %.2f)  init median %.2f" % (k[0], k[1], statistics.median(l), min(l), max(l), statistics.median(i)))
