"""The classifier merge loop under its scorers, on one synth volume: the feature stub, the 10 + 10 MLP (scored by the loop's own
workgroup: no helper workgroups serve it), the 255-tree forest with GLIA_HMT_HELPERS=0 (the same route) and with its helpers.
Alternating runs, the median loop time of each, the MLP's merges/s and its ratio to the stub.

usage: bc_mlp_bench.py [size=512] [S=16] [reps=5] [--prof glia_amd/libglia_hmt_prof.so] [--out file]
--prof: one more MLP run in a child process against the profiling build (make -C glia_amd/csrc prof), whose loop kernel prints its
phase counters at the end of every launch; the phase "forest/publish" (PH(5)) lies between the feature vectors and the queue insertion
and is mlp_chunk under the MLP.  The counters tick in shader cycles, so the time is given as PH(5)'s share of all the phases' cycles
times the loop time of that run, per merge (a merge is one or more scoring rounds).
--out: the report is also written to that file (profiles/bc_mlp_bench.txt)."""
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from glia_amd import hmt
from glia_amd.synth_forest import synthetic_forest, write_model

argv = list(sys.argv[1:])
opt = {}
for flag in ("--prof", "--out", "--only"):
    if flag in argv:
        i = argv.index(flag)
        opt[flag] = argv[i + 1]
        del argv[i:i + 2]
size = int(argv[0]) if len(argv) > 0 else 512
S = int(argv[1]) if len(argv) > 1 else 16
reps = int(argv[2]) if len(argv) > 2 else 5
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


ctx = hmt.Context(0)
labels, pb = ctx.synth((size,) * 3, S, 8 * S)
cfg = hmt.make_config(pb, rb=[(pb, 8, 0.0, 1.0)])
rm = hmt.RegionMap(ctx, labels, pb=pb, cfg=cfg)
dim = rm.feat_dim()
stub = hmt.FeatureStubClassifier(ctx, 11 + 4 * 3 + 7 + 1)      # x0.b0.mean
# the MLP's min/max table spans the rows of the stub's run, so the model does not saturate and its order is as varied as a trained one's
_, _, rows = rm.merge_order_bc(stub, want_feats=True)
rng = np.random.default_rng(1010)
w = rng.standard_normal((dim + 1) * 10 + 11 * 10 + 11) * 0.4
mlp = hmt.MLP.from_arrays(ctx, w, 10, 10, rows.min(0) - 0.25, rows.max(0) + 0.25)
with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, "m.bin")
    write_model(path, synthetic_forest(ntree=255, dim=3))
    forest = hmt.RandomForest(ctx, path, predict_label=-1)
runs = [("stub", stub, {}), ("mlp 10+10", mlp, {}), ("forest 255, helpers 0", forest, dict(GLIA_HMT_HELPERS=0)), ("forest 255, helpers", forest, {})]
if "--only" in opt:                                     # the child of --prof: one scorer, once; the kernel's printout goes to stdout
    name, clf, env = next(r for r in runs if r[0] == opt["--only"])
    sys.stdout.flush()
    with hmt.options(**env):
        order, _ = rm.merge_order_bc(clf)
    ctx.sync()
    print("CHILD %s loop_ms %.3f merges %d" % (name, rm.last_merge_timing()["ms_loop"], len(order)), flush=True)
    sys.exit(0)
loop = {name: [] for name, _, _ in runs}
init = {name: [] for name, _, _ in runs}
merges = {}
say("size=%d S=%d regions=%d pairs=%d D_f=%d libm exp variant=%d" % (size, S, rm.num_regions, rm.num_pairs, dim, ctx.libm_exp()))
for rep in range(reps):
    for name, clf, env in runs:
        with hmt.options(**env):
            order, sal = rm.merge_order_bc(clf)
        tm = rm.last_merge_timing()
        loop[name].append(tm["ms_loop"]); init[name].append(tm["ms_init"]); merges[name] = len(order)
        say("  rep %d  %-24s loop %9.2f ms  init %8.2f ms  merges %d  distinct saliencies %d" % (rep, name, tm["ms_loop"], tm["ms_init"], len(order), len(np.unique(sal))))
med = {k: statistics.median(v) for k, v in loop.items()}
for name, _, _ in runs:
    say("%-24s loop median %9.2f ms (min %.2f, max %.2f)  init median %.2f ms  %9.0f merges/s  per merge %.2f us" % (
        name, med[name], min(loop[name]), max(loop[name]), statistics.median(init[name]), merges[name] / (med[name] * 1e-3), med[name] * 1e3 / merges[name]))
say("mlp / stub loop time: %.3f   forest(helpers 0) / stub: %.3f   forest(helpers) / stub: %.3f   mlp / forest(helpers): %.3f" % (
    med["mlp 10+10"] / med["stub"], med["forest 255, helpers 0"] / med["stub"], med["forest 255, helpers"] / med["stub"],
    med["mlp 10+10"] / med["forest 255, helpers"]))
assert hmt.Context.internal_errors() == 0
if "--prof" in opt:
    for name in ("mlp 10+10", "stub"):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), str(size), str(S), "1", "--only", name],
                             env=dict(os.environ, GLIA_HMT_LIB=os.path.abspath(opt["--prof"])), capture_output=True, text=True)
        if out.returncode != 0:
            say("profiling run of %s failed (%d): %s" % (name, out.returncode, out.stderr[-300:]))
            sys.exit(1)
        phases = {}
        for ln in out.stdout.splitlines():
            if ln.startswith("[bc profile] merges"):
                for key, val in re.findall(r"([a-z][a-z0-9+_/ -]*?) (\d+)(?=  |\)| \()", ln.split(":", 1)[1].replace("(top2: ", "  ")):
                    phases[key.strip()] = phases.get(key.strip(), 0) + int(val)
        child = re.search(r"CHILD .* loop_ms ([0-9.]+) merges (\d+)", out.stdout)
        loop_ms, n = float(child.group(1)), int(child.group(2))
        main = {k: v for k, v in phases.items() if k not in ("second-best pass", "table clear + barrier")}      # (parts of top2)
        total = sum(main.values())
        ph5 = main["forest/publish"]
        say("profiling build, %-10s loop %.2f ms, %d merges: PH(5) (mlp_chunk under the MLP) %d cycles = %.1f %% of the phases' cycles = %.2f us per merge; "
            "PH(4) local scoring (staging + feature vectors) %.1f %% = %.2f us per merge" % (
                name + ":", loop_ms, n, ph5, 100.0 * ph5 / total, ph5 / total * loop_ms * 1e3 / n,
                100.0 * main["local scoring"] / total, main["local scoring"] / total * loop_ms * 1e3 / n))
if "--out" in opt:
    with open(opt["--out"], "w") as f:
        f.write("\n".join(report) + "\n")
