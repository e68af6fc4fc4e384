"""Initial-edge scoring with and without the median layout (GLIA_USE_MEDIAN_AS_FEATS) on a synthetic volume, rb = [pb]:
    python tools/median_init_bench.py --size 1024 --S 16 --steps 3
Prints one JSON line: ms_init (HIP events around the scoring stage, glia_hmt_score_initial_edges) per step for both layouts, and the
stage split the library reports under GLIA_HMT_TRACE (sort stage | selection kernels | memory) on stderr of one extra call."""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--S", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import torch
    from glia_amd import hmt
    from glia_amd.synth_forest import synthetic_forest, write_model
    ctx = hmt.Context(0)
    labels, pb = ctx.synth((args.size,) * 3, args.S, 8 * args.S)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "forest.bin")
        write_model(path, synthetic_forest(ntree=255, dim=3))
        clf = hmt.RandomForest(ctx, path, predict_label=-1)
    out = dict(size=args.size, S=args.S)
    for name, med in (("default", False), ("median", True)):
        rm = hmt.RegionMap(ctx, labels, pb=pb, cfg=hmt.make_config(pb, rb=[(pb, 8, 0.0, 1.0)], use_median_features=med))
        ms = []
        for i in range(args.warmup + args.steps):
            n, t = rm.score_initial_edges(clf)
            if i >= args.warmup:
                ms.append(round(t, 3))
        out[name] = dict(n_edges=n, R=rm.num_regions, feat_dim=rm.feat_dim(), ms_init=ms)
        if med:
            free0, total = torch.cuda.mem_get_info()
            with hmt.options(GLIA_HMT_TRACE=1):
                rm.score_initial_edges(clf)
            out[name]["device_mem_in_use_after_GB"] = round((total - torch.cuda.mem_get_info()[0]) / 2 ** 30, 2)
        rm.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
