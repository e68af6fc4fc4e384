#!/usr/bin/env python
"""bench.py -- HMT hot path on N MI355X (one process per GPU).

A "step" is one pass of the hot path over one synthetic volume that is already resident in HBM:
  region-adjacency + sufficient-statistics accumulation (K1-K3)  ->  edge table (K4)  ->
  greedy pb-mean merge loop (K5).
`value` = region merges per second over the whole step (all ranks; weak scaling: every rank owns its own volume,
the merge loop does not shard -- SURVEY.md 8e).  `roofline` describes the dominant streaming kernel
(rag_accumulate: 8 algorithmic bytes per voxel), timed live with HIP events on the library's stream.
A plain run sets up, warms up, times --steps steps and prints the line; --dump-outputs DIR also writes what the last
timed step returned (rank 0).  Everything else runs with --full only, after the timed steps:
  `verify`        digests of the last step's merge order / saliencies against recorded ones;
  `bc_loop`       the classifier-linkage merge tree of the same volume, timed once (--no-bc skips it);
  `cpu_baseline`  the oracle (the CPU restatement of GLIA's algorithm) and the reference's own engine on bounded
                  sub-volumes on this host (--no-cpu skips it);
  `slab_rag`      with N > 1 (or --force-slab), ONE volume split into z-slabs across the ranks, the partial region/pair
                  records exchanged over RCCL (--no-slab skips it).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def cpu_baseline(size, S, bc_size, curve_sizes=(), target_regions=0):
    """oracle (reference-faithful port of GLIA's algorithm, 1 thread) on bounded sub-volumes of the same synthetic
    workload: RAG + greedy pb-mean merge tree on size^3, and the classifier-path feature evaluations on bc_size^3."""
    import numpy as np  # noqa: F401
    from oracle import pyoracle as O
    labels, pb = O.synth((size,) * 3, S, 8 * S)
    t0 = time.time()
    rag = O.Rag(labels, only_contour=True)
    t1 = time.time()
    order, _ = rag.merge_order_pb(pb, type=2)
    t2 = time.time()
    out = {"value": len(order) / (t2 - t0), "unit": "region-merges/s", "cores": 1, "kind": "port",
           "sample": "%d^3 synthetic volume, S=%d (%d regions): RAG %.2fs + greedy pb-mean %.2fs, oracle/hmt_oracle.cc; "
                     "edge features: classifier path on %d^3" % (size, S, len(order) + 1, t1 - t0, t2 - t1, bc_size),
           "merge_loop_only": len(order) / max(t2 - t1, 1e-9)}
    # the reference's own engine (type/boundary_table.hxx, type/region_map.hxx, util/struct_merge.hxx:13-33 compiled in
    # place into oracle/_ref/ref_engine, which travels prebuilt): same sample, fed the region map as a dump
    ref = os.path.join(ROOT, "oracle", "_ref", "ref_engine")
    if os.path.exists(ref):
        try:
            import subprocess
            import tempfile
            with tempfile.TemporaryDirectory() as d:
                dump = os.path.join(d, "dump.txt")
                rag.dump(pb, 2, False, dump)
                with open(dump) as f:
                    t3 = time.time()
                    res = subprocess.run([ref], stdin=f, capture_output=True, text=True, check=True, timeout=600)
                    t4 = time.time()
            n_ref = len([l for l in res.stdout.split("\n") if l.strip() and not l.startswith("K ")])     # ("K a b" lines: its transformKeys)
            eng = [l for l in res.stderr.split("\n") if l.startswith("engine_seconds")]
            if eng:
                t4 = t3 + float(eng[-1].split()[1])     # the engine's own clock around genMergeOrderGreedy (no dump parsing)
            if n_ref == len(order):
                out.update({"value": n_ref / ((t1 - t0) + (t4 - t3)), "kind": "reference", "merge_loop_only": n_ref / (t4 - t3),
                            "port_value": len(order) / (t2 - t0),
                            "sample": "%d^3 synthetic volume, S=%d (%d regions): RAG %.2fs (oracle port) + the reference's own greedy engine "
                                      "(oracle/_ref/ref_engine: boundary table + genMergeOrderGreedy headers built in place, reads a dump of the "
                                      "region map) %.2fs; edge features: classifier path (port) on %d^3"
                                      % (size, S, n_ref + 1, t1 - t0, t4 - t3, bc_size)})
        except Exception:      # noqa: BLE001 -- the port's numbers stand
            pass
    labels, pb = O.synth((bc_size,) * 3, S // 2, 4 * S)
    cfg = O.make_cfg(pb, rb=[(pb, 8, 0.0, 1.0)])
    rag = O.Rag(labels)
    t0 = time.time()
    order, _ = rag.merge_order_bc(cfg, None, stub_index=31)
    t1 = time.time()
    out["edge_features_per_sec"] = rag.n_feat_evals / (t1 - t0)
    out["bc_merges_per_sec"] = len(order) / (t1 - t0)
    out["bc_note"] = ("classifier path: the oracle port only (the reference's bc tools need ITK and its third-party forest code, absent here: "
                      "no reference-engine leg, no curve)")
    if curve_sizes and os.path.exists(ref):
        out["curve"] = reference_curve(curve_sizes, S, ref, target_regions)
    return out


def openmp_bc_feat_baseline(size, S):
    """The GLIA_MT OpenMP baseline the north star names.  bc_feat is the only OpenMP user on the path (hmt/main_bc_feat.cxx:59-101):
    oracle/_ref/ref_parfor_st / _mt are the reference's own util/mp.hxx (parfor) compiled in place without / with -DGLIA_MT -fopenmp,
    driving the oracle's feature functions over the pb-mean order of a size^3 sample of the same synthetic workload.  One D_f vector
    per merge: edge-features/s = merges / seconds of the two parfor loops + serialisation (the region map's set-up excluded)."""
    import subprocess
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    nthr = int(os.environ.get("OMP_NUM_THREADS") or ncpu)        # a thread count the environment sets is the one this host grants
    st = os.path.join(ROOT, "oracle", "_ref", "ref_parfor_st"); mt = os.path.join(ROOT, "oracle", "_ref", "ref_parfor_mt")
    if not (os.path.exists(st) and os.path.exists(mt)):
        return None
    out = {"sample": "%d^3 synthetic volume, S=%d, --rbi pb --rbb 8 --bt 0.2 0.5 0.8 (D_f=104), given pb-mean merge order; "
                     "reference parfor (util/mp.hxx built in place) over the oracle's RegionFeats / BoundaryFeats restatement" % (size, S),
           "cores_available": ncpu, "kind": "reference parfor + port features", "threads": [], "seconds": [], "edge_features_per_sec": []}
    fnv = set()
    for exe, threads in ((st, 1), (mt, nthr)):
        try:
            res = subprocess.run([exe, str(size), str(S)], capture_output=True, text=True, check=True, timeout=600,
                                 env=dict(os.environ, OMP_NUM_THREADS=str(threads)))
        except Exception:      # noqa: BLE001
            return None
        w = res.stdout.split(); kv = dict(zip(w[0::2], w[1::2]))
        secs = float(kv["seconds_regions"]) + float(kv["seconds_boundaries"]) + float(kv["seconds_serialize"])
        out["threads"].append(int(kv["threads"])); out["seconds"].append(secs); out["edge_features_per_sec"].append(int(kv["merges"]) / secs)
        out["regions"] = int(kv["regions"]); out["merges"] = int(kv["merges"]); fnv.add(kv["rows_fnv"])
    out["rows_identical_across_builds"] = len(fnv) == 1
    return out


def reference_curve(sizes, S, ref, target_regions):
    """The reference's own merge engine (oracle/_ref/ref_engine) at several region counts of the same synthetic workload:
    its boundary-table update scans a std::map prefix per merge (type/boundary_table.hxx:127-128), so the rate falls with
    the region count.  Fits merges/s = a * R^b on the measured points and EXTRAPOLATES to the bench's region count."""
    import math
    import subprocess
    import tempfile
    from oracle import pyoracle as O
    pts = []
    for size in sizes:
        labels, pb = O.synth((size,) * 3, S, 8 * S)
        rag = O.Rag(labels, only_contour=True)
        with tempfile.TemporaryDirectory() as d:
            dump = os.path.join(d, "dump.txt")
            rag.dump(pb, 2, False, dump)
            with open(dump) as f:
                t0 = time.time()
                res = subprocess.run([ref], stdin=f, capture_output=True, text=True, check=True, timeout=900)
                dt = time.time() - t0
        eng = [l for l in res.stderr.split("\n") if l.startswith("engine_seconds")]
        if eng:
            dt = float(eng[-1].split()[1])
        n = len([l for l in res.stdout.split("\n") if l.strip() and not l.startswith("K ")])
        pts.append({"size": size, "regions": n + 1, "merges": n, "engine_seconds": dt, "merges_per_sec": n / dt})
    xs = [math.log(p["regions"]) for p in pts]; ys = [math.log(p["merges_per_sec"]) for p in pts]
    mx, my = sum(xs) / len(xs), sum(ys) / len(ys)
    b = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
    a = math.exp(my - b * mx)
    return {"points": pts, "fit": "merges/s = %.4g * regions^%.3f" % (a, b), "exponent": b,
            "extrapolated": {"regions": target_regions, "merges_per_sec": a * target_regions ** b,
                             "note": "EXTRAPOLATED from the fit, not measured: the reference needs hours at this size"}}


def slab_phase(ctx, hmt, dist, torch, size, S, world, rank, clf):
    """SURVEY.md 8e / BASELINE config 4: ONE volume z-split across the ranks through the route a C++ host would use --
    glia_hmt_comm_create_rccl (RCCL, one rank per process and GPU; the 128-byte id of rank 0 travels by a torch.distributed
    broadcast, the launcher's job) + ONE collective call, glia_hmt_rag_build_distributed (glia_amd/csrc/slab_dist.cpp): partial map
    per slab, cut flags, keyed owner exchange of the cut records as unpadded ncclSend / ncclRecv inside one group, reduction at the
    owners, hand-over to the loop owner (rank 0).  Timed apart from `value` (the merge loop does not shard); rank 0 checks the
    merged map against its single-pass build."""
    labels, pb = ctx.synth((size,) * 3, S, 8 * S)            # the same volume on every rank (same seed)
    first, nplanes, zb, ze = hmt.slab_range(size, world, rank)
    sl, sp = labels[first:first + nplanes].contiguous(), pb[first:first + nplanes].contiguous()
    cfg = hmt.make_config(sp, rb=[(sp, 8, 0.0, 1.0)], thresholds=(0.2, 0.5, 0.8))
    idt = torch.zeros(128, dtype=torch.uint8, device="cuda")
    if rank == 0:
        idt.copy_(torch.frombuffer(bytearray(hmt.Comm.unique_id()), dtype=torch.uint8))
    dist.broadcast(idt, 0)
    comm = hmt.Comm(ctx, world, rank, bytes(idt.cpu().numpy().tobytes()))
    stats = {}

    def once():
        merged, st_ = hmt.build_distributed(ctx, comm, [(sl, sp, first, zb, ze, cfg)], size, only_contour=False, loop_owner=0)
        stats.update(records=int(st_.records), cut_records=int(st_.cut_records), bytes_sent_cut_exchange=int(st_.bytes_cut_exchange),
                     bytes_sent_to_loop_owner=int(st_.bytes_to_loop_owner))
        return merged

    m0 = once()                                              # warm-up (RCCL channels, allocations)
    if m0 is not None:
        m0.close()
    dist.barrier(); torch.cuda.synchronize(); ctx.sync()
    t0 = time.time()
    merged = once()
    dist.barrier(); torch.cuda.synchronize(); ctx.sync()
    t = torch.tensor([time.time() - t0], dtype=torch.float64, device="cuda")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    sent = torch.tensor([float(stats["bytes_sent_cut_exchange"]), float(stats["bytes_sent_to_loop_owner"]), float(stats["records"]),
                         float(stats["cut_records"])], dtype=torch.float64, device="cuda")
    smax = sent.clone(); dist.all_reduce(smax, op=dist.ReduceOp.MAX)
    dist.all_reduce(sent, op=dist.ReduceOp.SUM)
    out = {"ms": float(t.item()) * 1e3, "slab_planes_per_rank": ze - zb,
           "route": "C ABI: glia_hmt_comm_create_rccl + glia_hmt_rag_build_distributed (slab_dist.cpp)",
           "exchange": "cut records (label on a plane next to a cut) -> keyed owner (hash(label) mod N), ncclSend / ncclRecv in one group, "
                       "unpadded; reduced cut + interior records once to the loop owner (rank 0)",
           "records_all_ranks": int(sent[2].item()), "cut_records_all_ranks": int(sent[3].item()),
           "bytes_sent_cut_exchange_max_rank": int(smax[0].item()), "bytes_sent_to_loop_owner_max_rank": int(smax[1].item()),
           "bytes_sent_all_ranks": int(sent[0].item() + sent[1].item())}
    comm.close()
    if rank == 0:
        out["regions"] = merged.num_regions; out["pairs"] = merged.num_pairs
    lo, hi = first, first + nplanes
    # the merged map lives on the loop owner only: the others receive its compact records for the sharded scoring below
    rec = merged.to_tensors() if rank == 0 else None
    # every rank must issue the SAME sequence of collectives: the number of image channels travels with the shapes and the
    # receivers allocate the per-channel record tensors (rrec1 / prec1 ...) the owner's map carries
    nchan = 1 + sum(1 for k_ in rec if k_.startswith("rrec") and k_ != "rrec") if rank == 0 else 0
    shapes = torch.tensor([rec["rlabel"].numel(), rec["pa"].numel(), nchan] if rank == 0 else [0, 0, 0], dtype=torch.int64, device="cuda")
    dist.broadcast(shapes, 0)
    if rank != 0:
        like = hmt.RegionMap(ctx, sl, pb=sp, cfg=cfg, slab=(lo, size, zb, ze))
        lt = like.to_tensors()
        R_, P_, nchan = int(shapes[0].item()), int(shapes[1].item()), int(shapes[2].item())
        rec = dict(rlabel=torch.empty(R_, dtype=torch.int32, device="cuda"), rrec=torch.empty((R_, lt["rrec"].shape[1]), dtype=torch.int32, device="cuda"),
                   pa=torch.empty(P_, dtype=torch.int32, device="cuda"), pb=torch.empty(P_, dtype=torch.int32, device="cuda"),
                   prec=torch.empty((P_, lt["prec"].shape[1]), dtype=torch.int32, device="cuda"))
        for c_ in range(1, nchan):
            rec["rrec%d" % c_] = torch.empty((R_, lt["rrec"].shape[1]), dtype=torch.int32, device="cuda")
            rec["prec%d" % c_] = torch.empty((P_, lt["prec"].shape[1]), dtype=torch.int32, device="cuda")
    for k_ in sorted(rec.keys()):
        dist.broadcast(rec[k_], 0)
    if rank != 0:
        merged = hmt.RegionMap.from_tensors(ctx, like, rec)
        like.close()
    # K7 on the merged map, sharded by record (independent per edge): every rank scores 1/world of the initial edges,
    # one all_gather of the scores, element-wise max
    dist.barrier(); torch.cuda.synchronize(); ctx.sync()
    t0 = time.time()
    mine = torch.from_numpy(merged.score_initial_edges_shard(clf, rank, world)).cuda()
    parts = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(parts, mine)
    scores = torch.stack(parts).max(dim=0).values
    dist.barrier(); torch.cuda.synchronize(); ctx.sync()
    t = torch.tensor([time.time() - t0], dtype=torch.float64, device="cuda")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    out["sharded_edge_scoring_ms"] = float(t.item()) * 1e3
    out["edges_scored"] = int(torch.isfinite(scores).sum().item())
    if rank == 0:
        wcfg = hmt.make_config(pb, rb=[(pb, 8, 0.0, 1.0)], thresholds=(0.2, 0.5, 0.8))
        whole = hmt.RegionMap(ctx, labels, pb=pb, cfg=wcfg)
        a, b = whole.pairs(), merged.pairs()
        ra, rb = whole.regions(), merged.regions()
        out["identical_to_single_pass"] = bool(all((a[k] == b[k]).all() for k in a) and all((ra[k] == rb[k]).all() for k in ra))
        out["ms_single_gpu_accumulate"] = whole.last_pass()[0]
        full = torch.from_numpy(whole.score_initial_edges_shard(clf, 0, 1)).cuda()
        out["scores_identical_to_single_gpu"] = bool(torch.equal(full, scores))
        whole.close()
    merged.close()
    return out


def world_size():
    return int(os.environ.get("WORLD_SIZE", "1"))


OUTPUT_BYTES = 64 * 10 ** 6


def dump_outputs(d, arrays):
    """arrays: {name: array with one row per item} -> d/<name>.npy as float64.  Above OUTPUT_BYTES together, every array keeps
    the same fixed, seeded sample of its rows, and d/<name>_rows.npy holds the row numbers kept."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    total = sum(8 * a.size for a in arrays.values())
    for name, a in arrays.items():
        a = np.asarray(a, np.float64)
        if total > OUTPUT_BYTES:                 # half the budget for the rows, at most as much again for their numbers
            keep = max(1, len(a) * OUTPUT_BYTES // (2 * total))
            rows = np.sort(np.random.default_rng(0).choice(len(a), keep, replace=False)).astype(np.float64)
            np.save(os.path.join(d, name + "_rows.npy"), rows)
            a = a[rows.astype(np.int64)]
        np.save(os.path.join(d, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--S", type=int, default=16)
    ap.add_argument("--cpu-size", type=int, default=256)
    ap.add_argument("--cpu-bc-size", type=int, default=40)
    ap.add_argument("--cpu-bcfeat-size", type=int, default=128, help="sample of the OpenMP bc_feat baseline (S/2 supervoxels: 4096 regions at 128)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-curve", type=str, default="128,256,384", help="volume sizes for the reference engine's scaling curve ('' = none)")
    ap.add_argument("--no-bc", action="store_true", help="skip the classifier-linkage merge tree (timed once, outside the steps)")
    ap.add_argument("--no-slab", action="store_true", help="N > 1: skip the z-slab split + RCCL exchange phase")
    ap.add_argument("--slab-timeout", type=int, default=240)
    ap.add_argument("--force-slab", action="store_true", help="with --full: rehearse the slab phase with a 1-rank RCCL group (N = 1)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also the digest check, the classifier-linkage merge tree, the CPU baselines and the slab phase")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the merge order and saliencies the last timed step returned to DIR/<name>.npy (float64)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    slab = args.full and (world_size() > 1 or args.force_slab) and not args.no_slab

    import tempfile
    import torch
    import torch.distributed as dist
    from glia_amd import hmt
    from glia_amd.synth_forest import synthetic_forest, write_model

    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = world_size()
    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    elif slab:
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29517", rank=0, world_size=1,
                                device_id=torch.device("cuda", local))

    ctx = hmt.Context(local)
    shape = (args.size,) * 3
    labels, pb = ctx.synth(shape, args.S, 8 * args.S, seed=0x9E3779B97F4A7C15 + rank)
    cfg = hmt.make_config(pb, rb=[(pb, 8, 0.0, 1.0)], thresholds=(0.2, 0.5, 0.8))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "forest_rank%d.bin" % rank)
        write_model(path, synthetic_forest(ntree=255, dim=3))
        clf = hmt.RandomForest(ctx, path, predict_label=-1)
    N = labels.numel()

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        ctx.sync()

    def step():
        # K1-K3 accumulation (regions + directed pairs, all statistics) -> K4 compaction
        t_a = time.time()
        rm = hmt.RegionMap(ctx, labels, pb=pb, only_contour=False, cfg=cfg)
        ms, by = rm.last_pass()
        if os.environ.get("GLIA_BENCH_SYNC"):
            torch.cuda.synchronize(); ctx.sync()
        t_b = time.time()
        # K6 + K7: feature vector + forest score of every initial edge (TBoundaryTable::init, classifier linkage)
        n_edges, ms_score = rm.score_initial_edges(clf)
        t_c = time.time()
        # K4b + K5: edge table + greedy merge loop (pb-mean linkage), R-1 contractions
        order, sal = rm.merge_order_pb(type=2)
        t_d = time.time()
        tm = rm.last_merge_timing()
        info = dict(R=rm.num_regions, P=rm.num_pairs, merges=len(order), acc_ms=ms, acc_bytes=by, n_edges=n_edges,
                    ms_score=ms_score, feat_dim=rm.feat_dim(), **tm)
        rm.close()
        t_e = time.time()
        info["host_ms"] = dict(build=(t_b - t_a) * 1e3, score=(t_c - t_b) * 1e3, merge_order=(t_d - t_c) * 1e3, close=(t_e - t_d) * 1e3)
        info["_result"] = (order, sal)          # dumped / hashed after the timed region (--dump-outputs, the `verify` field)
        return info

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.time()
    infos = [step() for _ in range(args.steps)]
    barrier()
    dt = time.time() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        m = torch.tensor([float(sum(i["merges"] for i in infos)), float(sum(i["n_edges"] for i in infos))],
                         dtype=torch.float64, device="cuda")
        dist.all_reduce(m, op=dist.ReduceOp.SUM)
        merges, edges = float(m[0].item()), float(m[1].item())
    else:
        merges = float(sum(i["merges"] for i in infos))
        edges = float(sum(i["n_edges"] for i in infos))
    if rank == 0 and args.dump_outputs:
        o_, s_ = infos[-1]["_result"]
        dump_outputs(args.dump_outputs, {"pb_mean_order": o_, "pb_mean_saliency": s_})

    # `verify`: digests of the LAST timed step's whole merge order / saliency arrays, computed outside the timed region, against the
    # digests tests/test_gpu_headline.py gates (recorded from kernels that were bit-identical to the oracle wherever it finishes)
    import hashlib
    sha = lambda a: hashlib.sha1(__import__("numpy").ascontiguousarray(a).tobytes()).hexdigest()
    known_pb = {(512, 16): ("652c84e7efe781bacc9df8c0a16675ca7e34cf17", "d78663710b1699d331a62c40471ba2d90ffc6515"),
                (1024, 16): ("977022085e1a37a4d143841a51ea8834b6f53c59", "7923436b47d4484f1e95962ac87ff409d4f2c617")}
    known_bc = {(256, 16): ("51b7b5316e0d8fd648ab2b444527633d8eaf65c5", "5eadbd683d6a042f7bf950aa2352ef93bdc12956"),
                (512, 16): ("8e620b69eab2cc31991eaca662446f52ad2231df", "8e30e7ba92d7b89dc09c413260a0841df1cbf886"),
                (1024, 16): ("6d930d8a816d75d194b20c5f4eb068a3bd362f3f", "1915075dc494d7c5b56baea947414d1890c2d8f8")}
    verify = None
    if rank == 0 and args.full:
        o_, s_ = infos[-1]["_result"]
        got = (sha(o_), sha(s_))
        exp = known_pb.get((args.size, args.S))
        verify = {"pb_mean_order_sha1": got[0], "pb_mean_saliency_sha1": got[1], "expected": list(exp) if exp else None,
                  "ok": (got == exp) if exp else None}
    for i_ in infos:
        i_.pop("_result", None)
    bc_loop = None
    if rank == 0 and args.full and not args.no_bc:
        # the north-star linkage: the classifier-driven merge tree (util/struct_merge_bc.hxx:10-58) of the SAME volume, every
        # new edge featurised (D_f doubles) and scored by the 255-tree forest inside the greedy loop; timed once, outside `value`
        rm = hmt.RegionMap(ctx, labels, pb=pb, only_contour=False, cfg=cfg)
        torch.cuda.synchronize(); ctx.sync()
        t0 = time.time()
        order, sal = rm.merge_order_bc(clf)
        t1 = time.time()
        tm = rm.last_merge_timing()
        bc_loop = {"linkage": "boundary classifier (random forest, 255 trees, D_f=%d)" % rm.feat_dim(), "merges": len(order),
                   "seconds": t1 - t0, "merges_per_sec": len(order) / (t1 - t0), "edges_scored": tm["n_edges_scored"],
                   "edge_features_per_sec": tm["n_edges_scored"] / (t1 - t0), "ms_init": tm["ms_init"], "ms_loop": tm["ms_loop"]}
        got = (sha(order), sha(sal))
        exp = known_bc.get((args.size, args.S))
        bc_loop["verify"] = {"order_sha1": got[0], "saliency_sha1": got[1], "expected": list(exp) if exp else None, "ok": (got == exp) if exp else None}
        rm.close()
    out = None
    if rank == 0:
        acc_ms = sum(i["acc_ms"] for i in infos) / len(infos)
        achieved = infos[0]["acc_bytes"] / (acc_ms * 1e-3) / 1e9
        loop_ms = sum(i["ms_loop"] for i in infos) / len(infos)
        score_ms = sum(i["ms_score"] for i in infos) / len(infos)
        # HBM traffic of the accumulation kernel: PMC counters from separate rocprofv3 --pmc passes (profiles/README.md),
        # FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for wide coalesced streams on gfx950
        traffic = None
        try:
            with open(os.path.join(ROOT, "profiles", "acc_traffic.json")) as f:
                t = json.load(f).get("%d^3 S=%d" % (args.size, args.S))
            if t:
                traffic = (2.0 * t["fetch_size_kb"] + t["write_size_kb"]) * 1024.0
        except Exception:
            pass
        out = {
            "metric": "region_merges_per_sec", "value": merges / dt, "unit": "region-merges/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u32 labels / f32 image / f64 statistics and features", "data": "synthetic",
            "config": {"workload": "%d^3 synthetic EM volume (jittered-Voronoi supervoxels S=%d, Q8 pb): K1-K3 RAG + "
                                   "boundary/region statistics accumulation, K4 edge table, K6+K7 feature vector (D_f=%d) + "
                                   "255-tree forest score of every initial edge, K5 greedy pb-mean merge tree"
                                   % (args.size, args.S, infos[0]["feat_dim"]),
                       "voxels": N, "regions": infos[0]["R"], "directed_pairs": infos[0]["P"],
                       "initial_edges": infos[0]["n_edges"], "merges_per_step": infos[0]["merges"],
                       "parallelism": "replica x%d (the merge loop does not shard)" % world},
            "edge_features_per_sec": edges / dt,
            # calls that ended with GLIA_HMT_ERR_INTERNAL (a loop's own consistency stop, or an order that failed the O(R) replay of
            # glia_hmt_check_merge_order); the library never runs a loop twice, so a healthy line carries 0 here
            "internal_errors": hmt.Context.internal_errors(),
            "phases_ms": {"accumulate": acc_ms, "edge_features_and_scores": score_ms,
                          "edge_table": sum(i["ms_table"] for i in infos) / len(infos), "merge_loop": loop_ms},
            "host_call_ms": {k: sum(i["host_ms"][k] for i in infos) / len(infos) for k in infos[0]["host_ms"]},
            "merge_loop_merges_per_sec": infos[0]["merges"] / (loop_ms * 1e-3) if loop_ms else None,
            "edge_feature_kernel_per_sec": infos[0]["n_edges"] / (score_ms * 1e-3) if score_ms else None,
            "roofline": {"bound": "hbm", "kernel": "rag_accumulate_kernel", "achieved": achieved, "peak": 8000.0,
                         "unit": "GB/s", "frac": achieved / 8000.0, "traffic": traffic,
                         "traffic_source": "profiles/acc_traffic.json (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE of tools/acc_bench.py, separate passes; not measured in this run)",
                         "algorithmic_bytes_per_launch": infos[0]["acc_bytes"], "avg_launch_ms": acc_ms},
        }
        if verify is not None:
            out["verify"] = verify
        if bc_loop is not None:
            out["bc_loop"] = bc_loop
        if args.full and not args.no_cpu:
            curve = tuple(int(x) for x in args.cpu_curve.split(",") if x)
            out["cpu_baseline"] = cpu_baseline(args.cpu_size, args.S, args.cpu_bc_size, curve, infos[0]["R"])
            # the OpenMP leg, and the SAME sample through the library's bc_feat (given order, no queue) for a like-for-like ratio
            omp = openmp_bc_feat_baseline(args.cpu_bcfeat_size, args.S // 2)
            if omp is not None:
                l2, p2 = ctx.synth((args.cpu_bcfeat_size,) * 3, args.S // 2, 4 * args.S)
                c2 = hmt.make_config(p2, rb=[(p2, 8, 0.0, 1.0)], thresholds=(0.2, 0.5, 0.8))
                rm2 = hmt.RegionMap(ctx, l2, pb=p2, only_contour=False, cfg=c2)
                o2, _ = rm2.merge_order_pb(type=2)
                rm2.bc_feat(o2)                                    # warm-up
                torch.cuda.synchronize(); ctx.sync()
                tq = time.time()
                f2 = rm2.bc_feat(o2)
                tq = time.time() - tq
                rm2.close()
                omp["gpu_same_sample"] = {"merges": len(o2), "seconds": tq, "edge_features_per_sec": len(o2) / tq, "dim": int(f2.shape[1]),
                                          "ratio_vs_openmp": (len(o2) / tq) / omp["edge_features_per_sec"][-1],
                                          "ratio_vs_1_thread": (len(o2) / tq) / omp["edge_features_per_sec"][0]}
                out["cpu_baseline"]["bc_feat"] = omp
                out["cpu_baseline"]["cores_note"] = "value / curve: 1 thread (GLIA's merge loop is single-threaded); bc_feat: %d OpenMP threads" % omp["threads"][-1]

    def emit(slab_info):
        if rank == 0:
            if slab_info is not None:
                out["slab_rag"] = slab_info     # z-slab split of ONE volume + RCCL record exchange
            print(json.dumps(out), flush=True)

    if slab:
        # Outside the timed region and never allowed to take the bench line down: an exception is reported inside the
        # line, a hang (a collective that never completes) is cut by a watchdog that emits the line without it.
        import threading

        def give_up():
            emit({"error": "slab phase did not finish within %d s" % args.slab_timeout})
            os._exit(3)         # a process that touched the GPU and lost a collective: the line is out, the exit status says so

        dog = threading.Timer(args.slab_timeout, give_up)
        dog.daemon = True
        dog.start()
        try:
            del labels, pb, cfg
            torch.cuda.empty_cache()
            slab_info = slab_phase(ctx, hmt, dist, torch, args.size, args.S, world, rank, clf)
        except Exception as e:          # noqa: BLE001
            slab_info = {"error": "%s: %s" % (type(e).__name__, e)}
        dog.cancel()
        emit(slab_info)
    else:
        emit(None)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
