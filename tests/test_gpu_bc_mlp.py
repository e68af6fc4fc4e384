"""The MLP as the classifier of the merge loop (glia_hmt_merge_order_bc_mlp, merge_order_bc --bct 2; glia_amd/csrc/greedy_bc.hip:
classify_serial for the initial edges, mlp_chunk per round).  All images are Q8 but one: the float32 volume at the end of part 3, where the loop is compared with itself.

1. One-column models (tests/_bc_mlp_cases.py): the probability is a function F(mean of the shared boundary) alone, so the second
   author tests/_loopdef.py gives the expected order and saliencies, ties included -- on the hub image, whose contractions cross W.cap
   several times, and on the thin hub image under every instance tier and the smallest capacities.  F comes from tests/_mlpdef.py.
   One threshold on the columns {x0.b0.mean, bias} can separate two members of an ensemble, never three (the bias column is 1.0 on every
   row): two ensembles with the dimensions exchanged reach members {0, 2} and {1, 2}; all three in one run are part 3's.
2. Dense weights against a brute-force author (tests/_loopdef_rows.py: _loopdef's table and tie rules, every new edge scored from its
   full _featdef row by _mlpdef) on a 30-region image: the order exactly, where the replay's best and second-best saliency are equal or
   more than 1e-9 apart at every step (checked on the CPU); the saliencies against the host predictor on the returned rows.
3. Identities on a 32^3 synth volume (64 regions) under dense random models: returned rows = bc_feat_batch rows of the returned order,
   saliencies = the host predictor on the returned rows, initial scores = the host predictor on the initial rows record by record,
   shards, two calls.
4. Refusals."""

import numpy as np
import pytest

import _bc_mlp_cases as M
import _bc_mlp_dense_cases as DC
import _featdef
import _loopdef
import _loopdef_rows
import _mlpdef
from _hub_cases import hub_image, thin_hub_image

kLimit = 32                        # glia_hmt_mlp_loop_limits, asserted below
IMAGES = {"hub": lambda: hub_image(None), "thin30": lambda: thin_hub_image(30)}
_cpu, _dev = {}, {}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _image(name):
    if ("img", name) not in _cpu:
        lab, pb = IMAGES[name]()
        _cpu["img", name] = (lab, pb)
        _cpu["leaves", name] = _loopdef.leaf_pairs(lab, pb)
    return _cpu["img", name]


def _models():
    if "models" not in _cpu:
        _cpu["models"] = M.models(kLimit)
    return _cpu["models"]


def _F(model):
    m = _models()[model]
    return M.score_of(m["weights"], m["n1"], m["n2"], m["mn"], m["mx"], m["dist"])


def _reference(name, model):
    """generate() under the model's F, once"""
    key = ("ref", name, model)
    if key not in _cpu:
        lab, pb = _image(name)
        _cpu[key] = _loopdef.generate(lab, pb, F=_F(model), leaves=_cpu["leaves", name])
    return _cpu[key]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from glia_amd import hmt
    c = hmt.Context(0)
    assert c.libm_exp() != 0, "host exp not pinned"
    assert hmt.mlp_loop_limits()["max_hidden"] == kLimit
    yield c
    c.close()
    _dev.clear()


def _rm(ctx, name):
    from glia_amd import hmt
    if name not in _dev:
        import torch
        lab, pb = _image(name)
        _dev[name] = (torch.from_numpy(lab.view(np.int32)).cuda(), torch.from_numpy(pb).cuda())
    d_lab, d_pb = _dev[name]
    rm = hmt.RegionMap(ctx, d_lab, pb=d_pb, cfg=hmt.make_config(d_pb, rb=[(d_pb, 8, 0.0, 1.0)]))
    assert rm.feat_dim() == M.DIM
    return rm


def _mlp(ctx, m):
    from glia_amd import hmt
    return hmt.MLP.from_arrays(ctx, m["weights"], m["n1"], m["n2"], m["mn"], m["mx"], m["dist"])


def _same(got, ref):
    return got[0].shape == ref[0].shape and (got[0] == ref[0]).all() and (_bits(got[1]) == _bits(ref[1])).all()


MODELS = ["10+10", "1+1", "limit", "10+10 minmax", "dead relu", "saturated", "ensemble 0/2", "ensemble 1/2"]


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_one_column_models_on_the_hub_image(ctx, model):
    from glia_amd import hmt
    lab, pb = _image("hub")
    ref = _reference("hub", model)
    m = _models()[model]
    assert len(ref[0]) == 1800
    if model == "dead relu":
        assert len(np.unique(ref[1])) < len(ref[1]), "the tie rule decides merges"
        assert len(np.unique(_F(model)(np.linspace(0.0, 0.29, 30)))) == 1
    if model == "saturated":
        assert (ref[1] == 1.0).any() and (ref[1] < 1e-300).any()
    if model.startswith("ensemble"):
        reached = np.unique(M.picks(m, np.arange(256) / 256.0)).tolist()
        assert reached == ([0, 2] if model.endswith("0/2") else [1, 2])
    clf = _mlp(ctx, m)
    before = hmt.Context.internal_errors()
    rm = _rm(ctx, "hub")
    o, s, f = rm.merge_order_bc(clf, want_feats=True)
    rm.close()
    step = _loopdef.check(lab, pb, o, s, F=_F(model), explain=True, leaves=_cpu["leaves", "hub"])
    assert step == (-1, ""), step
    assert _same((o, s), ref)
    # the saliencies are the host predictor's values of the returned (raw) rows, and F of their column
    assert (_bits(s) == _bits(clf.predict_host(f))).all()
    assert (_bits(s) == _bits(_F(model)(f[:, M.STUB]))).all()
    clf.close()
    assert hmt.Context.internal_errors() == before == 0


@pytest.mark.gpu
@pytest.mark.parametrize("env", [dict(), dict(GLIA_HMT_MINCAP=1), dict(GLIA_HMT_BC_GENERIC=1, GLIA_HMT_BC_NOCOMMON=1)])
def test_thin_hub_image_and_the_smallest_capacities(ctx, env):
    """The MLP has ONE instance of the loop kernel (greedy_bc_mlp), whatever the tier switches say: the third case only shows that they
    are ignored for it.  The smallest capacities (device arrays that grow during the run) are a path of their own."""
    from glia_amd import hmt
    ref = _reference("thin30", "10+10 minmax")
    assert len(ref[0]) == 900
    clf = _mlp(ctx, _models()["10+10 minmax"])
    before = hmt.Context.internal_errors()
    with hmt.options(**env):
        rm = _rm(ctx, "thin30")
        got = rm.merge_order_bc(clf)
        rm.close()
    assert _same(got, ref), env
    clf.close()
    assert hmt.Context.internal_errors() == before == 0


@pytest.mark.gpu
def test_a_spoilt_weight_is_noticed(ctx):
    """the output bias changed by a quarter: check() under the unspoilt F names a step"""
    lab, pb = _image("hub")
    m = dict(_models()["10+10"])
    w = m["weights"].copy()
    w[-1] += 0.25
    m["weights"] = w
    clf = _mlp(ctx, m)
    rm = _rm(ctx, "hub")
    o, s = rm.merge_order_bc(clf)
    rm.close()
    clf.close()
    step, why = _loopdef.check(lab, pb, o, s, F=_F("10+10"), explain=True, leaves=_cpu["leaves", "hub"])
    assert 0 <= step < len(o) and why, (step, why)


# ---- 2. dense weights against the brute-force author --------------------------------------------------------------------------------
def _dense_case():
    """the image, both models, and per model the replay (order, saliencies, gaps, RowReplay): computed once, on the CPU"""
    if "dense" not in _cpu:
        lab, pb = DC.image()
        _, rows = _loopdef_rows.initial_rows(lab, pb)
        models = DC.models(rows, rows.shape[1])
        _cpu["dense"] = (lab, pb, models, {k: _loopdef_rows.generate(lab, pb, m) for k, m in models.items()})
    return _cpu["dense"]


@pytest.mark.parametrize("model", ["10+10 minmax", "ensemble"])
def test_dense_replay_is_decided_far_from_rounding(model):
    """no GPU: at every step the best and the second-best saliency are exactly equal or more than 1e-9 apart, so a last-ulp difference
    between Python-summed and device-summed features cannot decide a merge; no initial edge joins regions of equal area"""
    lab, pb, models, ref = _dense_case()
    assert len(np.unique(lab)) == 30 and lab.size <= 2000 and models[model]["weights"] is not None
    o, s, gaps, rp = ref[model]
    assert len(o) == 29 and rp.equal_area_edges == 0
    assert ((gaps == 0.0) | (gaps > 1e-9)).all(), gaps.min()
    assert len(np.unique(s)) > 8
    if model == "ensemble":
        m = models[model]
        assert np.unique(_mlpdef.pick(_mlpdef.prepare(np.array(rp.rows_scored), m["mn"], m["mx"]), m["dist"])).tolist() == [0, 1, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["10+10 minmax", "ensemble"])
def test_dense_models_against_the_brute_force_author(ctx, model):
    import torch
    from glia_amd import hmt
    lab, pb, models, ref = _dense_case()
    o_ref, s_ref, _, _ = ref[model]
    d_lab, d_pb = torch.from_numpy(lab.view(np.int32)).cuda(), torch.from_numpy(pb).cuda()
    rm = hmt.RegionMap(ctx, d_lab, pb=d_pb, cfg=hmt.make_config(d_pb, rb=[(d_pb, 8, 0.0, 1.0)]))
    clf = _mlp(ctx, models[model])
    before = hmt.Context.internal_errors()
    o, s, f = rm.merge_order_bc(clf, want_feats=True)
    assert o.shape == o_ref.shape and (o == o_ref).all(), np.flatnonzero((o != o_ref).any(1))[:3]
    assert (_bits(s) == _bits(clf.predict_host(f))).all()
    assert np.allclose(s, s_ref, rtol=0.0, atol=1e-10)          # Python-summed features: the last ulps of a row are its own
    rm.close()
    clf.close()
    assert hmt.Context.internal_errors() == before == 0


# ---- 3. identities on a synth volume under dense models ----------------------------------------------------------------------------
def _dense_models(dim, rows):
    """random dense weights; the min/max table spans the columns of `rows` (the stub scorer's run), so that rescaled values stay in
    [-1, 1] and the models do not saturate"""
    rng = np.random.default_rng(323232)
    mn, mx = rows.min(0) - 0.25, rows.max(0) + 0.25
    one = dict(weights=rng.standard_normal(_mlpdef.n_weights(dim, 10, 10)) * 0.4, n1=10, n2=10, mn=mn, mx=mx, dist=None)
    ws = [rng.standard_normal(_mlpdef.n_weights(dim, 7, 12)) * 0.4 for _ in range(3)]
    return {"10+10 minmax": one, "ensemble": dict(weights=ws, n1=7, n2=12, mn=mn, mx=mx, dist=None)}


def _synth_map(ctx):
    from glia_amd import hmt
    if "synth" not in _dev:
        import torch
        from oracle import pyoracle as O
        labels, pb = O.synth((32,) * 3, 8, 16)
        _cpu["synth"] = (labels, pb)
        _dev["synth"] = (torch.from_numpy(labels.view(np.int32)).cuda(), torch.from_numpy(pb).cuda())
    labels, pb = _dev["synth"]
    rm = hmt.RegionMap(ctx, labels, pb=pb, cfg=hmt.make_config(pb, rb=[(pb, 8, 0.0, 1.0)]))
    assert rm.num_regions == 64
    return rm


def _initial_rows(rm):
    """(is a record a table edge [records], the rows of the table edges): the initial records are one per unordered adjacent leaf pair,
    lexicographic, the mutual pairs being the table edges; TBoundaryTable::init hands a pair over in the region map's iteration order
    (the oracle's region_iter_order).  The row of an initial edge is the bc_feat_batch row of an order in which it merges two leaves; a
    merge of two OTHER leaves changes nothing it reads, so matchings of edges share a call (as tests/test_gpu_median_init.py)."""
    if "synth rows" not in _cpu:
        from oracle import pyoracle as O
        from test_gpu_median_init import _matchings, _records
        rag = O.Rag(_cpu["synth"][0])
        par = rm.pairs()
        rec = _records(par["a"], par["b"])
        rank = {int(l): i for i, l in enumerate(rag.region_iter_order())}
        edges = [(x, y) if rank[x] < rank[y] else (y, x) for x, y, m in rec if m]
        key = int(_cpu["synth"][0].max()) + 1
        rows = None
        for m in _matchings(edges):
            order = np.array([[edges[i][0], edges[i][1], key + k] for k, i in enumerate(m)], np.uint32)
            f = rm.bc_feat_batch(order)
            rows = np.empty((len(edges), f.shape[1])) if rows is None else rows
            rows[m] = f
        _cpu["synth rows"] = (np.array([m for _, _, m in rec], bool), rows)
    return _cpu["synth rows"]


def _rows_are_batch_rows(rm, f, o):
    """as test_gpu_wide_linkages._rows_are: on equal areas the loop's row may be the row of the swapped pair"""
    r = rm.bc_feat_batch(o)
    assert f.shape == r.shape
    bad = ~(_bits(f) == _bits(r)).all(1)
    if bad.any():
        swapped = o.copy()
        swapped[:, [0, 1]] = o[:, [1, 0]]
        assert (_bits(f[bad]) == _bits(rm.bc_feat_batch(swapped)[bad])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["10+10 minmax", "ensemble"])
def test_identities_on_a_synth_volume(ctx, model):
    from glia_amd import hmt
    before = hmt.Context.internal_errors()
    rm = _synth_map(ctx)
    dim = rm.feat_dim()
    names = _featdef.column_names(3, 3, [8], [], [8])
    assert len(names) == dim
    _, _, stub_f = rm.merge_order_bc(hmt.FeatureStubClassifier(ctx, names.index("x0.b0.mean")), want_feats=True)
    m = _dense_models(dim, stub_f)[model]
    if model == "ensemble":
        # The distributor reads two rescaled columns under ONE threshold: their min/max entries are centred on the columns' means over
        # the stub scorer's rows, so that 0.0 splits both.  Which rows the loop returns depends on the model, so the pair of columns is
        # searched: the first pair whose run reaches all three members is the one the identities below are checked on.
        cols = [names.index(c) for c in ("x0.b0.mean", "x1.area", "x0.blen", "x2.r0.mean", "x1.r0.std", "x3.b0.mean", "x2.area", "x0.area_diff")]
        found = None
        for d0 in cols:
            for d1 in cols:
                if d0 == d1 or found is not None:
                    continue
                mn, mx = m["mn"].copy(), m["mx"].copy()
                for d in (d0, d1):
                    mid, half = float(np.mean(stub_f[:, d])), float(np.ptp(stub_f[:, d])) + 1.0
                    mn[d], mx[d] = mid - half, mid + half
                cand = dict(m, mn=mn, mx=mx, dist=(float(d0), float(d1), 0.0))
                clf = _mlp(ctx, cand)
                _, s, f = rm.merge_order_bc(clf, want_feats=True)
                assert (_bits(s) == _bits(clf.predict_host(f))).all(), (d0, d1)
                clf.close()
                if np.unique(_mlpdef.pick(_mlpdef.prepare(f, mn, mx), cand["dist"])).tolist() == [0, 1, 2]:
                    found = cand
        assert found is not None, "no pair of columns sends the loop's rows to all three members"
        m = found
    clf = _mlp(ctx, m)
    o, s, f = rm.merge_order_bc(clf, want_feats=True)
    assert len(o) == 63
    _rows_are_batch_rows(rm, f, o)
    pred, logit = clf.predict_host(f, want_logits=True)
    assert (_bits(s) == _bits(pred)).all()
    assert _mlpdef.same(logit, _mlpdef.logits(m["weights"], m["n1"], m["n2"], f, m["mn"], m["mx"], m["dist"]))
    assert _mlpdef.same(s, _mlpdef.sigmoid(logit))
    assert len(np.unique(s)) > 8
    # two calls are byte-identical
    o2, s2, f2 = rm.merge_order_bc(clf, want_feats=True)
    assert o2.tobytes() == o.tobytes() and s2.tobytes() == s.tobytes() and f2.tobytes() == f.tobytes()
    # the initial edges: the host predictor on the initial rows, record by record; -inf on the records that are no table edges
    table, rows0 = _initial_rows(rm)
    init = rm.score_initial_edges_shard(clf, 0, 1)
    assert len(init) == len(table) and (np.isfinite(init) == table).all() and (init[~table] == -np.inf).all()
    assert (_bits(init[table]) == _bits(clf.predict_host(rows0))).all()
    parts = [rm.score_initial_edges_shard(clf, k, 3) for k in range(3)]
    assert all(p.shape == init.shape for p in parts)
    assert (_bits(np.maximum.reduce(parts)) == _bits(init)).all()
    assert sum(int(np.isfinite(p).sum()) for p in parts) == int(table.sum()) > 0
    if model == "ensemble":
        picked = np.unique(_mlpdef.pick(_mlpdef.prepare(f, m["mn"], m["mx"]), m["dist"])).tolist()
        assert picked == [0, 1, 2], picked
    rm.close()
    clf.close()
    assert hmt.Context.internal_errors() == before == 0


@pytest.mark.gpu
def test_no_setting_changes_a_result_on_a_float32_volume(ctx):
    """The one image here that is not Q8: synth's variant=1 volume of tests/test_gpu_bc.py (float32 values, inexact f64 sums, 16
    bins).  On ONE map object (the RAG pass may differ from run to run in the last bit of an inexact sum) order, saliencies and
    popped rows are byte-identical under the tier switches and the smallest capacities, and the saliencies are the host predictor's
    values of the returned rows.  The MLP loop has no helper workgroups: every record is scored by the loop's own workgroup."""
    import torch
    from glia_amd import hmt
    from oracle import pyoracle as O
    labels, pb = O.synth((33, 30, 40), 5, 20, variant=1)
    assert np.unique(np.round(pb.astype(np.float64) * 256) - pb.astype(np.float64) * 256).size > 100, "not a Q8 volume"
    d_lab, d_pb = torch.from_numpy(labels.view(np.int32)).cuda(), torch.from_numpy(pb).cuda()
    before = hmt.Context.internal_errors()
    rm = hmt.RegionMap(ctx, d_lab, pb=d_pb, cfg=hmt.make_config(d_pb, rb=[(d_pb, 16, 0.0, 1.0)]))
    names = _featdef.column_names(3, 3, [16], [], [16])
    assert len(names) == rm.feat_dim()
    _, _, stub_f = rm.merge_order_bc(hmt.FeatureStubClassifier(ctx, names.index("x0.b0.mean")), want_feats=True)
    clf = _mlp(ctx, _dense_models(rm.feat_dim(), stub_f)["10+10 minmax"])
    o, s, f = rm.merge_order_bc(clf, want_feats=True)
    assert len(o) == len(np.unique(labels)) - 1 and len(np.unique(s)) > 8
    assert (_bits(s) == _bits(clf.predict_host(f))).all()
    for env in (dict(GLIA_HMT_BC_NOCOMMON=1), dict(GLIA_HMT_BC_GENERIC=1), dict(GLIA_HMT_MINCAP=1)):
        with hmt.options(**env):
            o2, s2, f2 = rm.merge_order_bc(clf, want_feats=True)
        assert o2.tobytes() == o.tobytes() and s2.tobytes() == s.tobytes() and f2.tobytes() == f.tobytes(), env
    rm.close()
    clf.close()
    assert hmt.Context.internal_errors() == before == 0


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(ctx):
    from glia_amd import hmt
    rng = np.random.default_rng(4)
    rm = _rm(ctx, "thin30")
    dim = M.DIM

    def refused(clf, rmap, *words):
        for call in (lambda: rmap.merge_order_bc(clf), lambda: rmap.score_initial_edges_shard(clf, 0, 1)):
            with pytest.raises(hmt.HmtError) as e:
                call()
            assert e.value.code == hmt.ERR_ARG, str(e.value)
            for w in words:
                assert w in str(e.value), str(e.value)

    for n1, n2 in ((kLimit + 1, 10), (10, kLimit + 1)):
        clf = hmt.MLP.from_arrays(ctx, rng.standard_normal(_mlpdef.n_weights(dim, n1, n2)), n1, n2)
        refused(clf, rm, "at most %d units" % kLimit, str(kLimit + 1))
        clf.close()
    clf = hmt.MLP.from_arrays(ctx, rng.standard_normal(dim + 1), 0, 0)
    refused(clf, rm, "logsig")
    clf.close()
    clf = hmt.MLP.from_arrays(ctx, rng.standard_normal(_mlpdef.n_weights(dim + 1, 10, 10)), 10, 10)
    refused(clf, rm, "%d columns" % (dim + 1), str(dim))
    clf.close()
    rm.close()
    d_lab, d_pb = _dev["thin30"]
    med = hmt.RegionMap(ctx, d_lab, pb=d_pb, cfg=hmt.make_config(d_pb, rb=[(d_pb, 8, 0.0, 1.0)], use_median_features=True))
    clf = hmt.MLP.from_arrays(ctx, rng.standard_normal(_mlpdef.n_weights(med.feat_dim(), 10, 10)), 10, 10)
    refused(clf, med, "GLIA_USE_MEDIAN_AS_FEATS")
    clf.close()
    med.close()
    # the limit itself is taken
    ok = hmt.MLP.from_arrays(ctx, rng.standard_normal(_mlpdef.n_weights(dim, kLimit, kLimit)), kLimit, kLimit)
    rm = _rm(ctx, "thin30")
    assert len(rm.merge_order_bc(ok)[0]) == 900
    rm.close()
    ok.close()
    assert hmt.Context.internal_errors() == 0
