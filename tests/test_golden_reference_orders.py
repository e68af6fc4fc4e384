"""tests/golden/headline/reference_<case>.npz -- merge orders of 13 824 to 32 768 regions that the REFERENCE'S OWN engine produced
(oracle/_ref/ref_engine, recorded by tests/golden/gen_reference_orders.py, which also demanded that the oracle gives the same arrays) --
checked as data: the stored digests are those of the stored arrays, every order obeys the rule of glia_hmt_check_merge_order, mean-linkage
saliencies do not increase, and pb512's digests are the PB_512 pair that tests/test_gpu_headline.py has demanded of the device since
round 2 -- so that pair is the reference's answer, not only one the kernels gave themselves.  The oracle then recomputes, live, the reduced
twin of every case (same generator code, 128^3, S = 8, 4 096 regions; the large cases take the oracle minutes, see the generator) and
must reproduce the reference's recorded twin byte for byte: a later change of the oracle cannot drift away from the reference unnoticed.
minsize192s8 (type 3) is the oracle's own answer: the reference has no caller of that linkage and its driver no path."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_reference_orders as G                                                     # noqa: E402

PB_512 = ("652c84e7efe781bacc9df8c0a16675ca7e34cf17", "d78663710b1699d331a62c40471ba2d90ffc6515")      # = test_gpu_headline.PB_512
CASES = sorted(G.CASES)


def load(case):
    """a missing fixture is a failure, not a skip"""
    path = G.fixture_path(case)
    assert os.path.exists(path), "%s is missing (python tests/golden/gen_reference_orders.py %s)" % (path, case)
    assert os.path.getsize(path) <= 484 * 1024
    return np.load(path)


def stored_order(g, prefix):
    x0, x1 = g[prefix + "_x0"], g[prefix + "_x1"]
    assert x0.dtype == np.uint32 and x1.dtype == np.uint32 and g[prefix + "_sal"].dtype == np.float64 and len(x0) == len(x1) == len(g[prefix + "_sal"])
    x2 = (int(g[prefix + "_first_new"]) + np.arange(len(x0))).astype(np.uint32)
    return np.stack([x0, x1, x2], axis=1), g[prefix + "_sal"]


@pytest.mark.parametrize("case", CASES)
def test_fixture_is_consistent(case):
    g = load(case)
    p = G.CASES[case]
    params = json.loads(str(g["params"]))
    assert params["runs"] == [list(r) for r in p["runs"]] and all(params[k] == v for k, v in p.items() if k != "runs")
    assert ("oracle only" in params["answer_from"]) == bool(p.get("oracle_only")) == (case == "minsize192s8")
    for twin in ("", "twin_"):
        R = int(g[twin + "regions"])
        for run in p["runs"]:
            order, sal = stored_order(g, twin + run[0])
            assert G.sha(order) == str(g[twin + run[0] + "_order_sha1"]) and G.sha(sal) == str(g[twin + run[0] + "_sal_sha1"])
            first_new = int(g[twin + run[0] + "_first_new"])
            present = np.arange(1, first_new)
            if p.get("mask"):
                present = np.setdiff1d(present, g[twin + "absent_labels"])
                assert len(g[twin + "absent_labels"]) >= 1                           # the mask removed a whole supervoxel
            assert len(present) == R
            G.replay(order, present, first_new)
            if run[1] == "pb" and p["only_contour"] and not p.get("mask"):
                assert len(order) == R - 1
            if run[1] == "pb" and run[2] == 2:
                assert (np.diff(sal) <= 1e-12).all()                                 # mean linkage is reducible
            if run[1] == "pre_merge" and not twin:
                assert 0.1 * R < len(order) < 0.9 * (R - 1)
    assert int(g["regions"]) == (p["size"] // p["S"]) ** 3 - (len(g["absent_labels"]) if p.get("mask") else 0) > 10000
    assert int(g["twin_regions"]) + (len(g["twin_absent_labels"]) if p.get("mask") else 0) == 4096


def test_pb512_is_the_headline_digest():
    """the 512^3 gate of tests/test_gpu_headline.py was recorded from the GPU; the reference's engine gives the same two digests"""
    g = load("pb512")
    assert int(g["regions"]) == 32768 and len(g["type2_x0"]) == 32767
    assert (str(g["type2_order_sha1"]), str(g["type2_sal_sha1"])) == PB_512


@pytest.mark.parametrize("case", CASES)
def test_oracle_reproduces_the_recorded_twin(case):
    g = load(case)
    out, _ = G.compute(G.twin_of(G.CASES[case]), reference=False)
    keys = [k[len("twin_"):] for k in g.files if k.startswith("twin_")]
    assert sorted(keys) == sorted(out)
    for k in keys:
        a, b = np.asarray(out[k]), g["twin_" + k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
