"""CPU-only: the C++ writer of the GLIA model file (glia_hmt_forest_model_write, glia_amd/csrc/forest_model.hpp) against the Python one
(glia_amd/synth_forest.write_model) byte for byte, read back by the library's parser; the Python writer's default bytes pinned to what
the commit before its new keywords wrote; the training entry points exported."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

from glia_amd import hmt, synth_forest

TRAIN_SYMBOLS = ("glia_hmt_train_opts_default", "glia_hmt_forest_train", "glia_hmt_forest_model_from_arrays", "glia_hmt_forest_model_sizes",
                 "glia_hmt_forest_model_arrays", "glia_hmt_forest_model_write", "glia_hmt_forest_model_free", "glia_hmt_forest_from_model",
                 "glia_hmt_last_forest_train_timing")
# sha256 of write_model(synthetic_forest(ntree=3, max_depth=3)) (1688 bytes), computed on the commit before write_model had keywords
PARENT_DIGEST = "786f9a41c9275864e5ccb148af9e93623e7c651b317c8f465275af28ca620284"


def _hand_made():
    """9 trees x 15 nodes, three classes: the tree arrays (135 and 270 elements) take the dense-flag byte, the per-class and per-tree
    arrays (3 and 9 elements) do not"""
    f = synth_forest.synthetic_forest(ntree=9, max_depth=3, seed=11)
    ntree, nrnodes = f["xbestsplit"].shape
    assert nrnodes == 15 and ntree * nrnodes > 128 > ntree
    rng = np.random.default_rng(4)
    f["orig_labels"] = np.array([-1, 1, 5], np.int32)
    leaves = f["nodestatus"] == -1
    f["nodeclass"][leaves] = rng.integers(1, 4, leaves.sum())
    f["mtry"] = 7
    f["classwt"] = np.array([1.0, 2.5, 1.0 / 3.0])
    f["cutoff"] = np.array([0.5, 0.25, 0.25])
    return f


def test_cxx_writer_equals_python_writer_and_parses_back(tmp_path):
    f = _hand_made()
    p_py, p_cc = str(tmp_path / "py.bin"), str(tmp_path / "cc.bin")
    synth_forest.write_model(p_py, f, mtry=f["mtry"], classwt=f["classwt"], cutoff=f["cutoff"])
    model = hmt.ForestModel.from_arrays(f)
    model.write(p_cc)
    assert open(p_cc, "rb").read() == open(p_py, "rb").read()
    back = model.arrays()
    for k in ("xbestsplit", "treemap", "nodestatus", "nodeclass", "bestvar", "ndbigtree", "classwt", "cutoff", "orig_labels"):
        assert (back[k] == f[k]).all(), k
    assert back["mtry"] == 7 and (back["new_labels"] == [1, 2, 3]).all()
    L = hmt.lib()
    for label, target in ((-1, 1), (5, 3)):
        nt, nn, nc = C.c_int(), C.c_int(), C.c_int()
        split = np.empty(f["xbestsplit"].shape)
        meta = np.empty(f["xbestsplit"].shape + (4,), np.int32)
        assert L.glia_hmt_forest_file_parse(p_cc.encode(), C.c_int(label), C.byref(nt), C.byref(nn), C.byref(nc), split.ctypes.data_as(C.c_void_p),
                                            meta.ctypes.data_as(C.c_void_p), C.c_int64(split.size)) == 0
        assert (nt.value, nn.value, nc.value) == (9, 15, 3)
        used = np.arange(15)[None, :] < f["ndbigtree"][:, None]
        inner, leaf = used & (f["nodestatus"] == 1), used & (f["nodestatus"] == -1)
        assert (split[used] == f["xbestsplit"][used]).all()
        assert (meta[..., 0][inner] == f["bestvar"][inner] - 1).all() and (meta[..., 1][inner] == f["treemap"][..., 0][inner] - 1).all()
        assert (meta[..., 2][inner] == f["treemap"][..., 1][inner] - 1).all() and (meta[..., 3][inner] == -1).all()
        assert (meta[..., 3][leaf] == (f["nodeclass"][leaf] == target)).all()
    assert L.glia_hmt_forest_file_parse(p_cc.encode(), C.c_int(3), C.byref(nt), C.byref(nn), C.byref(nc), None, None, C.c_int64(0)) == -1


def test_writer_refuses_what_it_cannot_write(tmp_path):
    model = hmt.ForestModel.from_arrays(_hand_made())
    try:
        model.write(str(tmp_path / "no_such_directory" / "m.bin"))
    except hmt.HmtError as e:
        assert e.code == -6 and "cannot create file" in str(e)
    else:
        raise AssertionError("a model was written into a directory that does not exist")


def test_stand_alone_check_program(tmp_path):
    """cli/forest_model_check: the option arithmetic and the writer without the library (the program a sanitizer build runs, cli/Makefile);
    the file it writes is the Python writer's for the same arrays"""
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cli")
    subprocess.check_call(["make", "-C", cli, "forest_model_check"], stdout=subprocess.DEVNULL)
    p, q = str(tmp_path / "check.bin"), str(tmp_path / "py.bin")
    r = subprocess.run([os.path.join(cli, "forest_model_check"), p], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "OK\n", r.stderr
    f = dict(xbestsplit=np.zeros((9, 15)), treemap=np.zeros((9, 15, 2), np.int32), nodestatus=np.zeros((9, 15), np.int32),
             nodeclass=np.zeros((9, 15), np.int32), bestvar=np.zeros((9, 15), np.int32), ndbigtree=np.full(9, 3, np.int32),
             orig_labels=np.array([-1, 1, 5], np.int32))
    for t in range(9):
        f["xbestsplit"][t, 0] = 0.25 * t
        f["bestvar"][t, 0] = 1 + t
        f["nodestatus"][t, :3] = (1, -1, -1)
        f["treemap"][t, 0] = (2, 3)
        f["nodeclass"][t, 1:3] = (1 + t % 3, 1 + (t + 1) % 3)
    synth_forest.write_model(q, f, mtry=7, classwt=[1.0, 2.5, 1.0 / 3.0], cutoff=[0.5, 0.25, 0.25])
    assert open(p, "rb").read() == open(q, "rb").read()


def test_python_writer_defaults_are_the_bytes_of_the_parent_commit(tmp_path):
    p = str(tmp_path / "m.bin")
    synth_forest.write_model(p, synth_forest.synthetic_forest(ntree=3, max_depth=3))
    data = open(p, "rb").read()
    assert len(data) == 1688 and hashlib.sha256(data).hexdigest() == PARENT_DIGEST
    q = str(tmp_path / "q.bin")
    synth_forest.write_model(q, synth_forest.synthetic_forest(ntree=3, max_depth=3), mtry=3, classwt=[1.0, 1.0], cutoff=[0.5, 0.5])
    assert open(q, "rb").read() == data


def test_training_symbols_are_exported_and_declared():
    L = hmt.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glia_hmt.h")).read()
    for n in TRAIN_SYMBOLS:
        assert hasattr(L, n), "missing export: " + n
        assert n + "(" in hdr, "not declared: " + n
    o = hmt.TrainOpts()
    L.glia_hmt_train_opts_default(C.byref(o))
    assert (o.ntree, o.mtry, o.sample_ratio, o.nodesize, o.balance, o.max_depth, o.seed) == (255, 0, 0.7, 1, 1, 0, 0x9E3779B97F4A7C15)
