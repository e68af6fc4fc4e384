"""CPU-only: the model file with the out-of-bag arrays in their slots (glia_amd/csrc/forest_model.hpp; ml/rf/ml_rf_model.cxx:428-448,
shaped as ml/rf/ml_rf_train.cxx:728-784 leaves them): the writer's bytes read back by a plain reader of the documented layout, a model
without the arrays byte for byte what it was, the library's parser on the longer file, the new entry points, and the stand-alone check
program of the host arithmetic."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from glia_amd import hmt, synth_forest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OOB_SYMBOLS = ("glia_hmt_oob_opts_default", "glia_hmt_forest_train_oob", "glia_hmt_forest_model_oob_sizes", "glia_hmt_forest_model_oob_arrays",
               "glia_hmt_forest_model_set_oob", "glia_hmt_last_forest_oob_timing")
# offset of the int n[2] pair of every array slot in the 520-byte header, in the order the arrays follow it; None: a scalar in between
SLOTS = (("ncat", 104, "i"), ("categorical_feature", 120, "i"), ("nrnodes", None, "i"), ("ntree", None, "i"), ("xbestsplit", 144, "d"),
         ("classwt", 160, "d"), ("cutoff", 176, "d"), ("treemap", 192, "i"), ("nodestatus", 208, "i"), ("nodeclass", 224, "i"), ("bestvar", 240, "i"),
         ("ndbigtree", 256, "i"), ("mtry", None, "i"), ("orig_labels", 280, "i"), ("new_labels", 296, "i"), ("nclass", None, "i"), ("outcl", 320, "i"),
         ("outclts", 336, "i"), ("counttr", 352, "i"), ("proximity", 368, "d"), ("proximity_tst", 384, "d"), ("localImp", 400, "d"),
         ("importance", 416, "d"), ("importanceSD", 432, "d"), ("errtr", 448, "d"), ("errts", 464, "d"), ("inbag", 480, "i"), ("votes", 496, "i"),
         ("oob_times", 512, "i"))


def read_model_file(path):
    """the whole file by its documented layout: {name: (n0, n1, flat array)} and the scalars; asserts that nothing is left over"""
    data = open(path, "rb").read()
    hdr, pos, out = data[:520], 520, {}
    for name, off, kind in SLOTS:
        if off is None:
            out[name] = struct.unpack_from("<i", data, pos)[0]
            pos += 4
            continue
        n0, n1 = struct.unpack_from("<ii", hdr, off)
        n = n0 * n1
        if n > 128:
            assert data[pos] == 0, name + ": not dense"
            pos += 1
        a = np.frombuffer(data, np.int32 if kind == "i" else np.float64, n, pos)
        pos += a.nbytes
        out[name] = (n0, n1, a)
    assert pos == len(data)
    return out


def _forest():
    f = synth_forest.synthetic_forest(ntree=9, max_depth=3, seed=11)
    f["orig_labels"] = np.array([-1, 1, 5], np.int32)
    leaves = f["nodestatus"] == -1
    f["nodeclass"][leaves] = np.random.default_rng(4).integers(1, 4, leaves.sum())
    return f


def _oob_arrays(N, D, ntree, nclass, rng):
    counttr = rng.integers(0, 4, (nclass, N)).astype(np.int32)
    times = counttr.sum(axis=0).astype(np.int32)
    return dict(counttr=counttr, votes=np.ascontiguousarray(counttr.T), oob_times=times,
                outcl=np.where(times > 0, counttr.argmax(axis=0) + 1, 0).astype(np.int32), errtr=rng.random((ntree, nclass + 1)),
                importance=rng.normal(size=(D, nclass + 2)), importanceSD=rng.random((D, nclass + 1)))


@pytest.mark.parametrize("N,D", [(200, 40), (30, 3)])          # arrays longer than 128 elements take the flag byte, shorter ones do not
def test_writer_with_the_tail_arrays_parses_back(tmp_path, N, D):
    f = _forest()
    p_plain, p_oob, p_imp, p_both = (str(tmp_path / n) for n in ("plain.bin", "oob.bin", "imp.bin", "both.bin"))
    model = hmt.ForestModel.from_arrays(f)
    model.write(p_plain)
    with pytest.raises(hmt.HmtError) as e:
        model.oob()
    assert e.value.code == hmt.ERR_ARG and "no out-of-bag arrays" in str(e.value)
    a = _oob_arrays(N, D, 9, 3, np.random.default_rng(N))
    groups = (("outcl", "counttr", "votes", "oob_times", "errtr"), ("importance", "importanceSD"))
    model.set_oob(N, D, {k: a[k] for k in groups[0]})
    model.write(p_oob)
    assert sorted(model.oob()) == sorted(groups[0] + ("err_wrong", "err_seen"))
    model.set_oob(N, D, {k: a[k] for k in groups[1]})
    model.write(p_imp)
    assert sorted(model.oob()) == sorted(groups[1])
    model.set_oob(N, D, a)
    model.write(p_both)
    back = model.oob()
    for k in a:
        assert back[k].dtype == a[k].dtype and back[k].shape == a[k].shape and (back[k] == a[k]).all(), k
    plain = read_model_file(p_plain)
    shapes = dict(outcl=(N, 1), counttr=(3, N), importance=(D, 5), importanceSD=(D, 4), errtr=(9, 4), votes=(N, 3), oob_times=(N, 1))
    for path, held in ((p_plain, ()), (p_oob, groups[0]), (p_imp, groups[1]), (p_both, groups[0] + groups[1])):
        got = read_model_file(path)
        for name, off, _ in SLOTS:
            if off is None or name not in shapes:
                # everything in front of the tail, and the slots this library leaves empty, as in the file without it
                assert got[name] == plain[name] if off is None else (got[name][:2] == plain[name][:2] and (got[name][2] == plain[name][2]).all()), name
            elif name in held:
                assert got[name][:2] == shapes[name] and (got[name][2] == a[name].reshape(-1)).all(), name
            else:
                assert got[name][:2] == (0, 0), name
    assert open(p_both, "rb").read()[:len(open(p_plain, "rb").read())][520:] == open(p_plain, "rb").read()[520:]


def test_a_model_without_them_is_the_bytes_of_the_python_writer(tmp_path):
    f = _forest()
    p_py, p_cc, p_again = (str(tmp_path / n) for n in ("py.bin", "cc.bin", "again.bin"))
    synth_forest.write_model(p_py, f)
    hmt.ForestModel.from_arrays(f).write(p_cc)
    assert open(p_cc, "rb").read() == open(p_py, "rb").read()
    assert all(read_model_file(p_cc)[k][:2] == (0, 0) for k in ("outcl", "counttr", "importance", "importanceSD", "errtr", "votes", "oob_times"))


def test_the_parser_accepts_the_longer_file(tmp_path):
    f = _forest()
    p_plain, p_both = str(tmp_path / "plain.bin"), str(tmp_path / "both.bin")
    model = hmt.ForestModel.from_arrays(f)
    model.write(p_plain)
    model.set_oob(200, 40, _oob_arrays(200, 40, 9, 3, np.random.default_rng(1)))
    model.write(p_both)
    L = hmt.lib()
    parsed = []
    for path in (p_plain, p_both):
        nt, nn, nc = C.c_int(), C.c_int(), C.c_int()
        split = np.empty(f["xbestsplit"].shape)
        meta = np.empty(f["xbestsplit"].shape + (4,), np.int32)
        assert L.glia_hmt_forest_file_parse(path.encode(), C.c_int(5), C.byref(nt), C.byref(nn), C.byref(nc), split.ctypes.data_as(C.c_void_p),
                                            meta.ctypes.data_as(C.c_void_p), C.c_int64(split.size)) == 0
        parsed.append((nt.value, nn.value, nc.value, split.tobytes(), meta.tobytes()))
    assert parsed[0] == parsed[1] and parsed[0][:3] == (9, 15, 3)


def test_set_oob_refuses_half_a_group():
    model = hmt.ForestModel.from_arrays(_forest())
    a = _oob_arrays(30, 3, 9, 3, np.random.default_rng(2))
    for keys in ((), ("outcl", "counttr"), ("importance",)):
        with pytest.raises(hmt.HmtError) as e:
            model.set_oob(30, 3, {k: a[k] for k in keys})
        assert e.value.code == hmt.ERR_ARG


def test_oob_symbols_are_exported_and_declared():
    L = hmt.lib()
    hdr = open(os.path.join(ROOT, "include", "glia_hmt.h")).read()
    for n in OOB_SYMBOLS:
        assert hasattr(L, n), "missing export: " + n
        assert n + "(" in hdr, "not declared: " + n
    o = hmt.OobOpts(7, 7)
    L.glia_hmt_oob_opts_default(C.byref(o))
    assert (o.oob, o.importance) == (0, 0)
    assert C.sizeof(hmt.TrainOpts) == 40                                      # glia_hmt_train_opts is mirrored by callers: unchanged


def test_stand_alone_check_program(tmp_path):
    """cli/forest_oob_check: the host arithmetic of the out-of-bag outputs and the writer's optional arrays without the library (the
    program a sanitizer build runs, cli/Makefile); the file it writes reads back by the documented layout"""
    cli = os.path.join(ROOT, "cli")
    subprocess.check_call(["make", "-C", cli, "forest_oob_check"], stdout=subprocess.DEVNULL)
    p = str(tmp_path / "check.bin")
    r = subprocess.run([os.path.join(cli, "forest_oob_check"), p], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "OK\n", r.stderr
    got = read_model_file(p)
    assert got["outcl"][:2] == (200, 1) and got["counttr"][:2] == (3, 200) and got["votes"][:2] == (200, 3) and got["oob_times"][:2] == (200, 1)
    assert got["errtr"][:2] == (9, 4) and got["importance"][:2] == (3, 5) and got["importanceSD"][:2] == (3, 4)
    assert (got["counttr"][2].reshape(3, 200) == got["votes"][2].reshape(200, 3).T).all() and (got["oob_times"][2] == 2).all()
    assert (got["errtr"][2] == 0.125).all() and (got["importance"][2] == 0.5).all() and (got["importanceSD"][2] == 0.25).all()
