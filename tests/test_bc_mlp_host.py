"""The MLP in the classifier loop, what can be checked without a GPU: the exported entry points and their argument checks (which come
before the first HIP call), the loop's limit on hidden layers, the sigmoid the loop uses against tests/_mlpdef.py's, and the argument
checks of merge_order_bc --bct 2 that precede its first read of an image.  (GPU part: test_gpu_bc_mlp.py, test_gpu_bc_mlp_cli.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np

import _mlpdef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "glia_amd", "libglia_hmt.so")
ERR_ARG = -1


def _lib():
    lib = C.CDLL(SO)
    lib.glia_hmt_last_error.restype = C.c_char_p
    return lib


def test_loop_limit_is_exported_and_covers_the_layers_the_tools_default_to():
    v = C.c_int(-1)
    assert _lib().glia_hmt_mlp_loop_limits(C.byref(v)) == 0
    assert v.value >= 32
    from glia_amd import hmt
    assert hmt.mlp_loop_limits() == {"max_hidden": v.value}
    assert hmt.mlp_limits()["max_hidden"] >= v.value        # what the loop takes, the batch predictor takes


def test_entry_points_refuse_null_arguments_before_any_device_call():
    lib = _lib()
    n = C.c_int64(-1)
    for fn, args in ((lib.glia_hmt_merge_order_bc_mlp, (None, None, None, None, None, None, C.c_int64(0), C.byref(n))),
                     (lib.glia_hmt_score_initial_edges_shard_mlp, (None, None, None, C.c_int(0), C.c_int(1), None, C.c_int64(0), C.byref(n)))):
        assert fn(*args) == ERR_ARG
        assert b"invalid argument" in lib.glia_hmt_last_error()


def test_loop_sigmoid_is_the_definitions_sigmoid():
    """step 7 of DESIGN 3.13 as the loop computes it (glia_hmt_host_libm_eval function 4, the probed variant) = _mlpdef.sigmoid, on logits
    of every size, saturated ones included"""
    lib = _lib()
    v = C.c_int(0)
    assert lib.glia_hmt_host_libm_probe_exp(C.byref(v)) == 0 and v.value in (1, 2)
    rng = np.random.default_rng(77)
    h = np.concatenate([rng.standard_normal(20000) * s for s in (0.5, 5.0, 50.0, 400.0)] + [np.array([0.0, -0.0, 36.7, 36.8, 511.9, 512.0, -745.0, -746.0,
                                                                                                     np.inf, -np.inf, np.nan])])
    out = np.empty_like(h)
    assert lib.glia_hmt_host_libm_eval(C.c_int(4), v, h.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_int64(h.size)) == 0
    assert _mlpdef.same(out, _mlpdef.sigmoid(h))
    assert (out == 1.0).any() and ((out > 0.0) & (out < 1e-300)).any() and (out == 0.0).any()


def test_tool_checks_its_classifier_arguments_first():
    """the reference's messages (hmt/main_merge_order_bc.cxx:117-118, :125); both checks come before an image is opened"""
    cli = os.path.join(ROOT, "cli")
    exe = os.path.join(cli, "merge_order_bc")
    assert os.path.exists(exe), "cli/merge_order_bc has not been built"
    common = ["-s", "none.mha", "--pb", "none.mha", "-o", os.devnull]
    r = subprocess.run([exe, "--bct", "2", "--bcm", "a", "--bcm", "b"] + common, capture_output=True, timeout=60)
    assert r.returncode == 1 and b"model distributor needs 3 arguments" in r.stderr
    r = subprocess.run([exe, "--bct", "2", "--nn1", "10", "--nn2", "10", "--bcm", "a", "--bcm", "b", "--bcm", "c", "--bcmd", "1", "--bcmd", "2"] + common,
                       capture_output=True, timeout=60)
    assert r.returncode == 1 and b"model distributor needs 3 arguments" in r.stderr
    r = subprocess.run([exe, "--bct", "3", "--bcm", "a"] + common, capture_output=True, timeout=60)
    assert r.returncode == 1 and b"unsupported classifier type" in r.stderr
