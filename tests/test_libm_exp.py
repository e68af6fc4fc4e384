"""exp and the sigmoid built on it must carry the HOST libm's bits: the classifier loop's MLP turns its logit into the queue key with
1 / (1 + exp(-h)) (alg/nn.hxx), a saturated model gives many edges exactly 1.0, and the tie rule then decides the
order.  glibc's exp is an IFUNC with an FMA and a non-FMA build that differ in the last bit on ~0.05 % of arguments; the library restates
both (glia_amd/csrc/glibc_math.hpp) and probes which one this host runs.  CPU part: the host code of the restatement against math.exp,
bit for bit.  (GPU part: test_gpu_libm_exp.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np

import _libm_exp_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "glia_amd", "libglia_hmt.so")


def _lib():
    return C.CDLL(SO)


def _host_eval(function, variant, x):
    x = np.ascontiguousarray(x, np.float64)
    out = np.empty_like(x)
    rc = _lib().glia_hmt_host_libm_eval(C.c_int(function), C.c_int(variant), x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                       C.c_int64(x.size))
    assert rc == 0
    return out


def _probed():
    v = C.c_int(-1)
    assert _lib().glia_hmt_host_libm_probe_exp(C.byref(v)) == 0
    return v.value


def test_new_symbols_are_exported():
    lib = _lib()
    for name in ("glia_hmt_ctx_libm_exp", "glia_hmt_host_libm_probe_exp", "glia_hmt_merge_order_bc_mlp", "glia_hmt_score_initial_edges_shard_mlp",
                 "glia_hmt_mlp_loop_limits"):
        assert hasattr(lib, name), name


def test_host_exp_is_pinned_by_a_restatement():
    assert _probed() in (1, 2), "no restatement reproduces this host's exp: the MLP's saliencies in the loop are unpinned"


def test_exp_restatement_equals_host_exp_bit_for_bit():
    v = _probed()
    x = X.inputs()
    assert x.size >= 100_000
    got = _host_eval(3, v, x)
    ok = X.same_bits(got, X.host_exp(x))
    assert ok.all(), "exp variant %d: %d of %d differ, first x=%r" % (v, (~ok).sum(), x.size, x[~ok][:3])


def test_sigmoid_restatement_equals_host_sigmoid_bit_for_bit():
    v = _probed()
    x = X.inputs(seed=23)
    got = _host_eval(4, v, x)
    ok = X.same_bits(got, X.host_sigmoid(x))
    assert ok.all(), "sigmoid variant %d: %d of %d differ, first h=%r" % (v, (~ok).sum(), x.size, x[~ok][:3])
    sat = _host_eval(4, v, np.array([512.0, 600.0, 1e300, np.inf, -np.inf, 30.0, 40.0]))      # exp(-30) > 2^-53 > exp(-40)
    assert (sat[:4] == 1.0).all() and sat[4] == 0.0 and sat[5] < 1.0 and sat[6] == 1.0


def test_the_probe_can_tell_the_two_builds_apart():
    """the other build's formula differs from the host on at least one of the probe arguments"""
    v = _probed()
    x = np.array(X.PROBE)
    ref = X.host_exp(x)
    assert X.same_bits(_host_eval(3, v, x), ref).all()
    assert not X.same_bits(_host_eval(3, 3 - v, x), ref).all()


def test_host_eval_refuses_unknown_functions_and_variants():
    x = np.zeros(1)
    out = np.zeros(1)
    lib = _lib()
    def call(function, variant):
        return lib.glia_hmt_host_libm_eval(C.c_int(function), C.c_int(variant), x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_int64(1))

    for function, variant in ((5, 1), (-1, 1), (3, 0), (4, 3)):
        assert call(function, variant) != 0
    for function, value in ((3, 1.0), (4, 0.5)):          # exp(0), sigmoid(0): accepted in both variants
        for variant in (1, 2):
            out[0] = -1.0
            assert call(function, variant) == 0 and out[0] == value


def test_stand_alone_check_program():
    """cli/libm_exp_check: the header alone, compiled by the host compiler, against this host's exp"""
    cli = os.path.join(ROOT, "cli")
    subprocess.check_call(["make", "-C", cli, "libm_exp_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(cli, "libm_exp_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
