"""Device code of the exp / sigmoid restatements (glia_amd/csrc/glibc_math.hpp, through glia_hmt_libm_eval functions 3 and 4) against
the host code of the same restatements, bit for bit, for both variants; and the variant the context probed against the host's own exp.
CPU part: test_libm_exp.py."""
import ctypes as C
import os

import numpy as np
import pytest

import _libm_exp_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_eval(function, variant, x):
    lib = C.CDLL(os.path.join(ROOT, "glia_amd", "libglia_hmt.so"))
    out = np.empty_like(x)
    assert lib.glia_hmt_host_libm_eval(C.c_int(function), C.c_int(variant), x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                       C.c_int64(x.size)) == 0
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("function", [3, 4])
def test_device_exp_and_sigmoid_equal_the_host_restatement_bit_for_bit(function):
    import torch
    from glia_amd import hmt
    ctx = hmt.Context(0)
    v = ctx.libm_exp()
    assert v != 0, "host exp not pinned"
    x = np.ascontiguousarray(X.inputs(seed=31 + function))
    d_x = torch.from_numpy(x).cuda()
    for variant in (1, 2):
        got = ctx.libm_eval(function, variant, d_x).cpu().numpy()
        ok = X.same_bits(got, _host_eval(function, variant, x))
        assert ok.all(), "function %d variant %d: %d of %d differ, first x=%r" % (function, variant, (~ok).sum(), x.size, x[~ok][:3])
    # the probed variant is the host's own function
    got = ctx.libm_eval(function, v, d_x).cpu().numpy()
    ref = X.host_exp(x) if function == 3 else X.host_sigmoid(x)
    assert X.same_bits(got, ref).all()
    # variant 0, the device's own exp: close, not pinned
    own = ctx.libm_eval(function, 0, d_x).cpu().numpy()
    fin = np.isfinite(ref) & (ref > 1e-300)
    assert np.allclose(own[fin], ref[fin], rtol=1e-13, atol=0.0)
    ctx.close()
