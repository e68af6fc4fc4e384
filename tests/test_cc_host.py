"""CPU-only checks of glia_hmt_label_components: the export, the option key, and every argument error -- all of them answered
before the first HIP call, so none needs a GPU.  Device pointers below are made-up addresses: they are never followed."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "glia_amd", "libglia_hmt.so")
ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "glia_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    L = C.CDLL(SO)
    L.glia_hmt_last_error.restype = C.c_char_p
    return L


def _call(lib, ctx=0x1000, dim=3, dims=(4, 5, 6), src=0x2000, mask=None, mode=0, dst=0x3000, with_n=True):
    d = None if dims is None else (C.c_int64 * 3)(*dims)
    n = C.c_uint32(12345)
    rc = lib.glia_hmt_label_components(C.c_void_p(ctx), C.c_int(dim), d, C.c_void_p(src), C.c_void_p(mask), C.c_int(mode), C.c_void_p(dst),
                                       C.byref(n) if with_n else None)
    return rc, lib.glia_hmt_last_error().decode()


def test_symbol_is_exported(lib):
    assert hasattr(lib, "glia_hmt_label_components")


def test_option_key_is_known_and_an_unknown_value_is_refused(lib):
    assert lib.glia_hmt_set_option(b"GLIA_HMT_CC", b"global") == 0
    assert lib.glia_hmt_set_option(b"GLIA_HMT_CC", b"tiled") == 0
    assert lib.glia_hmt_set_option(b"GLIA_HMT_CC", b"rows") == 0           # the table takes any string: the call refuses it
    try:
        rc, msg = _call(lib)
        assert rc == ERR_ARG and msg.startswith("label_components:") and "GLIA_HMT_CC" in msg and "rows" in msg
    finally:
        assert lib.glia_hmt_set_option(b"GLIA_HMT_CC", None) == 0


@pytest.mark.parametrize("what,kw", [
    ("NULL ctx", dict(ctx=None)),
    ("NULL dims", dict(dims=None)),
    ("NULL input", dict(src=None)),
    ("NULL output", dict(dst=None)),
    ("NULL n_components", dict(with_n=False)),
    ("dim 1", dict(dim=1)),
    ("dim 4", dict(dim=4)),
    ("zero extent", dict(dims=(4, 0, 6))),
    ("negative extent", dict(dims=(-4, 5, 6))),
    ("zero z extent in 3D", dict(dims=(4, 5, 0))),
    ("mode -1", dict(mode=-1)),
    ("mode 3", dict(mode=3)),
    ("in place", dict(src=0x2000, dst=0x2000)),
    ("2^32 - 1 voxels", dict(dims=(0xFFFFFFFF, 1, 1))),
    ("product past 2^64", dict(dims=(1 << 31, 1 << 31, 1 << 31))),
])
def test_argument_errors_come_before_any_hip_call(lib, what, kw):
    rc, msg = _call(lib, **kw)
    assert rc == ERR_ARG, what
    assert msg.startswith("label_components:"), (what, msg)


def test_dims2_is_ignored_in_2d(lib):
    """dims as for glia_hmt_watershed: a 2D call does not look at dims[2] -- with an unknown route value the call gets past the extent
    tests and stops at the option, still without a GPU"""
    assert lib.glia_hmt_set_option(b"GLIA_HMT_CC", b"none") == 0
    try:
        rc, msg = _call(lib, dim=2, dims=(4, 5, 0))
        assert rc == ERR_ARG and "GLIA_HMT_CC" in msg
        rc, msg = _call(lib, dim=3, dims=(4, 5, 0))
        assert rc == ERR_ARG and "GLIA_HMT_CC" not in msg
    finally:
        assert lib.glia_hmt_set_option(b"GLIA_HMT_CC", None) == 0


def test_header_states_the_semantics_with_the_reference_lines():
    hdr = open(os.path.join(ROOT, "include", "glia_hmt.h")).read()
    src = open(os.path.join(ROOT, "glia_amd", "csrc", "components.hip")).read()
    for text in (hdr, src):
        assert "util/image.hxx:331-373" in text and "util/image.hxx:302-313" in text
    assert "glia_hmt_label_components" in hdr and "GLIA_HMT_CC_BINARY_INVERTED" in hdr
