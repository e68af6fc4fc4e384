"""-m gpu: the drop-in tools labelcc_image (gadget/main_labelcc_image.cxx: -i -v -r -u -z -o) and labelicc_image
(gadget/main_labelicc_image.cxx: -i -m -u -z -o) on MetaImage files, against the CPU reference of tests/_cc_cases.py."""
import os
import subprocess

import numpy as np
import pytest

import _cc_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cli")


@pytest.fixture(scope="module")
def tools():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    subprocess.check_call(["make", "-C", CLI])
    return CLI


def _tool(tools, name, labels, tmp_path, *flags, mask=None):
    src, dst = str(tmp_path / "in.mha"), str(tmp_path / "out.mha")
    K.write_mha(src, labels)
    args = [os.path.join(tools, name), "-i", src, "-o", dst] + list(flags)
    if mask is not None:
        K.write_mha(str(tmp_path / "mask.mha"), mask)
        args += ["-m", str(tmp_path / "mask.mha")]
    subprocess.check_call(args)
    return K.read_mha(dst)


def _by_size(ref, n):
    """relabel_image as include/glia_hmt.h states it: sizes descending, ties by the smaller label -- here the earlier first voxel"""
    sizes = np.bincount(ref.ravel(), minlength=n + 1)[1:].astype(np.int64)
    new = np.zeros(n + 1, np.uint32)
    new[np.lexsort((np.arange(n), -sizes)) + 1] = np.arange(1, n + 1)
    return new[ref]


@pytest.mark.parametrize("name", ["synth_mod5_cropped", "mask_random_2d"])
@pytest.mark.parametrize("invert", [False, True])
def test_labelcc_image(tools, tmp_path, name, invert):
    labels = K.case(name).labels
    if invert:
        labels = np.where(labels == 3, 0, labels).astype(np.uint32)      # some background for the inverted run to label
    ref, n = K.cc_reference(labels, None, "binary_inverted" if invert else "binary")
    got, kv = _tool(tools, "labelcc_image", labels, tmp_path, *(["-v", "1"] if invert else []))
    assert got.dtype == np.uint32 and kv["CompressedData"] == "False" and int(kv["NDims"]) == labels.ndim
    assert (got == ref).all() and got.max() == n


def test_labelcc_image_relabel_write16_compress(tools, tmp_path):
    labels = K.case("mask_random_identity").labels                     # ~a quarter background: dozens of components in both senses
    for flags, mode in ((["-r", "1"], "binary"), (["-v", "1", "-r", "1", "-u", "1", "-z", "1"], "binary_inverted")):
        ref, n = K.cc_reference(labels, None, mode)
        assert n > 3
        want = _by_size(ref, n)
        got, kv = _tool(tools, "labelcc_image", labels, tmp_path, *flags)
        assert (got == want).all()
        assert (np.diff(np.bincount(got.ravel())[1:].astype(np.int64)) <= 0).all()
        assert kv["ElementType"] == ("MET_USHORT" if "-u" in flags else "MET_UINT") and kv["CompressedData"] == str("-z" in flags)


@pytest.mark.parametrize("name", ["synth_mod5_cropped", "checker2d_two_labels", "mask_random_identity", "mask_random_2d", "mask_plane_cuts_label"])
def test_labelicc_image(tools, tmp_path, name):
    c = K.case(name)
    ref, n = K.expected(name)
    got, kv = _tool(tools, "labelicc_image", c.labels, tmp_path, mask=c.mask)
    assert got.dtype == np.uint32 and (got == ref).all() and got.max() == n


def test_labelicc_image_write16_compress(tools, tmp_path):
    c = K.case("mask_random_identity")
    ref, n = K.expected(c.name)
    assert n < 65536
    got, kv = _tool(tools, "labelicc_image", c.labels, tmp_path, "-u", "1", "-z", "1", mask=c.mask)
    assert got.dtype == np.uint16 and kv["CompressedData"] == "True" and (got == ref).all()


def test_tools_refuse_a_missing_required_option(tools, tmp_path):
    for name in ("labelcc_image", "labelicc_image"):
        r = subprocess.run([os.path.join(tools, name), "-o", str(tmp_path / "o.mha")], capture_output=True, text=True)
        assert r.returncode == 1 and "inputImage" in r.stderr
