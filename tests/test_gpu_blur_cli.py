"""-m gpu: the drop-in tool blur_image (gadget/main_blur_image.cxx: -i -s -k -d -z -o) on MetaImage files of float, uchar and ushort
pixels, against the host definition (glia_hmt_blur_image_host) -- equality of bytes."""
import os
import subprocess

import numpy as np
import pytest

import _blurdef as D
from glia_amd import hmt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cli")


@pytest.fixture(scope="module")
def tool():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    subprocess.check_call(["make", "-C", CLI, "blur_image"], stdout=subprocess.DEVNULL)
    return os.path.join(CLI, "blur_image")


def _run(tool, img, tmp_path, *flags):
    src, dst = str(tmp_path / "in.mha"), str(tmp_path / "out.mha")
    D.write_mha(src, img)
    r = subprocess.run([tool, "-i", src, "-o", dst] + [str(f) for f in flags], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out, kv = D.read_mha(dst)
    return out, kv, r.stderr


@pytest.mark.parametrize("kind", ["q8", "u8", "u16"])
@pytest.mark.parametrize("shape", [(9, 17, 65), (17, 65)], ids=["3D", "2D"])
def test_blur_image_keeps_the_pixel_type_and_equals_the_definition(tool, tmp_path, kind, shape):
    img = D.inputs(shape, kind, seed=3)
    out, kv, err = _run(tool, img, tmp_path, "-s", 1, "-k", 3)
    assert out.dtype == img.dtype and kv["ElementType"] == D.ELEMENT[img.dtype] and kv["CompressedData"] == "False" and int(kv["NDims"]) == img.ndim
    assert out.tobytes() == hmt.blur_image_host(img, 1.0, 3).tobytes()
    assert "Warning" not in err
    for d in range(img.ndim):                                       # slice-wise, compressed
        out, kv, err = _run(tool, img, tmp_path, "-s", 1.5, "-k", 8, "-d", d, "-z", 1)
        assert kv["CompressedData"] == "True" and out.dtype == img.dtype
        assert out.tobytes() == hmt.blur_image_host(img, 1.5, 8, dim=d).tobytes(), d
    out, kv, err = _run(tool, img, tmp_path, "-s", 1, "-k", 3, "-d", -1)          # the reference's default, spelled out
    assert out.tobytes() == hmt.blur_image_host(img, 1.0, 3).tobytes()


def test_a_cut_kernel_warns_with_the_covered_mass(tool, tmp_path):
    img = D.inputs((5, 9, 11), "q8")
    out, kv, err = _run(tool, img, tmp_path, "-s", 3, "-k", 5)
    assert "Warning" in err and "kernelWidth = 5" in err and "0.9339" in err
    assert out.tobytes() == hmt.blur_image_host(img, 3.0, 5).tobytes()


def test_other_pixel_types_end_as_the_reference(tool, tmp_path):
    src = str(tmp_path / "in.mha")
    D.write_mha(src, np.arange(24, dtype=np.int32).reshape(2, 3, 4))
    r = subprocess.run([tool, "-i", src, "-s", "1", "-k", "3", "-o", str(tmp_path / "o.mha")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Error: unsupported image pixel type..." in r.stderr
    assert not os.path.exists(str(tmp_path / "o.mha"))


def test_a_missing_required_option_prints_the_usage(tool, tmp_path):
    src = str(tmp_path / "in.mha")
    D.write_mha(src, D.inputs((3, 4), "q8"))
    for args in (["-i", src, "-k", "3", "-o", "o.mha"], ["-i", src, "-s", "1", "-o", "o.mha"], ["-s", "1", "-k", "3", "-o", "o.mha"], ["-i", src, "-s", "1", "-k", "3"]):
        r = subprocess.run([tool] + args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 1 and "Usage: blur_image" in r.stderr and "required but missing" in r.stderr
