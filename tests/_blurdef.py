"""The second author of blur_image: NumPy (and math.exp for the one exp), written from the definition of DESIGN.md 3.18 /
include/glia_hmt.h, not from the C++.  Arrays are in numpy axis order (z, y, x); `axis` and `skip_axis` below are the
reference's (0 = x = the last array axis), as in the C ABI."""
import math

import numpy as np

MAX_ERROR = 0.01

# the known answers of the issue: (t, max_width) -> radius, and the covered mass where it is stated
RADII = {(1, 3): 3, (1, 32): 3, (4, 32): 5, (0.25, 32): 2, (0.01, 32): 1, (9, 5): 5, (64, 32): 21, (100, 64): 26}
COVERED = {(1, 32): 0.99777, (9, 5): 0.9339}


def discrete_gaussian(n, t):
    """T(n) = exp(-t) I_n(t), the power series in Python floats (IEEE doubles), operation for operation"""
    h = t / 2
    term = 1.0
    for j in range(1, n + 1):
        term = term * h / j
    hh = h * h
    s = 0.0
    k = 0
    while True:
        s += term
        k += 1
        term = term * hh / (k * (k + n))
        if term < s * 2.0 ** -60:
            break
    return math.exp(-t) * s


def kernel(t, max_width, max_error=MAX_ERROR):
    """-> (one-sided coefficients c[0..r] float64, r, covered mass)"""
    c = [discrete_gaussian(0, t), discrete_gaussian(1, t)]
    total = c[0] + 2.0 * c[1]
    i = 2
    while total < 1.0 - max_error:
        ti = discrete_gaussian(i, t)
        c.append(ti)
        total += 2.0 * ti
        if ti <= 0.0 or len(c) > max_width:
            break
        i += 1
    return np.array([v / total for v in c], np.float64), len(c) - 1, total


def axis_pass(vol, axis, c):
    """one pass over a float32 array along the reference's axis: float64 accumulation from +0.0, taps in ascending offset, indices
    clipped into the array, one rounding to float32"""
    ax = vol.ndim - 1 - axis
    r = len(c) - 1
    idx = np.arange(vol.shape[ax])
    acc = np.zeros(vol.shape, np.float64)
    for o in range(-r, r + 1):
        acc = acc + c[abs(o)] * np.take(vol, np.clip(idx + o, 0, vol.shape[ax] - 1), axis=ax).astype(np.float64)
    return acc.astype(np.float32)


def to_pixels(v, dtype):
    """the cast after the last pass: clamp to the type's range, truncate toward zero"""
    if dtype == np.float32:
        return v
    top = float(np.iinfo(dtype).max)
    return np.trunc(np.clip(v.astype(np.float64), 0.0, top)).astype(dtype)


def blur(image, sigma, max_width, skip_axis=-1):
    """sigma: a scalar or one value per axis in the reference's order (x, y[, z])"""
    image = np.asarray(image)
    dim = image.ndim
    sig = [float(sigma)] * dim if np.isscalar(sigma) else [float(s) for s in sigma]
    axes = [a for a in range(dim) if a != skip_axis]
    if not axes:
        return image.copy()
    v = image.astype(np.float32)
    for a in axes:
        v = axis_pass(v, a, kernel(sig[a] * sig[a], max_width)[0])
    return to_pixels(v, image.dtype)


def inputs(shape, kind, seed=0):
    """test volumes: "q8" = Q8 values plus sub-quantum float32 noise; "u8" = a ramp over all three axes modulo 256; "u16" = random
    values with voxels at 0 and 65535"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if kind == "q8":
        v = rng.integers(0, 256, n).astype(np.float32) / np.float32(256) + (rng.random(n, np.float32) - np.float32(0.5)) * np.float32(2.0 ** -10)
        return v.reshape(shape).astype(np.float32)
    if kind == "u8":
        g = np.indices(shape).astype(np.int64)
        return ((sum(g[i] * (3 + 4 * i) for i in range(len(shape)))) % 256).astype(np.uint8)
    assert kind == "u16"
    v = rng.integers(0, 65536, n).astype(np.uint16)
    v[0] = 65535
    v[-1] = 0
    if n > 4:
        v[n // 2] = 65535
        v[n // 3] = 0
    return v.reshape(shape)


# ---- MetaImage files as the tools read and write them --------------------------------------------------------------------------
ELEMENT = {np.dtype(np.float32): "MET_FLOAT", np.dtype(np.uint8): "MET_UCHAR", np.dtype(np.uint16): "MET_USHORT", np.dtype(np.int32): "MET_INT"}


def write_mha(path, arr):
    arr = np.ascontiguousarray(arr)
    hdr = "ObjectType = Image\nNDims = %d\nBinaryData = True\nBinaryDataByteOrderMSB = False\nCompressedData = False\n" % arr.ndim
    hdr += "DimSize = %s\nElementType = %s\nElementDataFile = LOCAL\n" % (" ".join(str(d) for d in arr.shape[::-1]), ELEMENT[arr.dtype])
    with open(path, "wb") as f:
        f.write(hdr.encode() + arr.tobytes())


def read_mha(path):
    """-> (array in numpy axis order, header dict) of a single-file MetaImage"""
    import zlib
    raw = open(path, "rb").read()
    marker = b"ElementDataFile = LOCAL\n"
    at = raw.index(marker) + len(marker)
    kv = dict(line.split(" = ", 1) for line in raw[:at].decode().strip().split("\n"))
    data = raw[at:]
    if kv["CompressedData"] == "True":
        assert len(data) == int(kv["CompressedDataSize"])
        data = zlib.decompress(data)
    dtype = {v: k for k, v in ELEMENT.items()}[kv["ElementType"]]
    shape = tuple(int(d) for d in kv["DimSize"].split())[::-1]
    assert len(shape) == int(kv["NDims"])
    return np.frombuffer(data, dtype).reshape(shape), kv
