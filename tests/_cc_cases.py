"""Face-connected component labelling: the CPU reference and the shared cases of test_cc_reference.py, test_gpu_components.py
and test_gpu_components_cli.py.

The reference states the definition (include/glia_hmt.h, glia_hmt_label_components) in plain Python: one breadth-first flood per
component, started in raster order -- a different algorithm from the device's union-find.  Definition, with the reference's lines:
  * a voxel takes part if it is not masked out (MASK_OUT_VAL = 0; util/image.hxx:349) and, identity / binary mode, its label is not
    BG_VAL = 0 (image.hxx:350; itk::ConnectedComponentImageFilter's background, image.hxx:309), or, inverted mode, its label is 0
    (gadget/main_labelcc_image.cxx:10-18);
  * two face neighbours (type/neighbor.hxx:72-89: -x, +x, -y, +y, [-z, +z], inside the region and not masked out, :80-86) are joined
    if both take part and, identity mode, carry the same label (image.hxx:359);
  * components get 1, 2, ... in raster order of their first voxel (image.hxx:344-367: the scan is the image iterator, x fastest);
    every other voxel gets 0 (image.hxx:340).
Arrays are in numpy axis order (z, y, x) / (y, x).  T / T2: edge of the device's 3D / 2D tile (components.hip)."""
import collections
import functools
import zlib

import numpy as np

T, T2 = 16, 64
MODES = ("identity", "binary", "binary_inverted")


def cc_reference(labels, mask=None, mode="identity"):
    """-> (uint32 volume of component numbers, n)"""
    lab = np.ascontiguousarray(labels, dtype=np.uint32)
    part = (lab == 0) if mode == "binary_inverted" else (lab != 0)
    if mask is not None:
        part = part & (np.asarray(mask) != 0)
    # what must be equal for two voxels that take part to be joined: the label (identity) or nothing (binary); -1: takes no part
    same = np.where(part, lab.astype(np.int64) if mode == "identity" else 0, -1)
    # a border of voxels that take no part stands for "outside the region"
    pad = np.full(tuple(s + 2 for s in lab.shape), -1, np.int64)
    pad[tuple(slice(1, -1) for _ in lab.shape)] = same
    steps = []
    for ax in range(lab.ndim - 1, -1, -1):                 # x first (the last numpy axis), then y, then z
        st = int(np.prod(pad.shape[ax + 1:], dtype=np.int64))
        steps += [-st, st]
    key = pad.ravel().tolist()
    out = [0] * len(key)
    n = 0
    for start in np.flatnonzero(pad.ravel() >= 0).tolist():      # raster order
        if out[start]:
            continue
        n += 1
        k = key[start]
        out[start] = n
        queue = collections.deque([start])
        while queue:
            i = queue.popleft()
            for st in steps:
                j = i + st
                if key[j] == k and not out[j]:
                    out[j] = n
                    queue.append(j)
    res = np.array(out, np.uint32).reshape(pad.shape)[tuple(slice(1, -1) for _ in lab.shape)]
    return np.ascontiguousarray(res), n


# ---- the hand literals (ISSUE: identity / binary / inverted of one 4 x 4 image) --------------------------------------------------
HAND_IN = np.array([[1, 1, 0, 2], [0, 1, 0, 2], [3, 0, 2, 2], [3, 3, 0, 1]], np.uint32)
HAND_OUT = {
    "identity": (np.array([[1, 1, 0, 2], [0, 1, 0, 2], [3, 0, 2, 2], [3, 3, 0, 4]], np.uint32), 4),
    "binary": (np.array([[1, 1, 0, 2], [0, 1, 0, 2], [3, 0, 2, 2], [3, 3, 0, 2]], np.uint32), 3),
    "binary_inverted": (np.array([[0, 0, 1, 0], [2, 0, 1, 0], [0, 3, 0, 0], [0, 0, 4, 0]], np.uint32), 4),
}

Case = collections.namedtuple("Case", "name labels mask mode")


def _u(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _grid_sum(shape):
    return sum(np.indices(shape))


def _u_turn(axis):
    """two arms in the first tile along `axis` (0 = x), the bend in the next one: (z, y, x) volume"""
    a = np.zeros((4, 8, T + 4), np.uint32)                # arms along the last axis
    a[1, 2, T - 4:T + 2] = 6
    a[1, 5, T - 4:T + 2] = 6
    a[1, 2:6, T + 1] = 6
    a[2, 3, T - 2] = 6                                    # a third piece of the same label that stays alone
    return _u(np.moveaxis(a, 2, 2 - axis))


def _serpentine(n=130):
    a = np.zeros((n, n), np.uint32)
    a[0::2, :] = 9
    a[1::4, n - 1] = 9
    a[3::4, 0] = 9
    return a


def _staircase(n=40):
    a = np.zeros((n, n, n), np.uint32)
    for i in range(n):
        a[i, i, i] = 4
        if i + 1 < n:
            a[i, i, i + 1] = 4
            a[i, i + 1, i + 1] = 4
    return a


@functools.lru_cache(maxsize=None)
def _synth5():
    from oracle import pyoracle as O
    return _u(O.synth((48, 64, 64), 8, 16)[0] % 5 + 1)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20)
    out = []

    def add(name, labels, mask=None, mode="identity"):
        out.append(Case(name, _u(labels), None if mask is None else _u(mask), mode))

    for m in MODES:
        add("hand_" + m, HAND_IN, mode=m)
    # degenerate
    add("one_voxel_background", np.zeros((1, 1, 1)))
    add("one_voxel_label7", np.full((1, 1, 1), 7))
    add("one_pixel_label7", np.full((1, 1), 7))
    runs = np.array([(i // 3) % 3 for i in range(37)])    # runs of three: 0 0 0 1 1 1 2 2 2 0 ...
    add("line_along_z", runs.reshape(37, 1, 1))
    add("line_along_x", runs.reshape(1, 1, 37))
    add("line_along_x_binary", runs.reshape(1, 1, 37), mode="binary")
    add("all_background", np.zeros((20, 17, 18)))
    add("all_background_inverted", np.zeros((20, 17, 18)), mode="binary_inverted")
    add("one_label_ragged_box", np.full((40, 36, 35), 3))
    big = np.zeros((5, 18, 20), np.uint32)
    big[:, :9] = 0xFFFFFFFE
    big[:, 9:, :10] = 0xFFFFFFFF
    add("label_fffffffe", big)
    corners = np.ones((18, 17, 19), np.uint32)
    corners[0, 0, 0] = corners[-1, -1, -1] = 0
    add("background_first_and_last", corners)
    add("background_first_and_last_inverted", corners, mode="binary_inverted")
    # most components
    add("checker3d_two_labels", 1 + _grid_sum((17, 18, 19)) % 2)
    add("checker3d_one_label", _grid_sum((17, 18, 19)) % 2)
    add("checker2d_two_labels", 1 + _grid_sum((67, 70)) % 2)
    add("checker2d_one_label", _grid_sum((67, 70)) % 2)
    add("checker2d_one_label_binary", _grid_sum((67, 70)) % 2, mode="binary")
    # numbering is by raster order, not tile order
    a = np.zeros((8, 2 * T2 + 12), np.uint32)
    a[0, T2 + 3:T2 + 6] = 5                               # A: first voxel (x = T2 + 3, y = 0), in the second tile
    a[1, 0:3] = 5                                         # B: first voxel (0, 1), in the first tile
    add("raster_not_tile_order_2d", a)
    a = np.zeros((T + 4, 4, T + 8), np.uint32)
    a[:, 0, T + 3] = 5                                    # A: (x = T + 3, y = 0, z = 0) down through the z tile border
    a[0, 1, 0:3] = 5                                      # B: (0, 1, 0)
    a[T + 1:, 3, 0:2] = 5                                 # C: (0, 3, T + 1), below the border, in the first x tile
    add("raster_not_tile_order_3d", a)
    # joined only through another tile
    for ax, nm in enumerate("xyz"):
        add("u_turn_3d_" + nm, _u_turn(ax))
    a = np.zeros((10, T2 + 6), np.uint32)
    a[2, T2 - 4:T2 + 2] = 6
    a[5, T2 - 4:T2 + 2] = 6
    a[2:6, T2 + 1] = 6
    add("u_turn_2d_x", a)
    add("u_turn_2d_y", a.T)
    a = np.zeros((T2 + 6, T2 + 6), np.uint32)
    a[T2 - 2:T2 + 2, T2 - 2:T2 + 2] = 8
    a[T2 - 1:T2 + 1, T2 - 1:T2 + 1] = 0
    add("ring_around_tile_corner_2d", a)
    a = np.zeros((T + 4, T + 4, T + 4), np.uint32)
    a[T - 2:T + 2, T - 2:T + 2, T - 2:T + 2] = 8          # a shell around the corner of eight tiles ...
    a[T - 1:T + 1, T - 1:T + 1, T - 1:T + 1] = 2          # ... and another label inside it
    add("shell_around_tile_corner_3d", a)
    # long chains
    add("serpentine", _serpentine())
    add("serpentine_reversed", _serpentine()[::-1, ::-1])
    add("serpentine_binary", _serpentine(), mode="binary")
    add("serpentine_inverted", _serpentine(), mode="binary_inverted")
    add("staircase", _staircase())
    add("staircase_reversed", _staircase()[::-1, ::-1, ::-1])
    # same label, several pieces
    add("synth_mod5", _synth5())
    add("synth_mod5_binary", _synth5(), mode="binary")
    add("synth_mod5_cropped", _synth5()[:33, :29, :31])
    # mask
    a = np.full((6, 20, 20), 4, np.uint32)
    m = np.ones(a.shape, np.uint32)
    m[:, :, 10] = 0
    add("mask_plane_cuts_label", a, m)
    a = np.zeros((3, 5), np.uint32)
    a[1] = 3
    m = np.full(a.shape, 7, np.uint32)
    m[1, 2] = 0
    add("mask_removes_bridge", a, m)
    a = np.array([[2, 0, 5, 5], [2, 2, 2, 0]], np.uint32)
    m = np.ones(a.shape, np.uint32)
    m[0, 0] = 0
    add("mask_removes_first_voxel", a, m)
    add("mask_removes_first_voxel_unmasked", a)
    add("mask_all_out", np.full((9, 20, 18), 2), np.zeros((9, 20, 18)))
    a = rng.integers(0, 4, size=(18, 20, 21))
    m = (rng.random(a.shape) > 0.25) * 3
    for md in MODES:
        add("mask_random_" + md, a, m, md)
    a2 = rng.integers(0, 3, size=(T2 + 5, T2 + 9))
    add("mask_random_2d", a2, rng.random(a2.shape) > 0.2)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(components, n) of a case by the reference: computed once per process, shared, never modified"""
    c = case(name)
    ref, n = cc_reference(c.labels, c.mask, c.mode)
    ref.setflags(write=False)
    return ref, n


def _count(name):
    return int(np.count_nonzero(case(name).labels))


# closed-form component counts (test_cc_reference.py holds the reference to them; the GPU tests hold the device to the reference)
KNOWN_N = {
    "hand_identity": 4, "hand_binary": 3, "hand_binary_inverted": 4,
    "one_voxel_background": 0, "one_voxel_label7": 1, "one_pixel_label7": 1,
    "line_along_z": 8, "line_along_x": 8, "line_along_x_binary": 4,          # 37 voxels: runs 0 1 2 | 0 1 2 | 0 1 2 | 0 1 2 | 0
    "all_background": 0, "all_background_inverted": 1, "one_label_ragged_box": 1, "label_fffffffe": 2,
    "background_first_and_last": 1, "background_first_and_last_inverted": 2,
    "checker3d_two_labels": 17 * 18 * 19, "checker3d_one_label": lambda: _count("checker3d_one_label"),
    "checker2d_two_labels": 67 * 70, "checker2d_one_label": lambda: _count("checker2d_one_label"),
    "checker2d_one_label_binary": lambda: _count("checker2d_one_label"),
    "raster_not_tile_order_2d": 2, "raster_not_tile_order_3d": 3,
    "u_turn_3d_x": 2, "u_turn_3d_y": 2, "u_turn_3d_z": 2, "u_turn_2d_x": 1, "u_turn_2d_y": 1,
    "ring_around_tile_corner_2d": 1, "shell_around_tile_corner_3d": 2,
    "serpentine": 1, "serpentine_reversed": 1, "serpentine_binary": 1, "serpentine_inverted": 65, "staircase": 1, "staircase_reversed": 1,
    "synth_mod5_binary": 1,
    "mask_plane_cuts_label": 2, "mask_removes_bridge": 2, "mask_removes_first_voxel": 2, "mask_removes_first_voxel_unmasked": 2,
    "mask_all_out": 0,
}


def known_n(name):
    v = KNOWN_N[name]
    return v() if callable(v) else v


# ---- MetaImage files for the tool tests ------------------------------------------------------------------------------------------
_ELEMENT = {np.dtype(np.uint32): "MET_UINT", np.dtype(np.uint16): "MET_USHORT", np.dtype(np.uint8): "MET_UCHAR"}


def write_mha(path, arr, compress=False):
    arr = np.ascontiguousarray(arr)
    data = arr.tobytes()
    if compress:
        data = zlib.compress(data, 6)
    hdr = "ObjectType = Image\nNDims = %d\nBinaryData = True\nBinaryDataByteOrderMSB = False\nCompressedData = %s\n" % (arr.ndim, compress)
    if compress:
        hdr += "CompressedDataSize = %d\n" % len(data)
    hdr += "DimSize = %s\nElementType = %s\nElementDataFile = LOCAL\n" % (" ".join(str(d) for d in arr.shape[::-1]), _ELEMENT[arr.dtype])
    with open(path, "wb") as f:
        f.write(hdr.encode() + data)


def read_mha(path):
    """-> (array in numpy axis order, header dict) of a single-file MetaImage as the tools write it"""
    raw = open(path, "rb").read()
    marker = b"ElementDataFile = LOCAL\n"
    at = raw.index(marker) + len(marker)
    kv = dict(line.split(" = ", 1) for line in raw[:at].decode().strip().split("\n"))
    data = raw[at:]
    if kv["CompressedData"] == "True":
        assert len(data) == int(kv["CompressedDataSize"])
        data = zlib.decompress(data)
    dtype = {v: k for k, v in _ELEMENT.items()}[kv["ElementType"]]
    shape = tuple(int(d) for d in kv["DimSize"].split())[::-1]
    assert len(shape) == int(kv["NDims"])
    return np.frombuffer(data, dtype).reshape(shape), kv
