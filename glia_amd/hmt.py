"""Host-side mirror of GLIA's HMT operators over the C ABI (include/glia_hmt.h).

Names follow the reference: RegionMap ~ TRegionMap(image, mask, onlyContour) (type/region_map.hxx:38-40),
merge_order_pb ~ hmt/main_merge_order_pb.cxx.  Volumes are torch CUDA tensors (device memory plumbing
only) in numpy axis order (z, y, x).  No CPU path exists here.

The prototypes live in one table (glia_amd/_abi.py) that lib() installs; the Structure classes and dtypes below re-state structs of
the header.  tests/test_binding_host.py holds both to the header.
"""
import ctypes as C
import os

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("GLIA_HMT_LIB", os.path.join(_HERE, "libglia_hmt.so"))   # override: kernel experiments only

MAX_IMAGES, MAX_BINS, MAX_THRESH = 8, 16, 4
PREDICT_STAGE_MAX_DIM = 767      # GLIA_HMT_PREDICT_STAGE_MAX_DIM: longer rows are walked from global memory (pinned to the library by the GPU tests)


def predict_tile_rows(n_rows, dim):
    """glia_hmt_forest_predict_tile_rows: rows of the LDS tile RandomForest.predict uses for this input (64, 32, 16, 8), 0 = not staged"""
    return _count(lib().glia_hmt_forest_predict_tile_rows(n_rows, dim))


class HmtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("glia_hmt error %d: %s" % (code, msg))
        self.code = code


class Image(C.Structure):
    _fields_ = [("d_image", C.c_void_p), ("bins", C.c_int), ("lo", C.c_double), ("hi", C.c_double)]


class FeatConfig(C.Structure):
    _fields_ = [
        ("n_region", C.c_int), ("region", Image * MAX_IMAGES),
        ("n_rlabel", C.c_int), ("rlabel", Image * MAX_IMAGES),
        ("n_boundary", C.c_int), ("boundary", Image * MAX_IMAGES),
        ("d_pb", C.c_void_p), ("n_thresholds", C.c_int), ("thresholds", C.c_double * MAX_THRESH),
        ("normalizing_area", C.c_double), ("normalizing_length", C.c_double),
        ("use_log_shape", C.c_int), ("use_simple_features", C.c_int),
        ("use_histogram_features", C.c_int), ("use_median_features", C.c_int),
    ]


_lib = None


def lib():
    """Loads libglia_hmt.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise ImportError("glia_amd/libglia_hmt.so is missing: run `python -c 'import __graft_entry__ as g; "
                              "g.build()'` (hipcc --offload-arch=gfx950); there is no CPU fallback")
        # torch wheels bundle their own HIP runtime: when torch is used in the process (tests, bench.py) it has to
        # be loaded first so that both sides share ONE runtime; a plain C host simply gets /opt/rocm's.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(_SO)
        for name, (result, params) in _abi.PROTOTYPES.items():     # the only place that gives a function its prototype
            f = getattr(L, name)
            f.restype = result
            f.argtypes = params
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise HmtError(rc, lib().glia_hmt_last_error().decode())


def _count(n):
    """the result of a call that returns a count, or a negative status"""
    if n < 0:
        raise HmtError(int(n), lib().glia_hmt_last_error().decode())
    return n


def _outs(fn, types, *args):
    """fn(*args, one out-parameter per type by reference), checked -> the values it wrote"""
    v = [t() for t in types]
    _check(fn(*args, *[C.byref(x) for x in v]))
    return [x.value for x in v]


def _struct_out(fn, cls, handle):
    """fn(handle, &struct), checked -> dict of the struct's fields, a nested struct as a dict: the last_*_timing getters"""
    def fields(s):
        return {k: fields(v) if isinstance(v, C.Structure) else v for k, v in ((k, getattr(s, k)) for k, *_ in s._fields_)}
    s = cls()
    _check(fn(handle, C.byref(s)))
    return fields(s)


def _new(fn, *args):
    """the handle that fn(*args, &handle) creates, checked"""
    h = C.c_void_p()
    _check(fn(*args, C.byref(h)))
    return h


class _Handle:
    """Owner of one native handle: h, freed once by the library function the class names; close() may be called again."""
    _free = None

    @classmethod
    def _wrap(cls, h, **attrs):
        """an instance around an existing handle, the constructor not run"""
        self = cls.__new__(cls)
        self.h = h
        vars(self).update(attrs)
        return self

    def close(self):
        if self.h:
            getattr(lib(), self._free)(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


ERR_ARG, ERR_CAPACITY, ERR_INTERNAL = -1, -4, -7

OVERLAP_ENTRY = np.dtype([("a", np.uint32), ("b", np.uint32), ("count", np.uint64)])      # glia_hmt_overlap_entry
VI_MODES = {"reference": 0, "exact": 1}                                                   # GLIA_HMT_VI_REFERENCE | GLIA_HMT_VI_EXACT


class EvalResult(C.Structure):
    """glia_hmt_eval_result"""
    _fields_ = [(k + s, C.c_uint64) for k in ("tp", "tn", "fp", "fn") for s in ("_lo", "_hi")] + \
               [(k, C.c_double) for k in ("precision", "recall", "f1", "rand_index", "false_split", "false_merge")]

    def as_dict(self):
        out = {k.upper(): (getattr(self, k + "_hi") << 64) | getattr(self, k + "_lo") for k in ("tp", "tn", "fp", "fn")}
        out.update({k: getattr(self, k) for k in ("precision", "recall", "f1", "rand_index", "false_split", "false_merge")})
        return out


class EvalTiming(C.Structure):
    """glia_hmt_eval_timing"""
    _fields_ = [("ms_count", C.c_double), ("entries", C.c_int64), ("repeats", C.c_int64)]


def overlap_scores(tables, vi_mode="reference"):
    """glia_hmt_overlap_scores (host-only, needs no GPU): the numbers of eval_ri / eval_vi from the contingency tables of one or
    more image pairs -- structured arrays as Context.label_overlap returns them (or anything np.asarray turns into one), taken
    as given.  -> dict: TP, TN, FP, FN (Python ints, summed over the tables before any ratio), precision, recall, f1 (NaN at
    0 / 0, as the reference), rand_index, false_split = H(a | b), false_merge = H(b | a) (means over the tables).
    vi_mode "reference": log2 of the INTEGER quotient floor(marginal / count), what the reference tool prints
    (util/image_stats.hxx:153 divides two uints); "exact": the real quotient."""
    if isinstance(tables, np.ndarray) and tables.dtype == OVERLAP_ENTRY:
        tables = [tables]
    keep = [np.ascontiguousarray(t, dtype=OVERLAP_ENTRY).reshape(-1) for t in tables]
    n = len(keep)
    ptrs = (C.c_void_p * max(n, 1))(*[t.ctypes.data if len(t) else None for t in keep])
    lens = (C.c_int64 * max(n, 1))(*[len(t) for t in keep])
    out = EvalResult()
    _check(lib().glia_hmt_overlap_scores(ptrs, lens, n, VI_MODES[vi_mode], C.byref(out)))
    return out.as_dict()


PIXEL_TYPES = {"float32": 0, "uint8": 1, "uint16": 2}     # GLIA_HMT_PIXEL_*
BLUR_ROUTES = {0: "passes", 1: "march"}                   # GLIA_HMT_BLUR_ROUTE_*
BLUR_MAX_ERROR = 0.01                                     # GLIA_HMT_BLUR_MAX_ERROR


def gaussian_kernel(variance, max_width, max_error=BLUR_MAX_ERROR):
    """glia_hmt_gaussian_kernel (host-only, needs no GPU): the discrete Gaussian of one axis as blur_image truncates it ->
    (one-sided coefficients c[0..radius] as float64, radius, covered mass before the division)."""
    c = np.empty(129, np.float64)
    r, cov = _outs(lib().glia_hmt_gaussian_kernel, (C.c_int, C.c_double), variance, max_width, max_error, _np(c), len(c))
    return c[:r + 1].copy(), r, cov


def blur_limits():
    """glia_hmt_blur_limits -> dict: tile_x, tile_y (the march route's tile), max_march_radius, max_radius"""
    return dict(zip(("tile_x", "tile_y", "max_march_radius", "max_radius"), _outs(lib().glia_hmt_blur_limits, (C.c_int,) * 4)))


def _blur_variances(sigma, dim):
    """sigma: a scalar, or one value per axis in the reference's order (x, y[, z]) -- the reverse of the array's shape"""
    s = [float(sigma)] * dim if np.isscalar(sigma) else [float(v) for v in sigma]
    if len(s) != dim:
        raise ValueError("sigma: a scalar or one value per axis")
    return (C.c_double * 3)(*([v * v for v in s] + [1.0] * (3 - dim)))


def blur_image_host(image, sigma, kernel_width, dim=-1):
    """glia_hmt_blur_image_host (needs no GPU): the definition of blur_image on a float32 / uint8 / uint16 ndarray in numpy axis
    order (z, y, x) -> ndarray of the same type.  sigma and dim as Context.blur_image."""
    a = np.ascontiguousarray(image)
    ndim, d = _dims(a.shape)
    out = np.empty_like(a)
    _check(lib().glia_hmt_blur_image_host(ndim, d, PIXEL_TYPES[a.dtype.name], _np(a), _blur_variances(sigma, ndim), kernel_width,
                                          dim if dim >= 0 else -1, _np(out)))
    return out


def set_option(key, value):
    """glia_hmt_set_option: a process-wide tuning / test switch of the loops (value None unsets it)."""
    _check(lib().glia_hmt_set_option(key.encode(), None if value is None else str(value).encode()))


class options:
    """with options(GLIA_HMT_WINCAP=32, ...): the switches are set inside the block and unset afterwards (no result depends on
    them; the queue tests use them to drive the window queue through its rare paths)."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.kv:
            set_option(k, None)
        return False


def check_merge_order(dense_order, n_regions):
    """glia_hmt_check_merge_order on a DENSE-id order ([n][3] uint32): -1 when every merge joins two regions that still exist and
    creates region n_regions + k, else the first merge that does not."""
    o = np.ascontiguousarray(dense_order, dtype=np.uint32).reshape(-1, 3)
    bad = C.c_int64(-1)
    rc = lib().glia_hmt_check_merge_order(_np(o), len(o), int(n_regions), C.byref(bad))
    if rc not in (0, ERR_ARG):
        _check(rc)
    return int(bad.value)


def _dims(shape):
    dim = len(shape)
    d = (C.c_int64 * 3)(1, 1, 1)
    for i, n in enumerate(shape[::-1]):
        d[i] = n
    return dim, d


def _np(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _ptr(t):
    """device pointer of a tensor that may be absent"""
    return None if t is None else t.data_ptr()


def _fence(t):
    """The library works on its own HIP stream: finish whatever torch has queued on the tensor's device first
    (a clone() or copy_ producing the input), so the kernels below see the data."""
    import torch
    torch.cuda.current_stream(t.device).synchronize()


class Context(_Handle):
    _free = "glia_hmt_ctx_destroy"

    def __init__(self, device=0, stream=None):
        self.h = _new(lib().glia_hmt_ctx_create, device, stream if stream else None)
        self.device = device
        self._overlap_room = 0           # entries of the last label_overlap table: the size of the next call's host buffer
        if lib().glia_hmt_ctx_libm_status(self.h) == 0:
            import warnings
            warnings.warn(lib().glia_hmt_last_error().decode())

    def sync(self):
        _check(lib().glia_hmt_ctx_sync(self.h))

    def libm(self):
        """(log2 variant, log variant) the kernels use: 1 = glibc non-FMA, 2 = glibc FMA, 0 = device libm (unpinned)."""
        return tuple(_outs(lib().glia_hmt_ctx_libm, (C.c_int, C.c_int), self.h))

    @staticmethod
    def release_cached_memory():
        """Scratch blocks the library parks for reuse go back to the driver (glia_hmt_release_cached_memory); returns the bytes released."""
        return int(lib().glia_hmt_release_cached_memory())

    @staticmethod
    def internal_errors():
        """Calls of this process that ended with GLIA_HMT_ERR_INTERNAL -- a merge loop's own consistency stop or an order that
        failed the replay of glia_hmt_check_merge_order (glia_hmt_internal_errors).  0 is the only healthy answer."""
        return int(lib().glia_hmt_internal_errors())

    def libm_pinned(self):
        """True when log2, log and pow of the host libm are all reproduced bit for bit (glia_hmt_ctx_libm_status)."""
        return lib().glia_hmt_ctx_libm_status(self.h) == 1

    def libm_pow(self):
        """variant of std::pow(perim, 1.5) the kernels use (same codes as libm())"""
        return _outs(lib().glia_hmt_ctx_libm_pow, (C.c_int,), self.h)[0]

    def libm_exp(self):
        """variant of std::exp the classifier loop's MLP sigmoid uses (same codes as libm()); not part of libm_pinned()"""
        return _outs(lib().glia_hmt_ctx_libm_exp, (C.c_int,), self.h)[0]

    def libm_eval(self, function, variant, x):
        """Device restatement of the host libm over a CUDA f64 tensor: function 0 = log2, 1 = log, 2 = pow(x, 1.5), 3 = exp,
        4 = the sigmoid 1 / (1 + exp(-x))."""
        import torch
        out = torch.empty_like(x)
        _check(lib().glia_hmt_libm_eval(self.h, function, variant, x.data_ptr(), out.data_ptr(), x.numel()))
        self.sync()
        return out

    def watershed(self, image, level):
        """glia::watershed (util/image_alg.hxx:9-21) of a CUDA float32 tensor -> (labels int32 tensor holding uint32 1..n, n, sweeps)."""
        import torch
        assert image.is_cuda and image.dtype == torch.float32 and image.is_contiguous()
        dim, d = _dims(tuple(image.shape))
        out = torch.empty(image.shape, dtype=torch.int32, device=image.device)
        _fence(image)
        n, sw = _outs(lib().glia_hmt_watershed, (C.c_uint32, C.c_int), self.h, dim, d, image.data_ptr(), level, out.data_ptr())
        return out, n, sw

    CC_MODES = {"identity": 0, "binary": 1, "binary_inverted": 2}

    def label_components(self, labels, mask=None, mode="identity"):
        """Face-connected components of a CUDA label tensor (uint32 payload) -> (out int32 tensor holding uint32 0..n, n), numbered
        in raster order of their first voxel.  mode "identity" = labelIdentityConnectedComponents (util/image.hxx:331-373, equal
        labels join), "binary" = labelConnectedComponents (util/image.hxx:302-313, non-zero voxels join), "binary_inverted" =
        labelcc_image --invert (zero voxels join).  mask: 0 masks a voxel out.  The input is left unchanged."""
        import torch
        assert labels.is_cuda and labels.is_contiguous() and labels.element_size() == 4 and labels.dim() in (2, 3)
        assert mask is None or (mask.is_cuda and mask.is_contiguous() and mask.element_size() == 4 and mask.shape == labels.shape)
        dim, d = _dims(tuple(labels.shape))
        out = torch.empty(labels.shape, dtype=torch.int32, device=labels.device)
        _fence(labels)
        n, = _outs(lib().glia_hmt_label_components, (C.c_uint32,), self.h, dim, d, labels.data_ptr(), _ptr(mask), self.CC_MODES[mode],
                   out.data_ptr())
        return out, n

    def blur_image(self, image, sigma, kernel_width, dim=-1):
        """blurImage (util/image.hxx:376-407, gadget/main_blur_image.cxx) of a CUDA tensor of float32, uint8 or uint16 (an int16
        tensor is taken as uint16 payload) in numpy axis order (z, y, x) -> a new tensor of the same type; the input is left
        unchanged.  sigma: a scalar, or one value per axis in the reference's order (x, y[, z]) -- the reverse of the tensor's
        shape --, in voxels; kernel_width: MaximumKernelWidth.  dim >= 0: the slice-wise mode, axis `dim` (reference order, 0 = x =
        the last tensor axis) is left alone.  The result equals blur_image_host bit for bit on either route (GLIA_HMT_BLUR)."""
        import torch
        names = {torch.float32: "float32", torch.uint8: "uint8", torch.uint16: "uint16", torch.int16: "uint16"}
        assert image.is_cuda and image.is_contiguous() and image.dtype in names and image.dim() in (2, 3)
        ndim, d = _dims(tuple(image.shape))
        out = torch.empty_like(image)
        _fence(image)
        _check(lib().glia_hmt_blur_image(self.h, ndim, d, PIXEL_TYPES[names[image.dtype]], image.data_ptr(), _blur_variances(sigma, ndim),
                                         kernel_width, dim if dim >= 0 else -1, out.data_ptr()))
        return out

    def last_blur_timing(self):
        """glia_hmt_last_blur_timing -> (device ms of the last blur_image call's kernels, the route that ran: "passes" | "march")"""
        ms, route = _outs(lib().glia_hmt_last_blur_timing, (C.c_double, C.c_int), self.h)
        return ms, BLUR_ROUTES[route]

    def label_overlap(self, a, b, mask=None, drop_zero_a=False, drop_zero_b=False):
        """glia_hmt_label_overlap: the contingency table of two CUDA label tensors (uint32 payload, same number of voxels, any
        shape) -> structured array (a, b, count) of the pairs with count > 0, ascending by (a, b).  mask: 0 drops the voxel;
        drop_zero_a / drop_zero_b drop the voxels whose label in a / b is 0.  Tensors that are not 16-byte aligned (a view one
        element into a buffer) take the scalar path to the same result."""
        for t in (a, b) + (() if mask is None else (mask,)):
            assert t.is_cuda and t.is_contiguous() and t.element_size() == 4 and t.numel() == a.numel()
            _fence(t)
        flags = (1 if drop_zero_a else 0) | (2 if drop_zero_b else 0)
        out = np.empty(max(self._overlap_room, 1 << 12), OVERLAP_ENTRY)
        n = C.c_int64(0)
        while True:
            rc = lib().glia_hmt_label_overlap(self.h, a.data_ptr(), b.data_ptr(), _ptr(mask), a.numel(), flags, _np(out), len(out), C.byref(n))
            if rc != ERR_CAPACITY or n.value <= len(out):
                break
            out = np.empty(n.value, OVERLAP_ENTRY)          # the table is larger than the guess: once more with room for it
        _check(rc)
        self._overlap_room = n.value                        # the next call on this context starts with room for a table of this size
        return out[:n.value].copy()

    def evaluate(self, res, ref, masks=None, vi_mode="reference"):
        """eval_ri and eval_vi (gadget/main_eval_ri.cxx, main_eval_vi.cxx) of proposed volumes against reference volumes on the
        device: CUDA label tensors (uint32 payload) or lists of them, pair i with masks[i] (None, one tensor, or a list that
        may hold None).  Masked-out voxels and voxels with reference label 0 are dropped.  -> dict: TP, TN, FP, FN (Python
        ints, summed over the pairs), precision, recall, f1, rand_index, false_split, false_merge (means over the pairs;
        vi_mode as overlap_scores)."""
        if not isinstance(res, (list, tuple)):
            res, ref = [res], [ref]
            masks = None if masks is None else [masks]
        assert len(res) == len(ref) and len(res) >= 1 and (masks is None or len(masks) == len(res))
        for i, (p, r) in enumerate(zip(res, ref)):
            for t in (p, r) + (() if masks is None or masks[i] is None else (masks[i],)):
                assert t.is_cuda and t.is_contiguous() and t.element_size() == 4 and t.numel() == p.numel()
                _fence(t)
        n = len(res)
        ptrs = lambda ts: (C.c_void_p * n)(*[_ptr(t) for t in ts])
        nv = (C.c_int64 * n)(*[p.numel() for p in res])
        out = EvalResult()
        _check(lib().glia_hmt_eval(self.h, n, ptrs(res), ptrs(ref), ptrs(masks) if masks is not None else None, nv, VI_MODES[vi_mode],
                                   C.byref(out)))
        return out.as_dict()

    def last_eval_timing(self):
        """the counting passes of the last label_overlap / evaluate call: ms_count (device), entries, repeats"""
        return _struct_out(lib().glia_hmt_last_eval_timing, EvalTiming, self.h)

    def set_table_hint(self, regions, pairs):
        _check(lib().glia_hmt_ctx_set_table_hint(self.h, regions, pairs))

    def synth(self, shape, S, G, seed=0x9E3779B97F4A7C15, variant=0):
        """Synthetic supervoxels + pb on the device; returns torch tensors (labels i32 view, pb)."""
        import torch
        dim, d = _dims(shape)
        dev = torch.device("cuda", self.device)
        labels = torch.empty(shape, dtype=torch.int32, device=dev)   # uint32 payload
        pb = torch.empty(shape, dtype=torch.float32, device=dev)
        _check(lib().glia_hmt_synth(self.h, dim, d, S, G, seed, variant, labels.data_ptr(), pb.data_ptr()))
        return labels, pb


def make_config(pb, rb=(), r=(), rl=(), b=(), thresholds=(0.2, 0.5, 0.8), normalizing_area=1.0,
                normalizing_length=1.0, use_log_shape=False, use_simple_features=False, use_histogram_features=False,
                use_median_features=False):
    """Builds the image lists the way prepareImages does (hmt/hmt_util.hxx:17-56).
    rb/r/rl/b: sequences of (device tensor, bins, lo, hi).  use_median_features (GLIA_USE_MEDIAN_AS_FEATS): supported by bc_feat
    and score_initial_edges / score_initial_edges_shard, refused by merge_order_bc."""
    cfg = FeatConfig()
    keep = [pb]

    def fill(arr, lst):
        for i, (img, bins, lo, hi) in enumerate(lst):
            keep.append(img)
            arr[i].d_image = img.data_ptr()
            arr[i].bins, arr[i].lo, arr[i].hi = bins, lo, hi
        return len(lst)

    cfg.n_region = fill(cfg.region, list(rb) + list(r))
    cfg.n_rlabel = fill(cfg.rlabel, list(rl))
    cfg.n_boundary = fill(cfg.boundary, list(rb) + list(b))
    cfg.d_pb = pb.data_ptr()
    cfg.n_thresholds = len(thresholds)
    for i, t in enumerate(thresholds):
        cfg.thresholds[i] = t
    cfg.normalizing_area, cfg.normalizing_length = normalizing_area, normalizing_length
    cfg.use_log_shape, cfg.use_simple_features = int(use_log_shape), int(use_simple_features)
    cfg.use_histogram_features, cfg.use_median_features = int(use_histogram_features), int(use_median_features)
    cfg._keep = keep
    return cfg


def gen_tree(order):
    """hmt::genTree (hmt/tree_build.hxx:12-38) -> (label, parent, child0, child1) arrays."""
    order = np.ascontiguousarray(order, dtype=np.uint32)
    cap = 3 * len(order) + 1      # a forest of several components has more than 2n+1 nodes
    lab = np.empty(cap, np.uint32)
    par = np.empty(cap, np.int32); c0 = np.empty(cap, np.int32); c1 = np.empty(cap, np.int32)
    n = _count(lib().glia_hmt_gen_tree(_np(order), len(order), _np(lab), _np(par), _np(c0), _np(c1), cap))
    return lab[:n], par[:n], c0[:n], c1[:n]


def transform_keys(order):
    """transformKeys (util/struct_merge.hxx:188-210): merge order -> (src, dst) label map, sorted by src."""
    order = np.ascontiguousarray(order, dtype=np.uint32)
    cap = 2 * len(order) + 1
    src = np.empty(cap, np.uint32); dst = np.empty(cap, np.uint32)
    n = _count(lib().glia_hmt_transform_keys(_np(order), len(order), _np(src), _np(dst), cap))
    return src[:n].copy(), dst[:n].copy()


def transform_image(ctx, labels, src, dst, mask=None, fill_missing=False):
    """transformImage (util/image.hxx:227-242): rewrites the CUDA label tensor in place."""
    src = np.ascontiguousarray(src, dtype=np.uint32); dst = np.ascontiguousarray(dst, dtype=np.uint32)
    assert labels.is_cuda and labels.is_contiguous() and labels.element_size() == 4
    _fence(labels)
    _check(lib().glia_hmt_transform_image(ctx.h, labels.data_ptr(), labels.numel(), _np(src), _np(dst), len(src), _ptr(mask),
                                          1 if fill_missing else 0))
    return lib().glia_hmt_last_transform_ms(ctx.h)


def relabel_image(ctx, labels, min_size=0):
    """relabelImage (util/image.hxx:992-1001): consecutive labels by decreasing size, in place; returns #labels."""
    assert labels.is_cuda and labels.is_contiguous() and labels.element_size() == 4
    _fence(labels)
    return _outs(lib().glia_hmt_relabel_image, (C.c_uint32,), ctx.h, labels.data_ptr(), labels.numel(), min_size)[0]


def tree_potentials(order, merge_probs=None, region_probs=None):
    """genTree / genTreeWithNodePotentials (hmt/tree_build.hxx:12-63) -> (label, parent, child0, child1, potential)."""
    order = np.ascontiguousarray(order, dtype=np.uint32)
    cap = 3 * len(order) + 1
    lab = np.empty(cap, np.uint32); par = np.empty(cap, np.int32); c0 = np.empty(cap, np.int32); c1 = np.empty(cap, np.int32)
    pot = np.empty(cap, np.float64)
    mp = None if merge_probs is None else np.ascontiguousarray(merge_probs, dtype=np.float64)
    rp = None if region_probs is None else np.ascontiguousarray(region_probs, dtype=np.float64)
    n = lib().glia_hmt_tree_potentials(_np(order), len(order), _np(mp), _np(rp), _np(lab), _np(par), _np(c0), _np(c1), _np(pot), cap)
    assert n >= 0
    return lab[:n].copy(), par[:n].copy(), c0[:n].copy(), c1[:n].copy(), pot[:n].copy()


def resolve_tree_greedy(parent, child0, child1, potential):
    """resolveTreeGreedy (hmt/tree_greedy.hxx:104-152, one tree): node indices in pick order."""
    par = np.ascontiguousarray(parent, np.int32); c0 = np.ascontiguousarray(child0, np.int32); c1 = np.ascontiguousarray(child1, np.int32)
    pot = np.ascontiguousarray(potential, np.float64)
    picks = np.empty(max(len(par), 1), np.int32)
    n = lib().glia_hmt_resolve_tree_greedy(_np(par), _np(c0), _np(c1), _np(pot), len(par), _np(picks), len(picks))
    assert n >= 0
    return picks[:n].copy()


def label_transform(node_label, child0, child1, picks, key_to_assign=1):
    """genLabelTransform (hmt/tree_segment.hxx:10-21) -> (src, dst) sorted by src."""
    lab = np.ascontiguousarray(node_label, np.uint32); c0 = np.ascontiguousarray(child0, np.int32); c1 = np.ascontiguousarray(child1, np.int32)
    picks = np.ascontiguousarray(picks, np.int32)
    src = np.empty(max(len(lab), 1), np.uint32); dst = np.empty(max(len(lab), 1), np.uint32)
    n = lib().glia_hmt_label_transform(_np(lab), _np(c0), _np(c1), len(lab), _np(picks), len(picks), key_to_assign, _np(src), _np(dst), len(src))
    assert n >= 0
    o = np.argsort(src[:n], kind="stable")
    return src[:n][o].copy(), dst[:n][o].copy()


def tree_energies(order, merge_probs):
    """The tree of segment_ccm (hmt/main_segment_ccm.cxx:39-53, hmt/tree_ccm.hxx:12-27) -> (label, parent, child0, child1, em, es, Em, Es):
    own energies and energy tuples per node."""
    order = np.ascontiguousarray(order, dtype=np.uint32).reshape(-1, 3)
    mp = np.ascontiguousarray(merge_probs, dtype=np.float64)
    assert len(mp) >= len(order)
    cap = 3 * len(order) + 1
    lab = np.empty(cap, np.uint32); par = np.empty(cap, np.int32); c0 = np.empty(cap, np.int32); c1 = np.empty(cap, np.int32)
    e = [np.empty(cap, np.float64) for _ in range(4)]
    n = _count(lib().glia_hmt_tree_energies(_np(order), len(order), _np(mp), _np(lab), _np(par), _np(c0), _np(c1), _np(e[0]), _np(e[1]), _np(e[2]),
                                            _np(e[3]), cap))
    return tuple(a[:n].copy() for a in [lab, par, c0, c1] + e)


def tree_energy_tuples(child0, child1, em, es):
    """computeEnergyTuples (hmt/tree_ccm.hxx:12-27) for given own energies -> (Em, Es)."""
    c0 = np.ascontiguousarray(child0, np.int32); c1 = np.ascontiguousarray(child1, np.int32)
    em = np.ascontiguousarray(em, np.float64); es = np.ascontiguousarray(es, np.float64)
    Em = np.empty(max(len(c0), 1), np.float64); Es = np.empty(max(len(c0), 1), np.float64)
    _check(lib().glia_hmt_tree_energy_tuples(_np(c0), _np(c1), _np(em), _np(es), len(c0), _np(Em), _np(Es)))
    return Em[:len(c0)].copy(), Es[:len(c0)].copy()


def resolve_tree_ccm(child0, child1, Em, Es):
    """resolveFactorTree (hmt/tree_ccm.hxx:31-47): node indices in pick order."""
    c0 = np.ascontiguousarray(child0, np.int32); c1 = np.ascontiguousarray(child1, np.int32)
    Em = np.ascontiguousarray(Em, np.float64); Es = np.ascontiguousarray(Es, np.float64)
    picks = np.empty(max(len(c0), 1), np.int32)
    n = _count(lib().glia_hmt_resolve_tree_ccm(_np(c0), _np(c1), _np(Em), _np(Es), len(c0), _np(picks), len(picks)))
    return picks[:n].copy()


def tree_ccm_confidence(parent, child0, child1, es, Em, Es):
    """The node value of segment_ccm -b (hmt/main_segment_ccm.cxx:76-86, hmt/tree_ccm.hxx:62-115) -> (pos, neg, confidence) per node."""
    par = np.ascontiguousarray(parent, np.int32); c0 = np.ascontiguousarray(child0, np.int32); c1 = np.ascontiguousarray(child1, np.int32)
    es = np.ascontiguousarray(es, np.float64); Em = np.ascontiguousarray(Em, np.float64); Es = np.ascontiguousarray(Es, np.float64)
    out = [np.empty(max(len(par), 1), np.float64) for _ in range(3)]
    _check(lib().glia_hmt_tree_ccm_confidence(_np(par), _np(c0), _np(c1), _np(es), _np(Em), _np(Es), len(par), _np(out[0]), _np(out[1]),
                                              _np(out[2])))
    return tuple(a[:len(par)].copy() for a in out)


def resolve_trees_greedy(trees):
    """resolveTreeGreedy over several trees (hmt/tree_greedy.hxx:104-152) -> (tree index, node index) per pick.
    trees: list of (label, parent, child0, child1, potential)"""
    nt = len(trees)
    keep = [[np.ascontiguousarray(t[0], np.uint32), np.ascontiguousarray(t[1], np.int32), np.ascontiguousarray(t[2], np.int32),
             np.ascontiguousarray(t[3], np.int32), np.ascontiguousarray(t[4], np.float64)] for t in trees]
    nn = (C.c_int64 * nt)(*[len(k[0]) for k in keep])
    arr = lambda j: (C.c_void_p * nt)(*[k[j].ctypes.data for k in keep])
    tot = sum(len(k[0]) for k in keep)
    pt = np.empty(max(tot, 1), np.int32); pn = np.empty(max(tot, 1), np.int32)
    n = lib().glia_hmt_resolve_trees_greedy(nt, nn, arr(0), arr(1), arr(2), arr(3), arr(4), _np(pt), _np(pn), len(pt))
    assert n >= 0
    return pt[:n].copy(), pn[:n].copy()


class RandomForest(_Handle):
    """alg::RandomForest / alg::EnsembleRandomForest (alg/rf.hxx) loaded from GLIA model files onto the device."""
    _free = "glia_hmt_forest_free"

    def __init__(self, ctx, model_files, predict_label=-1, distributor_args=None):
        if isinstance(model_files, str):
            model_files = [model_files]
        arr = (C.c_char_p * len(model_files))(*[m.encode() for m in model_files])
        dist = (C.c_double * 3)(*distributor_args) if distributor_args is not None else None
        self.ctx = ctx
        self.h = _new(lib().glia_hmt_forest_load, ctx.h, len(model_files), arr, predict_label, dist)

    def predict(self, rows):
        """pred_rf (ml/rf/main_pred_rf.cxx:28-38): the classifier's value for every row of an [n, dim] float64 array -- what bc_feat and
        merge_order_bc(want_feats=True) return.  A NumPy array goes through glia_hmt_forest_predict (rows streamed in chunks) and
        comes back as NumPy; a CUDA tensor (rows contiguous, any row stride) goes through glia_hmt_forest_predict_device and comes
        back as a tensor on the same device."""
        if isinstance(rows, np.ndarray):
            rows = np.ascontiguousarray(rows, dtype=np.float64)
            assert rows.ndim == 2
            out = np.empty(rows.shape[0], np.float64)
            _check(lib().glia_hmt_forest_predict(self.ctx.h, self.h, _np(rows), rows.shape[0], rows.shape[1], _np(out)))
            return out
        import torch
        assert rows.is_cuda and rows.dtype == torch.float64 and rows.dim() == 2 and (rows.shape[1] == 0 or rows.stride(1) == 1)
        assert rows.shape[0] <= 1 or rows.stride(0) >= rows.shape[1]
        out = torch.empty(rows.shape[0], dtype=torch.float64, device=rows.device)
        _fence(rows)
        _check(lib().glia_hmt_forest_predict_device(self.ctx.h, self.h, rows.data_ptr(), rows.shape[0], rows.shape[1],
                                                    rows.stride(0) if rows.shape[0] > 1 else rows.shape[1], out.data_ptr()))
        self.ctx.sync()
        return out


class FeatureStubClassifier(RandomForest):
    """Diagnostic scorer P(merge) = 1 - x[index] (tests; SURVEY.md Appendix D recipe P4)."""

    def __init__(self, ctx, index):
        self.ctx = ctx
        self.h = _new(lib().glia_hmt_forest_stub, ctx.h, index)


def mlp_limits(n1=10, n2=10):
    """glia_hmt_mlp_limits: the tier boundaries of MLP.predict under hidden layers of n1 and n2 units (0, 0: logsig) -- stage_max_dim (the
    longest row staged in LDS; longer rows are read from global memory; 0: none), unit_block (hidden units a thread accumulates at a
    time), slots (waves that split a layer), max_hidden, max_dim.  Host-only."""
    return dict(zip(("stage_max_dim", "unit_block", "slots", "max_hidden", "max_dim"), _outs(lib().glia_hmt_mlp_limits, (C.c_int,) * 5, n1, n2)))


def mlp_loop_limits():
    """glia_hmt_mlp_loop_limits: the most units per hidden layer of an MLP that RegionMap.merge_order_bc takes.  Host-only."""
    return dict(zip(("max_hidden",), _outs(lib().glia_hmt_mlp_loop_limits, (C.c_int,))))


def mlp_tile_rows(dim, n1, n2):
    """glia_hmt_mlp_predict_tile_rows: (rows of a workgroup's tile, whether rows of dim columns are staged in LDS).  Host-only."""
    staged = C.c_int()
    r = _count(lib().glia_hmt_mlp_predict_tile_rows(dim, n1, n2, C.byref(staged)))
    return r, bool(staged.value)


def mlp_file_parse(path):
    """glia_hmt_mlp_file_parse: the weights of a model file (readData(w, file, true)).  Host-only."""
    n, = _outs(lib().glia_hmt_mlp_file_parse, (C.c_int64,), str(path).encode(), None, 0)
    w = np.empty(n, np.float64)
    _outs(lib().glia_hmt_mlp_file_parse, (C.c_int64,), str(path).encode(), _np(w), n)
    return w


class MLP(_Handle):
    """alg::MLP2v / alg::EnsembleMLP2v (alg/nn.hxx) -- pred_mlp's classifier (sshmt/main_pred_mlp.cxx): one model file or three with
    distributor_args = (dim0, dim1, threshold), hidden layers of n1 and n2 units, an optional min/max file to rescale rows by.
    ctx = None gives a host-only model (predict_host).  The arithmetic: DESIGN 3.13."""
    _free = "glia_hmt_mlp_free"

    def __init__(self, ctx, model_files, n1, n2, minmax=None, distributor_args=None):
        if isinstance(model_files, (str, os.PathLike)):
            model_files = [model_files]
        arr = (C.c_char_p * len(model_files))(*[str(m).encode() for m in model_files])
        dist = (C.c_double * 3)(*distributor_args) if distributor_args is not None else None
        self.ctx = ctx
        self.h = _new(lib().glia_hmt_mlp_load, ctx.h if ctx is not None else None, len(model_files), arr, n1, n2,
                      str(minmax).encode() if minmax is not None else None, dist)

    @classmethod
    def from_arrays(cls, ctx, weights, n1, n2, mn=None, mx=None, distributor_args=None):
        """glia_hmt_mlp_create: weights = one array or a list of three (the model files' values)"""
        if isinstance(weights, np.ndarray):
            weights = [weights]
        ws = [np.ascontiguousarray(w, dtype=np.float64) for w in weights]
        ptrs = (C.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
        lens = (C.c_int64 * len(ws))(*[w.size for w in ws])
        dist = (C.c_double * 3)(*distributor_args) if distributor_args is not None else None
        if mn is not None:
            mn = np.ascontiguousarray(mn, dtype=np.float64); mx = np.ascontiguousarray(mx, dtype=np.float64)
        h = _new(lib().glia_hmt_mlp_create, ctx.h if ctx is not None else None, len(ws), ptrs, lens, n1, n2, _np(mn),
                 _np(mx) if mn is not None else None, min(mn.size, mx.size) if mn is not None else 0, dist)
        return cls._wrap(h, ctx=ctx)

    @property
    def dim(self):
        """glia_hmt_mlp_dim: the columns a row must have"""
        return lib().glia_hmt_mlp_dim(self.h)

    def predict_host(self, rows, want_logits=False):
        """glia_hmt_mlp_predict_host: the definition's forward pass on the host, no GPU"""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        assert rows.ndim == 2
        pred = np.empty(rows.shape[0], np.float64); logit = np.empty(rows.shape[0], np.float64)
        _check(lib().glia_hmt_mlp_predict_host(self.h, _np(rows), rows.shape[0], rows.shape[1], _np(pred), _np(logit)))
        return (pred, logit) if want_logits else pred

    def predict(self, rows, want_logits=False):
        """pred_mlp (sshmt/main_pred_mlp.cxx:34-46): the classifier's value for every row of an [n, dim] float64 array.  A NumPy array
        goes through glia_hmt_mlp_predict (rows streamed in chunks, the sigmoid applied on the host) and comes back as NumPy; a CUDA
        tensor (rows contiguous, any row stride) goes through glia_hmt_mlp_predict_device (the sigmoid computed on the device) and comes
        back as a tensor on the same device.  want_logits: (predictions, logits)."""
        if self.ctx is None:
            raise HmtError(ERR_ARG, "MLP.predict: a host-only model (ctx = None) has no device side; use predict_host")
        if isinstance(rows, np.ndarray):
            rows = np.ascontiguousarray(rows, dtype=np.float64)
            assert rows.ndim == 2
            pred = np.empty(rows.shape[0], np.float64); logit = np.empty(rows.shape[0], np.float64)
            _check(lib().glia_hmt_mlp_predict(self.ctx.h, self.h, _np(rows), rows.shape[0], rows.shape[1], _np(pred), _np(logit)))
            return (pred, logit) if want_logits else pred
        import torch
        assert rows.is_cuda and rows.dtype == torch.float64 and rows.dim() == 2 and (rows.shape[1] == 0 or rows.stride(1) == 1)
        assert rows.shape[0] <= 1 or rows.stride(0) >= rows.shape[1]
        pred = torch.empty(rows.shape[0], dtype=torch.float64, device=rows.device)
        logit = torch.empty(rows.shape[0], dtype=torch.float64, device=rows.device) if want_logits else None
        _fence(rows)
        _check(lib().glia_hmt_mlp_predict_device(self.ctx.h, self.h, rows.data_ptr(), rows.shape[0], rows.shape[1],
                                                 rows.stride(0) if rows.shape[0] > 1 else rows.shape[1], pred.data_ptr(), _ptr(logit)))
        self.ctx.sync()
        return (pred, logit) if want_logits else pred


class Logsig(MLP):
    """alg::Logsig (alg/function.hxx:33-34) -- pred_logsig's classifier (sshmt/main_pred_logsig.cxx): 1 / (1 + exp(-(x, 1) . w))."""

    def __init__(self, ctx, model_file):
        super().__init__(ctx, model_file, 0, 0)


def mlp_predict_host(weights, n1, n2, rows, mn=None, mx=None, distributor_args=None):
    """glia_hmt_mlp_predict_host on arrays: (predictions, logits) of the definition's forward pass; no GPU, no context."""
    m = MLP.from_arrays(None, weights, n1, n2, mn, mx, distributor_args)
    try:
        return m.predict_host(rows, want_logits=True)
    finally:
        m.close()


class MLPTrainOpts(C.Structure):
    """glia_hmt_mlp_train_opts: the options of train_sshmt_mlp's supervised part (sshmt/main_train_sshmt_mlp.cxx:20-47); the fields
    after seed are refused by train_mlp unless they hold their defaults; train_sshmt honours wu and update_sigma_u"""
    _fields_ = [("n1", C.c_int), ("n2", C.c_int), ("wr", C.c_double), ("ws", C.c_double), ("sigma_s", C.c_double), ("update_sigma_s", C.c_int),
                ("optimizer", C.c_int), ("step", C.c_double), ("step_decay", C.c_double), ("fixed_step_decay_iterations", C.c_int),
                ("sigma_update_step_period", C.c_int), ("max_iterations", C.c_int), ("n_sigma_updates", C.c_int), ("pos_target", C.c_double),
                ("neg_target", C.c_double), ("min_sigma2", C.c_double), ("seed", C.c_uint64), ("wu", C.c_double), ("update_sigma_u", C.c_int),
                ("sup_batch_size", C.c_int), ("uns_batch_size", C.c_int), ("balance_sup_batch", C.c_int), ("alt_su", C.c_int)]


class MLPTrainTiming(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("ms_total", "ms_upload", "ms_weights", "ms_chunk", "ms_fold", "ms_readback")] + \
               [(k, C.c_int64) for k in ("evals", "grad_evals", "iterations")] + [("device_bytes", C.c_uint64)]


MLP_TRAIN_RECORD = np.dtype([("fx", np.float64), ("xnorm", np.float64), ("gnorm", np.float64), ("step", np.float64), ("sigma2", np.float64),
                             ("round", np.int32), ("t", np.int32), ("kind", np.int32), ("rollbacks", np.int32)])      # glia_hmt_mlp_train_record


def mlp_train_limits():
    """glia_hmt_mlp_train_limits: rows of a chunk of the gradient's reduction, the most hidden units, the most columns"""
    return dict(zip(("chunk_rows", "max_hidden", "max_dim"), _outs(lib().glia_hmt_mlp_train_limits, (C.c_int,) * 3)))


def mlp_init_weights(seed, n):
    """glia_hmt_mlp_init_weight: the first n initial weights of an MLP under seed.  Host-only."""
    f = lib().glia_hmt_mlp_init_weight
    return np.array([f(seed, p) for p in range(n)], np.float64)


def rows_minmax(blocks):
    """glia_hmt_rows_minmax: the (minima, maxima) normalize_sample finds over several [n_i, dim] row blocks (util/stats.hxx:280-314)"""
    if isinstance(blocks, np.ndarray) and blocks.ndim == 2:
        blocks = [blocks]
    keep = [np.ascontiguousarray(b, dtype=np.float64) for b in blocks]
    dim = keep[0].shape[1]
    assert all(b.ndim == 2 and b.shape[1] == dim for b in keep)
    ptrs = (C.c_void_p * len(keep))(*[b.ctypes.data for b in keep])
    lens = (C.c_int64 * len(keep))(*[b.shape[0] for b in keep])
    mn = np.empty(dim, np.float64); mx = np.empty(dim, np.float64)
    _check(lib().glia_hmt_rows_minmax(ptrs, lens, len(keep), dim, _np(mn), _np(mx)))
    return mn, mx


class MLPModel(_Handle):
    """A trained MLP / logsig model on the host (glia_hmt_mlp_model): the weights after every sigma round, the optimiser's trace, the
    sigmas, whether training stopped on a value that was not finite."""
    _free = "glia_hmt_mlp_model_free"

    def __init__(self, handle, n1, n2):
        self.h = handle
        self.n1, self.n2 = n1, n2
        info = _outs(lib().glia_hmt_mlp_model_info, (C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int), self.h)
        self.rounds, self.n_weights, n_trace, stopped, self.n_used_rows, n_sigma = info
        self.stopped_nonfinite = bool(stopped)
        self.trace = np.zeros(n_trace, MLP_TRAIN_RECORD)
        _check(lib().glia_hmt_mlp_model_trace(self.h, _np(self.trace) if n_trace else None))
        self.sigma2 = np.zeros(n_sigma); self.sigma2_eval = np.zeros(n_sigma)
        _check(lib().glia_hmt_mlp_model_sigmas(self.h, _np(self.sigma2), _np(self.sigma2_eval)))
        # the merge-path term's (train_sshmt): sigma_u^2 per sigma update (zeros while the term is off), its paths and unlabelled rows
        self.sigma_u2 = np.zeros(n_sigma); self.sigma_u2_eval = np.zeros(n_sigma)
        _check(lib().glia_hmt_mlp_model_sigmas_u(self.h, _np(self.sigma_u2), _np(self.sigma_u2_eval)))
        self.n_paths, self.n_uns_rows = _outs(lib().glia_hmt_mlp_model_paths, (C.c_int64, C.c_int64), self.h)

    def weights(self, round=-1):
        w = np.empty(self.n_weights, np.float64)
        _check(lib().glia_hmt_mlp_model_weights(self.h, round, _np(w)))
        return w

    def write(self, path, round=-1):
        """one %.17g double per line: reads back bit for bit (mlp_file_parse, MLP(...))"""
        _check(lib().glia_hmt_mlp_model_write(self.h, str(path).encode(), round))

    def mlp(self, ctx, round=-1):
        """the classifier MLP.predict / RegionMap.merge_order_bc take, with the min/max table the training used; ctx None: host-only"""
        return MLP._wrap(_new(lib().glia_hmt_mlp_model_create_mlp, ctx.h if ctx is not None else None, self.h, round), ctx=ctx)


def _train_args(who, o, n1, n2, dim, minmax, init, opts):
    """What train_mlp and train_sshmt marshal alike.  o: MLPTrainOpts or SSHMTTrainOpts holding the defaults; receives n1, n2 and opts.
    Returns the trailing (options, minima, maxima, initial weights, model handle) arguments of the call, the handle, and the arrays
    the pointers look into."""
    base = getattr(o, "base", o)
    base.n1, base.n2 = n1, n2
    for k, v in opts.items():
        if k in dict(MLPTrainOpts._fields_):
            setattr(base, k, v)
        elif o is not base and k in dict(SSHMTTrainOpts._fields_) and k != "base":
            setattr(o, k, v)
        else:
            raise TypeError(who + ": unknown option " + k)
    mn = mx = None
    if minmax is not None:
        mn = np.ascontiguousarray(minmax[0], dtype=np.float64); mx = np.ascontiguousarray(minmax[1], dtype=np.float64)
        if min(mn.size, mx.size) < dim:
            raise HmtError(ERR_ARG, who + ": fewer min/max entries than columns")
    if init is not None:
        init = np.ascontiguousarray(init, dtype=np.float64)
        D = dim + 1
        if init.size != (D * n1 + (n1 + 1) * n2 + n2 + 1 if n1 else D):
            raise HmtError(ERR_ARG, who + ": %d initial weights do not fit the model" % init.size)
    h = C.c_void_p()
    return (C.byref(o), _np(mn), _np(mx), _np(init), C.byref(h)), h, (mn, mx, init)


def train_mlp(ctx, rows, labels, n1=10, n2=10, minmax=None, init=None, **opts):
    """train_sshmt_mlp / train_sshmt_logsig without the unsupervised term: rows [n, dim] float64, labels [n] (+1 / -1; any
    other label drops the row), n1 = n2 = 0 for logsig, minmax = (minima, maxima) to rescale rows by, init = initial weights.  Options:
    the fields of MLPTrainOpts (wr, ws, sigma_s, update_sigma_s, optimizer, step, step_decay, fixed_step_decay_iterations,
    sigma_update_step_period, max_iterations, n_sigma_updates, pos_target, neg_target, min_sigma2, seed).  Forward pass, backward pass and
    the gradient's reduction run on the device; ctx = None runs the definition on one host thread (train_mlp_host)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
    assert rows.ndim == 2 and labels.shape[0] == rows.shape[0]
    o = MLPTrainOpts()
    lib().glia_hmt_mlp_train_opts_default(C.byref(o))
    args, h, keep = _train_args("train_mlp", o, n1, n2, rows.shape[1], minmax, init, opts)
    _check(lib().glia_hmt_mlp_train(ctx.h if ctx is not None else None, _np(rows), rows.shape[0], rows.shape[1], _np(labels), *args))
    return MLPModel(h, n1, n2)


def train_mlp_host(rows, labels, n1=10, n2=10, minmax=None, init=None, **opts):
    """glia_hmt_mlp_train_host: the definition of DESIGN 3.14 on one host thread; no GPU, no context"""
    return train_mlp(None, rows, labels, n1, n2, minmax, init, **opts)


def last_mlp_train_timing(ctx):
    return _struct_out(lib().glia_hmt_last_mlp_train_timing, MLPTrainTiming, ctx.h)


class SSHMTTrainOpts(C.Structure):
    """glia_hmt_sshmt_train_opts: MLPTrainOpts (wu and update_sigma_u honoured) and the merge-path term's own options
    (sshmt/main_train_sshmt_mlp.cxx:41-53)"""
    _fields_ = [("base", MLPTrainOpts), ("sigma_u", C.c_double), ("merge_target", C.c_double), ("path_target", C.c_double),
                ("max_path_length", C.c_int), ("min_path_length", C.c_int)]


class SSHMTBlock(C.Structure):
    _fields_ = [("rows", C.c_void_p), ("order", C.c_void_p), ("n_merges", C.c_int64)]      # glia_hmt_sshmt_block


class SSHMTTrainTiming(C.Structure):
    _fields_ = [("sup", MLPTrainTiming)] + \
               [(k, C.c_double) for k in ("ms_u_upload", "ms_u_weights", "ms_u_forward", "ms_u_paths", "ms_u_gather", "ms_u_chunk", "ms_u_fold",
                                          "ms_u_readback")] + \
               [(k, C.c_int64) for k in ("u_evals", "u_grad_evals", "n_paths", "n_uns_rows")] + [("u_device_bytes", C.c_uint64)]


def merge_paths(order, max_len=3, min_len=2):
    """glia_hmt_merge_paths: the merge paths of an order [n, 3] (hmt/tree_build.hxx:150-180, the bounded genMergePaths) as a list of
    int64 arrays of merge indices, bottom-up, by ascending first member.  Host-only."""
    o = np.ascontiguousarray(order, dtype=np.uint32).reshape(-1, 3)
    n_paths, n_members = C.c_int64(0), C.c_int64(0)
    args = (_np(o) if len(o) else None, len(o), max_len, min_len, C.byref(n_paths), C.byref(n_members))
    _check(lib().glia_hmt_merge_paths(*args, None, None))
    off = np.zeros(n_paths.value + 1, np.int64); mem = np.zeros(max(n_members.value, 1), np.int64)
    _check(lib().glia_hmt_merge_paths(*args, _np(off), _np(mem)))
    return [mem[off[i]:off[i + 1]].copy() for i in range(n_paths.value)]


def _sshmt_inputs(who, rows, labels, unlabelled):
    """What train_sshmt and train_sshmt_batches marshal alike: the labelled rows and labels (empty when None), the unlabelled blocks as
    contiguous arrays, the number of columns and the glia_hmt_sshmt_block array whose pointers look into the blocks."""
    blocks = [(np.ascontiguousarray(r, dtype=np.float64), np.ascontiguousarray(o, dtype=np.uint32).reshape(-1, 3)) for r, o in unlabelled]
    dim = blocks[0][0].shape[1] if rows is None else np.asarray(rows).shape[1]
    rows = np.zeros((0, dim)) if rows is None else np.ascontiguousarray(rows, dtype=np.float64)
    labels = np.zeros(0, np.int32) if labels is None else np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
    assert rows.ndim == 2 and labels.shape[0] == rows.shape[0]
    for r, o in blocks:
        if r.ndim != 2 or r.shape[1] != dim or r.shape[0] != o.shape[0]:
            raise HmtError(ERR_ARG, who + ": a block needs one row of %d columns per merge" % dim)
    arr = (SSHMTBlock * max(len(blocks), 1))()
    for i, (r, od) in enumerate(blocks):
        arr[i] = SSHMTBlock(r.ctypes.data if len(r) else None, od.ctypes.data if len(od) else None, len(od))
    return rows, labels, blocks, dim, arr


def train_sshmt(ctx, rows, labels, unlabelled=(), n1=10, n2=10, minmax=None, init=None, **opts):
    """train_sshmt_mlp / train_sshmt_logsig with the merge-path term.  rows / labels as train_mlp takes them; both may be
    None when ws is off.  unlabelled: [(rows_u [n_i, dim], order_u [n_i, 3]), ...], row k of a block = merge k of its order.  Options:
    the fields of MLPTrainOpts (wu and update_sigma_u included) and sigma_u, merge_target, path_target, max_path_length,
    min_path_length.  ctx = None runs the definition on one host thread (train_sshmt_host)."""
    rows, labels, blocks, dim, arr = _sshmt_inputs("train_sshmt", rows, labels, unlabelled)
    o = SSHMTTrainOpts()
    lib().glia_hmt_sshmt_train_opts_default(C.byref(o))
    args, h, keep = _train_args("train_sshmt", o, n1, n2, dim, minmax, init, opts)
    _check(lib().glia_hmt_sshmt_train(ctx.h if ctx is not None else None, _np(rows) if len(rows) else None, rows.shape[0], dim,
                                      _np(labels) if len(labels) else None, arr, len(blocks), *args))
    return MLPModel(h, n1, n2)


def train_sshmt_host(rows, labels, unlabelled=(), n1=10, n2=10, minmax=None, init=None, **opts):
    """glia_hmt_sshmt_train_host: the definition of DESIGN 3.15 on one host thread; no GPU, no context"""
    return train_sshmt(None, rows, labels, unlabelled, n1, n2, minmax, init, **opts)


def last_sshmt_train_timing(ctx):
    """the last train_sshmt call of the context: the supervised evaluator's fields under "sup", then the merge-path term's stages"""
    return _struct_out(lib().glia_hmt_last_sshmt_train_timing, SSHMTTrainTiming, ctx.h)


class BatchOpts(C.Structure):
    """glia_hmt_batch_opts: the sampler's seed (--bseed), epochs per iteration (--te 1), batches per iteration when that is <= 0 (--tb 1)"""
    _fields_ = [("seed", C.c_uint64), ("epochs_per_iteration", C.c_int), ("batches_per_iteration", C.c_int)]


class BatchTiming(C.Structure):
    _fields_ = [("steps", C.c_int64), ("batches", C.c_int64), ("ms_plan", C.c_double), ("ms_upload", C.c_double), ("ms_steps", C.c_double),
                ("ms_wall", C.c_double), ("syncs", C.c_int64), ("route", C.c_int32), ("plan_bytes", C.c_uint64)]      # glia_hmt_batch_timing


def _batch_opts(batch):
    """BatchOpts from None (the defaults), a BatchOpts or a dict of its fields"""
    bo = BatchOpts()
    lib().glia_hmt_batch_opts_default(C.byref(bo))
    if isinstance(batch, BatchOpts):
        return batch
    for k, v in (batch or {}).items():
        if k not in dict(BatchOpts._fields_):
            raise TypeError("BatchOpts: unknown field " + k)
        setattr(bo, k, v)
    return bo


def train_mlp_batches(ctx, rows, labels, n1=10, n2=10, minmax=None, init=None, batch=None, **opts):
    """glia_hmt_mlp_train_batches: train_mlp with mini-batches.  Options as train_mlp's, with sup_batch_size (--bss) and
    balance_sup_batch (--bb) honoured; batch: a BatchOpts or a dict of its fields (seed, epochs_per_iteration, batches_per_iteration).
    The batches are this library's sampler's, a function of the seed -- not the reference's.  With no sampler asked for the result is
    train_mlp's.  ctx = None: the definition on one host thread."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
    assert rows.ndim == 2 and labels.shape[0] == rows.shape[0]
    o = MLPTrainOpts()
    lib().glia_hmt_mlp_train_opts_default(C.byref(o))
    bo = _batch_opts(batch)
    args, h, keep = _train_args("train_mlp_batches", o, n1, n2, rows.shape[1], minmax, init, opts)
    _check(lib().glia_hmt_mlp_train_batches(ctx.h if ctx is not None else None, _np(rows), rows.shape[0], rows.shape[1], _np(labels), args[0],
                                            C.byref(bo), *args[1:]))
    return MLPModel(h, n1, n2)


def train_sshmt_batches(ctx, rows, labels, unlabelled=(), n1=10, n2=10, minmax=None, init=None, batch=None, **opts):
    """glia_hmt_sshmt_train_batches: train_sshmt with mini-batches: sup_batch_size, balance_sup_batch and uns_batch_size
    (--bsu: batches of merge PATHS) honoured; batch as train_mlp_batches takes it.  ctx = None: the definition on one host thread."""
    rows, labels, blocks, dim, arr = _sshmt_inputs("train_sshmt_batches", rows, labels, unlabelled)
    o = SSHMTTrainOpts()
    lib().glia_hmt_sshmt_train_opts_default(C.byref(o))
    bo = _batch_opts(batch)
    args, h, keep = _train_args("train_sshmt_batches", o, n1, n2, dim, minmax, init, opts)
    _check(lib().glia_hmt_sshmt_train_batches(ctx.h if ctx is not None else None, _np(rows) if len(rows) else None, rows.shape[0], dim,
                                              _np(labels) if len(labels) else None, arr, len(blocks), args[0], C.byref(bo), *args[1:]))
    return MLPModel(h, n1, n2)


def batch_plan(labels, n_paths, k, sup_batch_size=-1, uns_batch_size=-1, balance_sup_batch=0, pos_target=0.05, neg_target=0.95, seed=0):
    """glia_hmt_batch_plan: the next k draws of the samplers of DESIGN 3.17 for labelled rows with these labels (+1 / -1, every row
    counts) and n_paths merge paths -> (sup, uns, end): per draw the int32 array of rows, the int32 array of paths (empty without that
    sampler) and whether the draw ended the epoch.  Host-only."""
    labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
    n_sup, n_uns = C.c_int64(0), C.c_int64(0)
    head = (_np(labels) if len(labels) else None, len(labels), n_paths, sup_batch_size, uns_batch_size, balance_sup_batch, pos_target, neg_target,
            seed, k, C.byref(n_sup), C.byref(n_uns))
    _check(lib().glia_hmt_batch_plan(*head, None, None, None, None, None))
    so = np.zeros(k + 1, np.int64); uo = np.zeros(k + 1, np.int64)
    sr = np.zeros(max(n_sup.value, 1), np.int32); up = np.zeros(max(n_uns.value, 1), np.int32)
    end = np.zeros(max(k, 1), np.int32)
    _check(lib().glia_hmt_batch_plan(*head, _np(so), _np(sr), _np(uo), _np(up), _np(end)))
    return ([sr[so[i]:so[i + 1]].copy() for i in range(k)], [up[uo[i]:uo[i + 1]].copy() for i in range(k)], [bool(e) for e in end[:k]])


def last_batch_timing(ctx):
    """the last train_*_batches call of the context: mini-batch steps, batches, plan build and upload, the steps' device time, waits"""
    return _struct_out(lib().glia_hmt_last_batch_timing, BatchTiming, ctx.h)


class TrainOpts(C.Structure):
    """glia_hmt_train_opts: train_rf's options (ml/rf/main_train_rf.cxx:11-15) + max_depth + seed"""
    _fields_ = [("ntree", C.c_int), ("mtry", C.c_int), ("sample_ratio", C.c_double), ("nodesize", C.c_int), ("balance", C.c_int),
                ("max_depth", C.c_int), ("seed", C.c_uint64)]


class ForestTrainTiming(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("ms_total", "ms_upload", "ms_bootstrap", "ms_prepare", "ms_gather", "ms_sort", "ms_scan", "ms_split",
                                          "ms_partition", "ms_download")] + \
               [(k, C.c_int64) for k in ("levels", "launches", "batches", "trees_in_flight", "nodes")] + [("device_bytes", C.c_uint64)]


class OobOpts(C.Structure):
    """glia_hmt_oob_opts"""
    _fields_ = [("oob", C.c_int), ("importance", C.c_int)]


class ForestOobTiming(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("ms_walk", "ms_tally", "ms_importance")] + \
               [(k, C.c_int64) for k in ("oob_rows", "walks_nominal", "walks_done")] + [("device_bytes", C.c_uint64)]


class ForestModel(_Handle):
    """A trained forest on the host (glia_hmt_forest_model): every array of the GLIA model file."""
    _free = "glia_hmt_forest_model_free"
    _TREE = (("xbestsplit", np.float64, 1), ("treemap", np.int32, 2), ("nodestatus", np.int32, 1), ("nodeclass", np.int32, 1),
             ("bestvar", np.int32, 1))
    _CLASS = (("classwt", np.float64), ("cutoff", np.float64), ("orig_labels", np.int32), ("new_labels", np.int32))

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.h = handle

    @classmethod
    def from_arrays(cls, arrays, ctx=None):
        """a model from a dict like synth_forest.synthetic_forest returns (+ optional mtry, classwt, cutoff, new_labels); host-only"""
        ntree, nrnodes = arrays["xbestsplit"].shape
        nclass = len(arrays["orig_labels"])
        a = dict(arrays)
        a.setdefault("classwt", np.ones(nclass)); a.setdefault("cutoff", np.full(nclass, 1.0 / nclass))
        a.setdefault("new_labels", np.arange(1, nclass + 1))
        keep = [np.ascontiguousarray(a[k], dtype=t) for k, t, _ in cls._TREE] + [np.ascontiguousarray(a["ndbigtree"], dtype=np.int32)] + \
               [np.ascontiguousarray(a[k], dtype=t) for k, t in cls._CLASS]
        return cls(ctx, _new(lib().glia_hmt_forest_model_from_arrays, ntree, nrnodes, nclass, int(a.get("mtry", 3)), *[_np(x) for x in keep]))

    def sizes(self):
        return dict(zip(("ntree", "nrnodes", "nclass", "mtry"), _outs(lib().glia_hmt_forest_model_sizes, (C.c_int,) * 4, self.h)))

    def arrays(self):
        """dict of the model's arrays in synth_forest's layout: tree arrays [ntree, nrnodes], treemap [ntree, nrnodes, 2]"""
        s = self.sizes()
        out = {k: np.zeros((s["ntree"], s["nrnodes"]) + ((2,) if w == 2 else ()), t) for k, t, w in self._TREE}
        out["ndbigtree"] = np.zeros(s["ntree"], np.int32)
        out.update({k: np.zeros(s["nclass"], t) for k, t in self._CLASS})
        order = [k for k, _, _ in self._TREE] + ["ndbigtree"] + [k for k, _ in self._CLASS]
        _check(lib().glia_hmt_forest_model_arrays(self.h, *[_np(out[k]) for k in order]))
        out["mtry"] = s["mtry"]
        return out

    def oob(self):
        """dict of the out-of-bag arrays of a model trained with oob=True and / or importance=True, shaped as the model file
        holds them: outcl [N], counttr [nclass, N], votes [N, nclass], oob_times [N], errtr [ntree, nclass + 1] with the integers it
        divides (err_wrong, err_seen); importance [D, nclass + 2], importanceSD [D, nclass + 1].  HmtError when the model has none."""
        N, D, has_oob, has_imp = _outs(lib().glia_hmt_forest_model_oob_sizes, (C.c_int64, C.c_int, C.c_int, C.c_int), self.h)
        s = self.sizes()
        nc, nt = s["nclass"], s["ntree"]
        out = {}
        if has_oob:
            out.update(outcl=np.zeros(N, np.int32), counttr=np.zeros((nc, N), np.int32), votes=np.zeros((N, nc), np.int32),
                       oob_times=np.zeros(N, np.int32), errtr=np.zeros((nt, nc + 1)), err_wrong=np.zeros((nt, nc + 1), np.int64),
                       err_seen=np.zeros((nt, nc + 1), np.int64))
        if has_imp:
            out.update(importance=np.zeros((D, nc + 2)), importanceSD=np.zeros((D, nc + 1)))
        order = ("outcl", "counttr", "votes", "oob_times", "errtr", "err_wrong", "err_seen", "importance", "importanceSD")
        _check(lib().glia_hmt_forest_model_oob_arrays(self.h, *[_np(out[k]) if k in out else None for k in order]))
        return out

    def set_oob(self, n_rows, dim, arrays):
        """host-only: gives the model out-of-bag arrays from a dict shaped like oob()'s (glia_hmt_forest_model_set_oob)"""
        order = (("outcl", np.int32), ("counttr", np.int32), ("votes", np.int32), ("oob_times", np.int32), ("errtr", np.float64),
                 ("importance", np.float64), ("importanceSD", np.float64))
        keep = [np.ascontiguousarray(arrays[k], dtype=t) if k in arrays else None for k, t in order]
        _check(lib().glia_hmt_forest_model_set_oob(self.h, n_rows, dim, *[_np(x) for x in keep]))

    def write(self, path):
        _check(lib().glia_hmt_forest_model_write(self.h, str(path).encode()))

    def forest(self, predict_label=-1, ctx=None):
        """the classifier RandomForest.predict / merge_order_bc take, without a trip through a file"""
        ctx = ctx or self.ctx
        return RandomForest._wrap(_new(lib().glia_hmt_forest_from_model, ctx.h, self.h, predict_label), ctx=ctx)


def train_forest(ctx, rows, labels, oob=False, importance=False, **opts):
    """train_rf (ml/rf/main_train_rf.cxx): grows the forest on the device by the rule of DESIGN 3.12.  rows [n, dim] float64, labels [n]
    integers; options ntree, mtry, sample_ratio, nodesize, balance, max_depth, seed (defaults: glia_hmt_train_opts_default).  oob /
    importance: also the out-of-bag error and the variable importances (ForestModel.oob()); the trees are the same."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
    assert rows.ndim == 2 and labels.shape[0] == rows.shape[0]
    o = TrainOpts()
    lib().glia_hmt_train_opts_default(C.byref(o))
    for k, v in opts.items():
        if k not in dict(TrainOpts._fields_):
            raise TypeError("train_forest: unknown option " + k)
        setattr(o, k, v)
    if oob or importance:
        oo = OobOpts(1 if oob else 0, 1 if importance else 0)
        h = _new(lib().glia_hmt_forest_train_oob, ctx.h, _np(rows), rows.shape[0], rows.shape[1], _np(labels), C.byref(o), C.byref(oo))
    else:
        h = _new(lib().glia_hmt_forest_train, ctx.h, _np(rows), rows.shape[0], rows.shape[1], _np(labels), C.byref(o))
    return ForestModel(ctx, h)


def last_forest_train_timing(ctx):
    return _struct_out(lib().glia_hmt_last_forest_train_timing, ForestTrainTiming, ctx.h)


def last_forest_oob_timing(ctx):
    """the out-of-bag passes of the last train_forest call (all zero when it asked for neither)"""
    return _struct_out(lib().glia_hmt_last_forest_oob_timing, ForestOobTiming, ctx.h)


class Slab(C.Structure):
    """glia_hmt_slab (include/glia_hmt.h)"""
    _fields_ = [("dims_local", C.c_int64 * 3), ("z_global_of_plane0", C.c_int64), ("z_begin", C.c_int64), ("z_end", C.c_int64),
                ("d_labels", C.c_void_p), ("d_pb", C.c_void_p), ("cfg", C.POINTER(FeatConfig))]


class DistStats(C.Structure):
    _fields_ = [("records", C.c_uint64), ("cut_records", C.c_uint64), ("bytes_cut_exchange", C.c_uint64), ("bytes_to_loop_owner", C.c_uint64)]


class Comm(_Handle):
    """glia_hmt_comm: the ranks of this process in the slab route (glia_amd/csrc/slab_dist.cpp)."""
    _free = "glia_hmt_comm_destroy"

    def __init__(self, ctx, world, rank=None, unique_id=None):
        """rank None: all `world` ranks in this process on ctx's GPU (device copies); else one RCCL rank (unique_id: 128 bytes
        from Comm.unique_id() on one rank)."""
        self.ctx, self.world = ctx, world
        if rank is None:
            self.h = _new(lib().glia_hmt_comm_create_local, ctx.h, world)
            self.local = list(range(world))
        else:
            buf = (C.c_char * 128).from_buffer_copy(unique_id)
            self.h = _new(lib().glia_hmt_comm_create_rccl, ctx.h, world, rank, buf)
            self.local = [rank]

    @staticmethod
    def unique_id():
        buf = (C.c_char * 128)()
        _check(lib().glia_hmt_comm_unique_id(buf))
        return bytes(buf)


def slab_range(nz, world, rank):
    """glia_hmt_slab_range -> (first plane handed in, planes handed in, z_begin, z_end)"""
    return tuple(_outs(lib().glia_hmt_slab_range, (C.c_int64,) * 4, nz, world, rank))


def build_distributed(ctx, comm, slabs, nz_global, only_contour=False, loop_owner=0, with_values=False):
    """glia_hmt_rag_build_distributed.  slabs: one (labels, pb, first_plane, z_begin, z_end, cfg) per LOCAL rank of comm, in rank
    order (labels / pb: CUDA tensors of the planes handed in).  Returns (RegionMap of the whole volume | None, DistStats)."""
    arr = (Slab * len(slabs))()
    keep = []
    for i, (lab, pb, first, zb, ze, cfg) in enumerate(slabs):
        assert lab.is_cuda and lab.is_contiguous() and lab.dim() == 3
        _fence(lab)
        arr[i].dims_local[0], arr[i].dims_local[1], arr[i].dims_local[2] = lab.shape[2], lab.shape[1], lab.shape[0]
        arr[i].z_global_of_plane0, arr[i].z_begin, arr[i].z_end = first, zb, ze
        arr[i].d_labels = lab.data_ptr()
        arr[i].d_pb = _ptr(pb)
        arr[i].cfg = C.pointer(cfg) if cfg is not None else None
        keep.append((lab, pb, cfg))
    h = C.c_void_p()
    st = DistStats()
    _check(lib().glia_hmt_rag_build_distributed(ctx.h, comm.h, arr, nz_global, int(only_contour), int(with_values), loop_owner, C.byref(h),
                                                C.byref(st)))
    rm = RegionMap._wrap(h)._configure(ctx, slabs[0][5]) if h else None
    if rm is not None:
        rm._keep = keep
    return rm, st


class BcLabelOpts(C.Structure):
    _fields_ = [("metric", C.c_int), ("tweak", C.c_int), ("max_prec_drop", C.c_double), ("opt_split", C.c_int), ("global_opt", C.c_int)]


class BcFeatTiming(C.Structure):
    _fields_ = [("ms_plan", C.c_double), ("ms_sets", C.c_double), ("ms_rows", C.c_double), ("height", C.c_int64),
                ("launches", C.c_int64), ("path_updates", C.c_int64), ("route", C.c_int)]


class BcLabelTiming(C.Structure):
    _fields_ = [("ms_count", C.c_double), ("ms_nodes", C.c_double), ("ms_rules", C.c_double), ("entries", C.c_int64),
                ("moves", C.c_int64), ("node_pairs", C.c_int64)]


class RegionMap(_Handle):
    """Device-resident region adjacency structure with sufficient statistics.
    Mirrors TRegionMap(image, mask, onlyContour) (type/region_map.hxx:38-40)."""
    _free = "glia_hmt_rag_free"

    def __init__(self, ctx, labels, pb=None, mask=None, only_contour=False, cfg=None, slab=None):
        """slab = (z_global_of_plane0, nz_global, z_begin, z_end): build the PARTIAL map of a z-slab whose planes
        (plus halo planes) are `labels` / `pb` (see include/glia_hmt.h, glia_hmt_rag_build_slab)."""
        self._configure(ctx, cfg, (labels, pb, mask))
        assert labels.is_cuda and labels.is_contiguous() and labels.element_size() == 4
        _fence(labels)
        self.shape = tuple(labels.shape)
        self.dim, d = _dims(self.shape)
        cfg_ref = C.byref(cfg) if cfg is not None else None
        if slab is None:
            self.h = _new(lib().glia_hmt_rag_build, ctx.h, self.dim, d, labels.data_ptr(), _ptr(mask), int(only_contour), _ptr(pb), cfg_ref)
        else:
            gz0, gnz, zb, ze = slab
            self.h = _new(lib().glia_hmt_rag_build_slab, ctx.h, d, gz0, gnz, zb, ze, labels.data_ptr(), int(only_contour), _ptr(pb), cfg_ref)

    def _configure(self, ctx, cfg, volumes=(None, None, None)):
        """what a built map and a map around a handle the library returned (_wrap) hold alike"""
        self.ctx, self.cfg, self._keep = ctx, cfg, volumes + (cfg,)
        self.bins = cfg.region[0].bins if cfg is not None and cfg.n_region else \
            (cfg.boundary[0].bins if cfg is not None and cfg.n_boundary else 8)
        self.nthr = cfg.n_thresholds if cfg is not None else 0
        return self

    @property
    def num_regions(self):
        return lib().glia_hmt_rag_num_regions(self.h)

    @property
    def num_pairs(self):
        return lib().glia_hmt_rag_num_pairs(self.h)

    def num_channels(self):
        return lib().glia_hmt_rag_num_channels(self.h)

    @staticmethod
    def merge(ctx, parts):
        """glia_hmt_rag_merge: combine the partial maps of several slabs (same configuration)."""
        arr = (C.c_void_p * len(parts))(*[p.h for p in parts])
        return RegionMap._wrap(_new(lib().glia_hmt_rag_merge, ctx.h, arr, len(parts)))._configure(ctx, parts[0].cfg)

    def to_tensors(self):
        """The compact record arrays as torch tensors on the context's device (for torch.distributed)."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        R, P = self.num_regions, self.num_pairs
        rw, pw = _outs(lib().glia_hmt_rag_device_arrays, (C.c_int, C.c_int), self.h, None, None, None, None, None)
        t = dict(rlabel=torch.empty(R, dtype=torch.int32, device=dev), rrec=torch.empty((R, rw), dtype=torch.int32, device=dev),
                 pa=torch.empty(P, dtype=torch.int32, device=dev), pb=torch.empty(P, dtype=torch.int32, device=dev),
                 prec=torch.empty((P, pw), dtype=torch.int32, device=dev))
        _check(lib().glia_hmt_rag_copy_arrays(self.h, *[t[k].data_ptr() for k in ("rlabel", "rrec", "pa", "pb", "prec")]))
        # further image channels (feature lists with several volumes): same keys, one more record set each
        for k in range(1, lib().glia_hmt_rag_num_channels(self.h)):
            t["rrec%d" % k] = torch.empty((R, rw), dtype=torch.int32, device=dev)
            t["prec%d" % k] = torch.empty((P, pw), dtype=torch.int32, device=dev)
            _check(lib().glia_hmt_rag_copy_channel(self.h, k, t["rrec%d" % k].data_ptr(), t["prec%d" % k].data_ptr()))
        return t

    def cut_flags(self, labels_slab, z_begin, z_end):
        """glia_hmt_rag_cut_flags: boolean CUDA tensors (regions, pairs) -- records whose label occurs next to a cut of the slab."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        _, d = _dims(tuple(labels_slab.shape))
        rcut = torch.zeros(max(self.num_regions, 1), dtype=torch.uint8, device=dev)
        pcut = torch.zeros(max(self.num_pairs, 1), dtype=torch.uint8, device=dev)
        _fence(labels_slab)
        _check(lib().glia_hmt_rag_cut_flags(self.ctx.h, self.h, d, z_begin, z_end, labels_slab.data_ptr(), rcut.data_ptr(), pcut.data_ptr()))
        return rcut[:self.num_regions].bool(), pcut[:self.num_pairs].bool()

    @staticmethod
    def from_tensors(ctx, like, t):
        for k in t:
            assert t[k].is_cuda and t[k].is_contiguous()
        _fence(t["rlabel"])
        h = _new(lib().glia_hmt_rag_from_arrays, ctx.h, like.h, t["rlabel"].numel(), t["rlabel"].data_ptr(), t["rrec"].data_ptr(), t["pa"].numel(),
                 t["pa"].data_ptr(), t["pb"].data_ptr(), t["prec"].data_ptr())
        k = 1
        while "rrec%d" % k in t:
            _check(lib().glia_hmt_rag_add_channel(ctx.h, h, t["rrec%d" % k].data_ptr(), t["prec%d" % k].data_ptr()))
            k += 1
        return RegionMap._wrap(h)._configure(ctx, like.cfg)

    def last_pass(self):
        return tuple(_outs(lib().glia_hmt_rag_last_pass, (C.c_double, C.c_double), self.h))

    def regions(self):
        n = self.num_regions
        out = dict(label=np.empty(n, np.uint32), count=np.empty(n, np.int64), border=np.empty(n, np.int64),
                   lo=np.empty((n, 3), np.int64), hi=np.empty((n, 3), np.int64), sum=np.empty(n), sumsq=np.empty(n),
                   min=np.empty(n), max=np.empty(n), hist=np.empty((n, self.bins), np.int64),
                   first=np.empty(n, np.int64))
        _check(lib().glia_hmt_rag_export_regions(self.h, *[_np(out[k]) for k in (
            "label", "count", "border", "lo", "hi", "sum", "sumsq", "min", "max", "hist", "first")]))
        return out

    def pairs(self):
        n = self.num_pairs
        out = dict(a=np.empty(n, np.uint32), b=np.empty(n, np.uint32), count=np.empty(n, np.int64), sum=np.empty(n),
                   sumsq=np.empty(n), min=np.empty(n), max=np.empty(n), hist=np.empty((n, self.bins), np.int64),
                   thr=np.empty((n, max(self.nthr, 1)), np.int64))
        _check(lib().glia_hmt_rag_export_pairs(self.h, *[_np(out[k]) for k in (
            "a", "b", "count", "sum", "sumsq", "min", "max", "hist")], _np(out["thr"]) if self.nthr else None))
        return out

    def merge_order_pb(self, type=1):
        """hmt/main_merge_order_pb.cxx: type 1 = median, 2 = mean.  Returns (order[n,3] uint32, saliency[n])."""
        cap = max(self.num_regions, 1)
        order = np.empty((cap, 3), np.uint32)
        sal = np.empty(cap, np.float64)
        n, = _outs(lib().glia_hmt_merge_order_pb, (C.c_int64,), self.ctx.h, self.h, type, _np(order), _np(sal), cap)
        return order[:n].copy(), sal[:n].copy()

    def feat_dim(self):
        return lib().glia_hmt_feat_dim(self.h)

    def merge_order_bc(self, classifier, want_feats=False):
        """hmt/main_merge_order_bc.cxx: --bct 1 with a RandomForest, --bct 2 with an MLP (its probability is the saliency; hidden
        layers up to mlp_loop_limits()).  Returns (order, saliency[, feats]); feats are the raw rows."""
        cap = max(self.num_regions, 1)
        order = np.empty((cap, 3), np.uint32)
        sal = np.empty(cap, np.float64)
        d = self.feat_dim()
        feats = np.empty((cap, d), np.float64) if want_feats else None
        fn = lib().glia_hmt_merge_order_bc_mlp if isinstance(classifier, MLP) else lib().glia_hmt_merge_order_bc
        n, = _outs(fn, (C.c_int64,), self.ctx.h, self.h, classifier.h, _np(order), _np(sal), _np(feats), cap)
        if want_feats:
            return order[:n].copy(), sal[:n].copy(), feats[:n].copy()
        return order[:n].copy(), sal[:n].copy()

    def pre_merge(self, size_thresholds, rpb_threshold):
        """gadget/main_pre_merge.cxx: pb-mean merges restricted by the region-size condition."""
        cap = max(self.num_regions, 1)
        order = np.empty((cap, 3), np.uint32)
        sal = np.empty(cap, np.float64)
        st = (C.c_int * len(size_thresholds))(*size_thresholds)
        n, = _outs(lib().glia_hmt_pre_merge, (C.c_int64,), self.ctx.h, self.h, st, len(size_thresholds), rpb_threshold, _np(order), _np(sal), cap)
        return order[:n].copy(), sal[:n].copy()

    def _bc_feat(self, fn, order, saliencies, init_sal, sal_bias):
        order = np.ascontiguousarray(order, dtype=np.uint32)
        d = lib().glia_hmt_bc_feat_dim(self.h, 1 if saliencies is not None else 0)
        feats = np.empty((len(order), d), np.float64)
        sal = None if saliencies is None else np.ascontiguousarray(saliencies, dtype=np.float64)
        _check(fn(self.ctx.h, self.h, _np(order), len(order), _np(sal), init_sal, sal_bias, _np(feats)))
        return feats

    def bc_feat(self, order, saliencies=None, init_sal=1.0, sal_bias=1.0):
        """hmt/main_bc_feat.cxx: feature rows of a given merge order; with `saliencies` (-y) also the saliency features."""
        return self._bc_feat(lib().glia_hmt_bc_feat_saliency, order, saliencies, init_sal, sal_bias)

    def bc_feat_batch(self, order, saliencies=None, init_sal=1.0, sal_bias=1.0):
        """the rows of bc_feat by the batch route (hmt/main_bc_feat.cxx:59-95 is parallel over merges too): every set of the known
        merge tree at once instead of a replay of the order; same arguments, row width and errors"""
        return self._bc_feat(lib().glia_hmt_bc_feat_batch, order, saliencies, init_sal, sal_bias)

    BC_FEAT_ROUTES = ("replay", "batch")

    def last_bc_feat_timing(self):
        """stages of the last bc_feat / bc_feat_batch call: ms_plan (host), ms_sets, ms_rows (device), height, launches,
        path_updates, route ("replay" | "batch")"""
        out = _struct_out(lib().glia_hmt_last_bc_feat_timing, BcFeatTiming, self.h)
        out["route"] = self.BC_FEAT_ROUTES[out["route"]]
        return out

    BC_METRICS = {"f1": 0, "ri": 1, "vi": 2}

    def bc_label(self, truths, order, metric="f1", tweak=False, mpd=1.0, opt_split=False, opt=0):
        """hmt/main_bc_label_ri.cxx (metric "f1" / "ri": --f1, --tweak, --mpd, --optSplit, --opt) and main_bc_label_vi.cxx
        (metric "vi", one or more truths: --opt): int32 label per merge, -1 merge / +1 split.  truths: one CUDA u32 tensor of the
        map's shape or a list of them; the map needs only_contour=False and its mask is the tools' -n / -m."""
        if not isinstance(truths, (list, tuple)):
            truths = [truths]
        for t in truths:
            assert t.is_cuda and t.is_contiguous() and t.element_size() == 4
            _fence(t)
        order = np.ascontiguousarray(order, dtype=np.uint32).reshape(-1, 3)
        ptrs = (C.c_void_p * max(len(truths), 1))(*[t.data_ptr() for t in truths])
        opts = BcLabelOpts(self.BC_METRICS[metric], int(bool(tweak)), float(mpd), int(bool(opt_split)), int(opt))
        out = np.empty(max(len(order), 1), np.int32)
        _check(lib().glia_hmt_bc_label(self.ctx.h, self.h, ptrs, len(truths), _np(order), len(order), C.byref(opts), _np(out)))
        return out[:len(order)].copy()

    def last_bc_label_timing(self):
        """stages of the last bc_label call: ms_count (device), ms_nodes, ms_rules (host), entries, moves, node_pairs"""
        return _struct_out(lib().glia_hmt_last_bc_label_timing, BcLabelTiming, self.h)

    def score_initial_edges(self, classifier):
        """features + scores of the initial table edges (TBoundaryTable::init) -> (edges scored, device ms).  With
        use_median_features the medians come from sorted value runs of every leaf and directed pair (whole-volume maps only)."""
        return tuple(_outs(lib().glia_hmt_score_initial_edges, (C.c_int64, C.c_double), self.ctx.h, self.h, classifier.h))

    def score_initial_edges_shard(self, classifier, shard, n_shards):
        """scores of the initial records e with e % n_shards == shard (-inf elsewhere); max over shards = all scores.  Works with
        use_median_features as well (whole-volume maps; merge_order_bc still refuses that layout) -- with a forest; an MLP takes the
        statistics layout only."""
        cap = max(self.num_pairs, 1)
        out = np.empty(cap, np.float64)
        fn = lib().glia_hmt_score_initial_edges_shard_mlp if isinstance(classifier, MLP) else lib().glia_hmt_score_initial_edges_shard
        n, = _outs(fn, (C.c_int64,), self.ctx.h, self.h, classifier.h, shard, n_shards, _np(out), cap)
        return out[:n].copy()

    def boundary_confidence(self, trees):
        """segment_greedy -b (genBoundaryConfidenceImage, all nodes): float32 CUDA tensor of the volume's shape"""
        import torch
        nt = len(trees)
        keep = [[np.ascontiguousarray(t[0], np.uint32), np.ascontiguousarray(t[1], np.int32), np.ascontiguousarray(t[2], np.int32),
                 np.ascontiguousarray(t[4], np.float64)] for t in trees]
        nn = (C.c_int64 * nt)(*[len(k[0]) for k in keep])
        arr = lambda j: (C.c_void_p * nt)(*[k[j].ctypes.data for k in keep])
        out = torch.empty(self.shape, dtype=torch.float32, device=torch.device("cuda", self.ctx.device))
        _check(lib().glia_hmt_boundary_confidence(self.ctx.h, self.h, nt, nn, arr(0), arr(1), arr(2), arr(3), out.data_ptr()))
        return out

    def last_merge_timing(self):
        return dict(zip(("ms_table", "ms_init", "ms_loop", "n_edges_scored"),
                        _outs(lib().glia_hmt_last_merge_timing, (C.c_double, C.c_double, C.c_double, C.c_int64), self.h)))
