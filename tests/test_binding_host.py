"""The Python binding held to include/glia_hmt.h (no GPU): the prototype table of glia_amd/_abi.py equals what the header declares,
hmt.lib() installs exactly that table, glia_amd/hmt.py calls nothing outside it, and every ctypes.Structure / NumPy dtype that
re-states a struct of the header has the header's layout.  A new entry point needs the header and a table entry; a new struct needs
the header, a mirror in hmt.py and a line in MIRRORS below -- this test says which of them is missing."""
import ctypes as C
import glob
import inspect
import os
import re

import numpy as np

from glia_amd import _abi, hmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "glia_hmt.h")).read()

# the mapping from C to ctypes, stated once: any object pointer is a c_void_p (it takes None, an int, byref(), an array, a pointer),
# `const char*` alone is a c_char_p, scalars map by width
SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "unsigned long long": C.c_uint64, "double": C.c_double, "void": None}
STRING = "char*"

# header struct -> its mirror in glia_amd.hmt (a Structure class or a dtype)
MIRRORS = {
    "glia_hmt_image": "Image", "glia_hmt_feat_config": "FeatConfig", "glia_hmt_slab": "Slab", "glia_hmt_dist_stats": "DistStats",
    "glia_hmt_train_opts": "TrainOpts", "glia_hmt_forest_train_timing": "ForestTrainTiming", "glia_hmt_oob_opts": "OobOpts",
    "glia_hmt_forest_oob_timing": "ForestOobTiming", "glia_hmt_mlp_train_opts": "MLPTrainOpts",
    "glia_hmt_mlp_train_record": "MLP_TRAIN_RECORD", "glia_hmt_mlp_train_timing": "MLPTrainTiming",
    "glia_hmt_sshmt_block": "SSHMTBlock", "glia_hmt_sshmt_train_opts": "SSHMTTrainOpts",
    "glia_hmt_sshmt_train_timing": "SSHMTTrainTiming", "glia_hmt_batch_opts": "BatchOpts", "glia_hmt_batch_timing": "BatchTiming",
    "glia_hmt_bc_feat_timing": "BcFeatTiming", "glia_hmt_bc_label_opts": "BcLabelOpts", "glia_hmt_bc_label_timing": "BcLabelTiming",
    "glia_hmt_overlap_entry": "OVERLAP_ENTRY", "glia_hmt_eval_result": "EvalResult", "glia_hmt_eval_timing": "EvalTiming",
}
NOT_MIRRORED = []      # header structs Python deliberately does not re-state


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def map_type(ctype, structs=None):
    """C type as the header writes it -> ctypes type (None for void), by the mapping above"""
    t = " ".join(re.sub(r"\s*\*\s*", "*", re.sub(r"\bconst\b", "", ctype)).split())
    if t.endswith("*"):
        return C.c_char_p if t == STRING else C.c_void_p
    if structs is not None and t in structs:
        return structs[t]
    return SCALARS[t]


def parse_prototypes(text):
    """{function: (result C type, [parameter C types])} of every function the header declares; array parameters decay to pointers"""
    text = strip_comments(text)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    text = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    text = re.sub(r"enum\s*\{.*?\}\s*;", "", text, flags=re.S)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)
    out = {}
    for stmt in text.split(";"):
        m = re.match(r"^\s*([\w\s\*]+?)\s*\b(glia_hmt_\w+)\s*\((.*)\)\s*$", stmt, re.S)
        if not m:
            continue
        params = []
        for p in m.group(3).split(","):
            p = " ".join(p.split())
            if p == "void":
                continue
            pm = re.match(r"^(.+?)\s*\b(\w+)\s*(\[\w*\])?$", p)
            params.append(pm.group(1) + ("*" if pm.group(3) else ""))
        out[m.group(2)] = (" ".join(m.group(1).split()), params)
    return out


def parse_structs(text):
    """{struct: [(C type, field, array length or None)]} of every `typedef struct { ... } name;`, in the header's order; array lengths
    are resolved through the header's own #define constants"""
    text = strip_comments(text)
    consts = {k: int(v) for k, v in re.findall(r"^\s*#define\s+(\w+)\s+(\d+)\s*$", text, re.M)}
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(glia_hmt_\w+)\s*;", text, re.S):
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            first, *more = [d.strip() for d in decl.split(",")]
            m = re.match(r"^(.+?)\s*\b(\w+)\s*(?:\[(\w+)\])?$", first)
            ctype = m.group(1)
            items = [(m.group(2), m.group(3))] + [re.match(r"^(\w+)\s*(?:\[(\w+)\])?$", d).groups() for d in more]
            for field, length in items:
                fields.append((ctype, field, None if length is None else consts[length] if length in consts else int(length)))
        out[name] = fields
    return out


def build_structs(text):
    """{struct: ctypes.Structure built from the header's fields}, nested structs resolved"""
    built = {}
    for name, fields in parse_structs(text).items():
        members = []
        for ctype, field, length in fields:
            t = map_type(ctype, built)
            members.append((field, t if length is None else t * length))
        built[name] = type(name, (C.Structure,), {"_fields_": members})
    return built


def layout(mirror):
    """[(field, offset, size)] and the total size of a Structure class or a structured dtype"""
    if isinstance(mirror, np.dtype):
        return [(k, mirror.fields[k][1], mirror.fields[k][0].itemsize) for k in mirror.names], mirror.itemsize
    return [(k, getattr(mirror, k).offset, getattr(mirror, k).size) for k, *_ in mirror._fields_], C.sizeof(mirror)


def drifted_structs(text):
    """the header structs whose mirror in hmt does not have their layout"""
    return sorted(name for name, s in build_structs(text).items() if name in MIRRORS and layout(s) != layout(getattr(hmt, MIRRORS[name])))


def drifted_prototypes(text, table):
    """the functions that the header declares and the table lacks, or the reverse, or whose types differ"""
    declared = {name: (map_type(res), tuple(map_type(p) for p in params)) for name, (res, params) in parse_prototypes(text).items()}
    return sorted(name for name in set(declared) | set(table) if declared.get(name) != table.get(name))


def test_table_equals_the_header():
    declared = parse_prototypes(HEADER)
    assert set(declared) == set(re.findall(r"\b(glia_hmt_[a-z_0-9]+)\s*\(", HEADER)), "a prototype the parser cannot read"
    assert len(declared) >= 145
    assert sorted(set(declared) - set(_abi.PROTOTYPES)) == [], "declared in the header, no table entry"
    assert sorted(set(_abi.PROTOTYPES) - set(declared)) == [], "in the table, not in the header"
    assert drifted_prototypes(HEADER, _abi.PROTOTYPES) == []


def test_table_is_installed_once():
    L = hmt.lib()
    for name, (res, params) in _abi.PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is res and tuple(f.argtypes) == tuple(params), name


def test_binding_calls_only_table_entries_and_declares_no_prototype_elsewhere():
    used = set(re.findall(r"glia_hmt_\w+", open(os.path.join(ROOT, "glia_amd", "hmt.py")).read()))
    types = set(re.findall(r"\b(glia_hmt_\w+)\s*;", strip_comments(HEADER)))      # struct and handle types, which docstrings name
    assert len(used) >= 100 and sorted(used - set(_abi.PROTOTYPES) - types) == []
    assignment = r"\.(?:restype|argtypes)\s*=(?!=)"
    installer = inspect.getsource(hmt.lib)
    assert len(re.findall(assignment, installer)) == 2
    for path in glob.glob(os.path.join(ROOT, "glia_amd", "*.py")):
        assert not re.search(assignment, open(path).read().replace(installer, "")), path


def test_struct_mirrors_have_the_headers_layout():
    structs = build_structs(HEADER)
    assert len(structs) >= 22
    assert sorted(set(structs) - set(MIRRORS) - set(NOT_MIRRORED)) == [], "a header struct without a mirror"
    assert sorted(set(MIRRORS) - set(structs)) == [] and NOT_MIRRORED == []
    assert len(set(MIRRORS.values())) == len(MIRRORS)
    mirrors = {k for k, v in vars(hmt).items() if isinstance(v, np.dtype) or (isinstance(v, type) and issubclass(v, C.Structure))}
    assert sorted(mirrors ^ set(MIRRORS.values())) == [], "a mirror in hmt that no header struct is tied to"
    for name, s in structs.items():
        assert layout(s) == layout(getattr(hmt, MIRRORS[name])), name
    assert drifted_structs(HEADER) == []
    for k, n in (("GLIA_HMT_MAX_IMAGES", hmt.MAX_IMAGES), ("GLIA_HMT_MAX_BINS", hmt.MAX_BINS), ("GLIA_HMT_MAX_THRESH", hmt.MAX_THRESH)):
        assert re.search(r"#define %s %d$" % (k, n), HEADER, re.M)


def test_a_drifted_header_is_reported():
    """the two comparers above on a header that is one type away from the binding: each names exactly what drifted"""
    field = "int64_t height;"
    assert HEADER.count(field) == 1
    assert drifted_structs(HEADER.replace(field, "int height;")) == ["glia_hmt_bc_feat_timing"]
    param = "int64_t expected_regions"
    assert HEADER.count(param) == 1
    assert drifted_prototypes(HEADER.replace(param, "int expected_regions"), _abi.PROTOTYPES) == ["glia_hmt_ctx_set_table_hint"]
    assert drifted_structs(HEADER.replace("#define GLIA_HMT_MAX_THRESH 4", "#define GLIA_HMT_MAX_THRESH 5")) == ["glia_hmt_feat_config"]
