"""Host side of the batch bc_feat route, no GPU: the C ABI exports the new entry points, the option key is known, NULL arguments
come back as GLIA_HMT_ERR_ARG with the replay's message, and the ctypes mirror of the timing struct has the header's layout."""
import ctypes as C
import os
import re

from glia_amd import hmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_and_option_key():
    L = hmt.lib()
    for name in ("glia_hmt_bc_feat_batch", "glia_hmt_last_bc_feat_timing"):
        assert hasattr(L, name), name
    hmt.set_option("GLIA_HMT_BCFEAT", "batch")                   # a known key (an unknown one raises)
    hmt.set_option("GLIA_HMT_BCFEAT", None)
    for args in ((None, None, None, C.c_int64(0), None, C.c_double(1.0), C.c_double(1.0), None),):
        errs = []
        for fn in (L.glia_hmt_bc_feat_saliency, L.glia_hmt_bc_feat_batch):
            errs.append((fn(*args), L.glia_hmt_last_error().decode()))
        assert errs[0] == errs[1] == (hmt.ERR_ARG, "bc_feat: invalid argument")
    assert L.glia_hmt_last_bc_feat_timing(None, None) == hmt.ERR_ARG


def test_timing_struct_mirrors_the_header():
    text = open(os.path.join(ROOT, "include", "glia_hmt.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} glia_hmt_bc_feat_timing;", text).group(1)
    fields = re.findall(r"^\s*(double|int64_t|int)\s+(\w+);", body, re.M)
    ctype = {"double": C.c_double, "int64_t": C.c_int64, "int": C.c_int}
    assert [(n, ctype[t]) for t, n in fields] == list(hmt.BcFeatTiming._fields_)
    assert "hmt/main_bc_feat.cxx:59-95" in text and "util/mp.hxx:24-106" in text
    assert hmt.RegionMap.BC_FEAT_ROUTES == ("replay", "batch")
    assert re.search(r"GLIA_HMT_BCFEAT_REPLAY = 0, GLIA_HMT_BCFEAT_BATCH = 1", text)
