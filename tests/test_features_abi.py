"""The first-hit feature planes at the boundary of the library (no GPU needed): the three entry points are exported, the
constants of abi.py are the header's, and a NULL context is refused."""
import ctypes as C
import os
import re
import subprocess

from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd._lib import LIB_PATH, SIGNATURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptrace.h")
NAMES = ("pt_render_features", "pt_features_ptr", "pt_read_features")


def test_the_library_exports_the_three_entry_points(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB_PATH], text=True)
    exported = set(re.findall(r" T (pt_[a-z0-9_]+)", out))
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert name in exported and hasattr(lib, name) and name in SIGNATURES, name
        h = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert h and len([a for a in h.group(1).split(",") if a.strip()]) == len(SIGNATURES[name][1]), name


def test_constants_match_the_header():
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("PT_OPT_FEATURES", "PT_FEAT_ALBEDO", "PT_FEAT_NORMAL", "PT_FEAT_POINT", "PT_FEAT_IDS", "PT_FEAT_PLANES"):
        m = re.search(r"\b%s\s*=\s*(-?\d+)" % name, header)
        assert m, name
        assert int(m.group(1)) == getattr(abi, name), name
    assert (abi.PT_OPT_FEATURES, abi.PT_FEAT_PLANES) == (8, 4)
    assert abi.BUILD_FEATURES == 4
    rust = open(os.path.join(ROOT, "bindings", "rust", "ptrace_sys.rs")).read()
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, rust), name
    assert re.search(r"PT_OPT_FEATURES: c_int = 8;", rust)


def test_a_null_context_is_refused(lib):
    ptr, n = C.c_void_p(), C.c_size_t()
    buf = (C.c_float * 4)()
    assert lib.pt_render_features(None) == abi.PT_ERR_INVALID
    assert lib.pt_features_ptr(None, abi.PT_FEAT_IDS, C.byref(ptr), C.byref(n)) == abi.PT_ERR_INVALID
    assert lib.pt_read_features(None, abi.PT_FEAT_ALBEDO, buf) == abi.PT_ERR_INVALID
