"""Ray queries at the C boundary, without a device: the two entry points are exported and have ctypes signatures, PtRay and
PtRayHit match the header as a C compiler lays them out (sizes and every field's offset), the constants are the header's, the
Rust declarations list the same arguments and fields, the header states the contract, and a NULL context is refused.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import tempfile

from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd._lib import ADDED_WITHIN_ABI_5, LIB_PATH, SIGNATURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptrace.h")
NAMES = ("pt_query_rays", "pt_query_batch")
RAY_FIELDS = ("origin", "_pad0", "direction", "_pad1")
HIT_FIELDS = ("albedo", "t", "normal", "_pad0", "point", "_pad1", "index", "uuid", "type", "front_face")


def test_symbols_and_signatures(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB_PATH], text=True)
    exported = set(re.findall(r" T (pt_[a-z0-9_]+)", out))
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert name in exported and hasattr(lib, name) and name in SIGNATURES and name in ADDED_WITHIN_ABI_5, name
        h = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert h and len([a for a in h.group(1).split(",") if a.strip()]) == len(SIGNATURES[name][1]), name
    assert lib.pt_abi_version() == 5   # added within the version
    assert SIGNATURES["pt_query_batch"][0] is C.c_uint32
    # the kernels' accessor stays inside the library
    assert "pt_query_kernel" not in exported


def test_structs_and_constants_match_the_header():
    offs = ["offsetof(PtRay, %s)" % f for f in RAY_FIELDS] + ["offsetof(PtRayHit, %s)" % f for f in HIT_FIELDS]
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "ptrace.h"
int main(void){
 size_t v[] = {sizeof(PtRay), sizeof(PtRayHit), %s};
 for (size_t i = 0; i < sizeof v / sizeof v[0]; i++) printf("%%zu ", v[i]);
 printf("\n%%d %%d\n", (int)PT_OPT_RAY_QUERIES, (int)PT_RAY_INVALID);
 return 0; }''' % ", ".join(offs)
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        l1, l2 = subprocess.check_output([exe], text=True).strip().split("\n")
    got = [int(x) for x in l1.split()]
    assert got[:2] == [32, 64] == [C.sizeof(abi.PtRay), C.sizeof(abi.PtRayHit)]
    assert got[2:6] == [0, 12, 16, 28] == [getattr(abi.PtRay, f).offset for f in RAY_FIELDS]
    assert got[6:] == [0, 12, 16, 28, 32, 44, 48, 52, 56, 60] == [getattr(abi.PtRayHit, f).offset for f in HIT_FIELDS]
    assert [int(x) for x in l2.split()] == [abi.PT_OPT_RAY_QUERIES, abi.PT_RAY_INVALID] == [10, -2]


def test_rust_binding_declares_the_same_arguments_and_fields():
    text = open(os.path.join(ROOT, "bindings", "rust", "ptrace_sys.rs")).read()
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        r = re.search(r"pub fn %s\(([^)]*)\)" % name, text)
        h = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert r and h, name
        assert len([a for a in r.group(1).split(",") if a.strip()]) == len([a for a in h.group(1).split(",") if a.strip()]), name
    for struct, fields in (("PtRay", len(RAY_FIELDS)), ("PtRayHit", len(HIT_FIELDS))):
        body = re.search(r"pub struct %s \{(.*?)\n\}" % struct, text, flags=re.S).group(1)
        assert len(re.findall(r"pub \w+:", body)) == fields, struct
    assert re.search(r"PT_OPT_RAY_QUERIES: c_int = 10;", text) and re.search(r"PT_RAY_INVALID: i32 = -2;", text)


def test_the_header_carries_the_contract():
    text = " ".join(open(HEADER).read().split())
    for phrase in ("is the feature record of pt_render_features above, field for field",   # by reference, not a copy of the table
                   "a ray with a non-finite component (NaN, +inf, -inf) in origin or direction, or whose three direction components * are all +0 or -0, is invalid",
                   "{PT_RAY_INVALID, PT_RAY_INVALID, PT_RAY_INVALID, 0}", "ties go to the later sphere", "a band that owns no rows",
                   "PT_ERR_CAPACITY: the * planes are not in place after a failed allocation", "pt_last_trace_build"):
        assert phrase in text, phrase
    assert text.count("PT_FEAT_ALBEDO 0 {albedo.r") == 1  # the table stands once


def test_a_null_context_is_refused(lib):
    rays, hits = (abi.PtRay * 2)(), (abi.PtRayHit * 2)()
    assert lib.pt_query_rays(None, rays, 2, hits) == abi.PT_ERR_INVALID
    assert lib.pt_query_rays(None, rays, 0, hits) == abi.PT_ERR_INVALID
    assert lib.pt_query_rays(None, None, 0, None) == abi.PT_ERR_INVALID
    assert lib.pt_query_batch(None) == 0
    assert not bytes(hits).strip(b"\0")
