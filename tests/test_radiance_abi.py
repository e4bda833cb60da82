"""Radiance queries at the C boundary, without a device: pt_query_radiance is exported and has a ctypes signature, PtRayRadiance
matches the header as a C compiler lays it out, the Rust declarations list the same arguments and fields, the header states the
contract, and the errors that need no device are raised.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import tempfile

from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd._lib import ADDED_WITHIN_ABI_5, LIB_PATH, SIGNATURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptrace.h")
NAME = "pt_query_radiance"


def test_symbol_and_signature(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB_PATH], text=True)
    exported = set(re.findall(r" T (pt_[a-z0-9_]+)", out))
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert NAME in exported and hasattr(lib, NAME) and NAME in SIGNATURES and NAME in ADDED_WITHIN_ABI_5
    h = re.search(r"\b%s\s*\(([^)]*)\)" % NAME, header)
    assert h and len([a for a in h.group(1).split(",") if a.strip()]) == len(SIGNATURES[NAME][1]) == 5
    assert lib.pt_abi_version() == 5   # added within the version
    # the kernels' accessors stay inside the library
    assert "pt_radiance_kernel" not in exported and "pt_radiance_fold_kernel_handle" not in exported


def test_the_struct_matches_the_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "ptrace.h"
int main(void){
 printf("%zu %zu %zu\n", sizeof(PtRayRadiance), offsetof(PtRayRadiance, sum), offsetof(PtRayRadiance, samples));
 return 0; }'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got == [16, 0, 12] == [C.sizeof(abi.PtRayRadiance), abi.PtRayRadiance.sum.offset, abi.PtRayRadiance.samples.offset]


def test_rust_binding_declares_the_same_arguments_and_fields():
    text = open(os.path.join(ROOT, "bindings", "rust", "ptrace_sys.rs")).read()
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    r = re.search(r"pub fn %s\(([^)]*)\)" % NAME, text)
    h = re.search(r"\b%s\s*\(([^)]*)\)" % NAME, header)
    assert r and h
    assert len([a for a in r.group(1).split(",") if a.strip()]) == len([a for a in h.group(1).split(",") if a.strip()]) == 5
    body = re.search(r"pub struct PtRayRadiance \{(.*?)\n\}", text, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == ["sum", "samples"]


def test_the_header_carries_the_contract():
    text = " ".join(open(HEADER).read().split())
    for phrase in ("u_time = time + float(first_pass + b * n_passes + p) * step", "seed = init_global_seed(vx, vy, u_time)",
                   "NO jitter draw and NO lens draws precede it", "out.samples = out.samples + float(samples_per_pixel)",
                   "rays at the same place of different batches share no random * numbers",
                   "depends on its INDEX in the call and on the context's SIZE", "samples == 0 is the mark",
                   "first_pass is NOT advanced", "at most the passes reserved with pt_reserve_passes",
                   "PtStats.samples, total_spp, render_launches and render_kernel_ms"):
        assert phrase in text, phrase


def test_errors_that_need_no_device(lib):
    rays, out = (abi.PtRay * 2)(), (abi.PtRayRadiance * 2)()
    assert lib.pt_query_radiance(None, rays, 2, 1, out) == abi.PT_ERR_INVALID
    assert lib.pt_query_radiance(None, rays, 0, 1, out) == abi.PT_ERR_INVALID
    assert lib.pt_query_radiance(None, None, 0, 0, None) == abi.PT_ERR_INVALID
    assert not bytes(out).strip(b"\0")
