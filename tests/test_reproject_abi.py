"""Temporal reprojection at the C boundary, without a device: the five entry points are exported and have ctypes signatures, the
two structs and the option's number match the header as a C compiler lays them out, the Rust declarations list the same
arguments, and the argument checks that need no context answer as the header says.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd._lib import ADDED_WITHIN_ABI_5, SIGNATURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptrace.h")
NAMES = ("pt_keep_history", "pt_load_history", "pt_reproject", "pt_reproject_stats", "pt_reproject_constants")


def test_symbols_and_signatures(lib):
    for name in NAMES:
        assert hasattr(lib, name) and name in SIGNATURES and name in ADDED_WITHIN_ABI_5, name
    assert lib.pt_abi_version() == 5   # added within the version, as the last five features were


def test_structs_and_constants_match_the_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "ptrace.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %d\n", sizeof(PtReprojectOptions), sizeof(PtReprojectStats), offsetof(PtReprojectOptions, tolerance_px),
   offsetof(PtReprojectStats, pixels_kept), offsetof(PtReprojectStats, samples_kept), (int)PT_OPT_REPROJECT);
 printf("%.9g %.9g %.9g\n", (double)PT_REPROJECT_TOLERANCE_DEFAULT, (double)PT_REPROJECT_CAP_DIFFUSE_DEFAULT, (double)PT_REPROJECT_CAP_OTHER_DEFAULT);
 return 0; }'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        l1, l2 = subprocess.check_output([exe], text=True).strip().split("\n")
    assert [int(x) for x in l1.split()] == [C.sizeof(abi.PtReprojectOptions), C.sizeof(abi.PtReprojectStats),
                                            abi.PtReprojectOptions.tolerance_px.offset, abi.PtReprojectStats.pixels_kept.offset,
                                            abi.PtReprojectStats.samples_kept.offset, abi.PT_OPT_REPROJECT]
    assert C.sizeof(abi.PtReprojectOptions) == 16 and C.sizeof(abi.PtReprojectStats) == 32 and abi.PT_OPT_REPROJECT == 9
    assert [float(x) for x in l2.split()] == [abi.PT_REPROJECT_TOLERANCE_DEFAULT, abi.PT_REPROJECT_CAP_DIFFUSE_DEFAULT,
                                              abi.PT_REPROJECT_CAP_OTHER_DEFAULT]
    opt = abi.PtReprojectOptions()
    assert (opt.cap_diffuse, opt.cap_other, opt.tolerance_px) == (abi.PT_REPROJECT_CAP_DIFFUSE_DEFAULT, abi.PT_REPROJECT_CAP_OTHER_DEFAULT,
                                                                  abi.PT_REPROJECT_TOLERANCE_DEFAULT)


def test_rust_binding_declares_the_same_arguments():
    text = open(os.path.join(ROOT, "bindings", "rust", "ptrace_sys.rs")).read()
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        r = re.search(r"pub fn %s\(([^)]*)\)" % name, text)
        h = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert r and h, name
        assert len([a for a in r.group(1).split(",") if a.strip()]) == len([a for a in h.group(1).split(",") if a.strip()]), name
    for struct, fields in (("PtReprojectOptions", 4), ("PtReprojectStats", 4)):
        body = re.search(r"pub struct %s \{(.*?)\n\}" % struct, text, flags=re.S).group(1)
        assert len(re.findall(r"pub \w+:", body)) == fields, struct
    assert re.search(r"PT_OPT_REPROJECT: c_int = 9", text)


def test_the_header_carries_the_statement_list():
    text = open(HEADER).read()
    for line in ("done if ids.x < 0", "lam = (w.x*N.x + w.y*N.y) + w.z*N.z ;  done unless lam > 0", "lam2 = lam*lam ;  rhs = k * lam2",
                 "skip unless HIDS[q].x == ids.x && HIDS[q].w == ids.w", "nq = cnt / wsum ;  nq = floorf(nq) ;  if (nq > cap) nq = cap ;  done unless nq >= 1",
                 "k = tolerance_px^2 * (Hh.Hh) / width^2", "the planes are pinhole"):
        assert line in text, line


def test_argument_checks_that_need_no_device(lib):
    opt, st, p = abi.PtReprojectOptions(), abi.PtReprojectStats(), abi.PtParams()
    planes = np.zeros(4, np.float32).ctypes.data_as(C.c_void_p)
    assert lib.pt_keep_history(None) == abi.PT_ERR_INVALID
    assert lib.pt_load_history(None, C.byref(p), planes, planes) == abi.PT_ERR_INVALID
    assert lib.pt_reproject(None, C.byref(opt)) == abi.PT_ERR_INVALID
    assert lib.pt_reproject_stats(None, C.byref(st)) == abi.PT_ERR_INVALID
    out = np.zeros(16, np.float32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.pt_reproject_constants(None, 2.0, fp) == abi.PT_ERR_INVALID
    assert lib.pt_reproject_constants(C.byref(p), 2.0, fp) == abi.PT_ERR_INVALID   # an all-zero camera (and width 0)
    assert not out.any()
