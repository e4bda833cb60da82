"""The chunk-bounds arithmetic of the filtered read-out (csrc/pt_error_plan.hpp chunk_rows, the function pt_filter_kernel calls:
a local row -> the first and last local row of its chunk of band_rows image rows) on the CPU, through
tests/filter_plan_shim.cpp, against the restatement's `ly // band_rows` (tests/filter_ref.py chunk_of_rows).  Then the
stand-alone program tests/filter_plan_main.cpp under the address and undefined-behaviour sanitizers.  CPU only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import filter_ref as FR

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(tempfile.mkdtemp(prefix="filter_plan_"), "libfilter_plan_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", os.path.join(HERE, "filter_plan_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.filter_plan_chunk_rows.restype = None
    lib.filter_plan_chunk_rows.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    return lib


def _bounds(shim, ly, band_rows, rows):
    fl = (C.c_uint32 * 2)(0xdeadbeef, 0xdeadbeef)
    shim.filter_plan_chunk_rows(ly, band_rows, rows, fl)
    return fl[0], fl[1]


@pytest.mark.parametrize("band_rows", range(1, 10))
def test_chunk_rows_against_the_restatement_at_every_height_up_to_40(shim, band_rows):
    for rows in range(1, 41):
        chunk = FR.chunk_of_rows(rows, band_rows)
        assert np.array_equal(chunk, np.arange(rows) // band_rows)
        for ly in range(rows):
            same = np.nonzero(chunk == chunk[ly])[0]
            assert _bounds(shim, ly, band_rows, rows) == (same[0], same[-1]), (rows, band_rows, ly)
            assert np.array_equal(same, np.arange(same[0], same[-1] + 1))   # a chunk is a run of consecutive local rows


def test_a_context_that_is_no_band_looks_at_every_row(shim):
    for rows in range(1, 41):
        assert np.all(FR.chunk_of_rows(rows, 0) == 0)
        for ly in range(rows):
            assert _bounds(shim, ly, 0, rows) == (0, rows - 1)


def test_chunk_rows_under_address_and_undefined_behaviour_sanitizers():
    """tests/filter_plan_main.cpp: a stand-alone program (its own main) over chunk_rows, built with -fsanitize=address,undefined
    and run as a child; nothing sanitized is loaded into this process"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "filter_plan_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(HERE, "filter_plan_main.cpp"), "-o", exe])
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and "filter plan: ok" in out.stdout, out.stdout[-2000:]
