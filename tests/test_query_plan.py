"""The arithmetic of pt_query_rays (csrc/pt_query.hpp: batch splitting, the tile rows a batch covers, pack, unpack, the
sentinel, the validity predicate) on the CPU, through tests/query_plan_shim.cpp, against plain Python and tests/query_ref.py.
Then the stand-alone program tests/query_main.cpp under the address and undefined-behaviour sanitizers.  CPU only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import query_ref as Q
from ray_tracer_webgl_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(37, 21), (8, 8), (9, 1), (1920, 1080)]


def counts(w, r):
    return [1, 63, 64, 65, w * r - 1, w * r, w * r + 1, 2 * w * r + 5]


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(tempfile.mkdtemp(prefix="query_plan_"), "libquery_plan_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", os.path.join(HERE, "query_plan_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    u32 = C.c_uint32
    for name, args in (("query_n_batches", [u32, u32]), ("query_batch_rays", [u32, u32, u32]), ("query_tile_rows_covered", [u32, u32]),
                       ("query_tiles_covered", [u32, u32]), ("query_sizeof_ray", []), ("query_sizeof_hit", [])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = u32, args
    fp = C.POINTER(C.c_float)
    lib.query_ray_valid.restype, lib.query_ray_valid.argtypes = C.c_int, [fp, fp]
    lib.query_pack.restype, lib.query_pack.argtypes = None, [C.c_void_p, u32, C.c_void_p, u32]
    lib.query_unpack.restype, lib.query_unpack.argtypes = None, [C.c_void_p, u32, u32, C.c_void_p]
    lib.query_invalid.restype, lib.query_invalid.argtypes = None, [C.c_void_p, u32, u32]
    return lib


CASES = [(w, r, n) for w, r in SHAPES for n in counts(w, r)]


@pytest.mark.parametrize("w,r,n", CASES, ids=["%dx%d-n%d" % c for c in CASES])
def test_batches_and_covered_tile_rows(shim, w, r, n):
    assert len(CASES) == 32
    assert n >= 1
    batch = w * r
    nb = shim.query_n_batches(n, batch)
    assert nb == -(-n // batch)
    sizes = [shim.query_batch_rays(n, batch, k) for k in range(nb)]
    assert sum(sizes) == n and all(s == batch for s in sizes[:-1]) and 1 <= sizes[-1] <= batch
    tiles_x, tiles_y = (w + 7) // 8, (r + 7) // 8
    for m in set(sizes):
        rows = -(-m // w)            # ray i is local pixel i: the rows the rays occupy
        tile_rows = -(-rows // 8)    # ... and the rows of 8x8 tiles those lie in
        assert shim.query_tile_rows_covered(m, w) == tile_rows <= tiles_y
        assert shim.query_tiles_covered(m, w) == tile_rows * tiles_x
        # every ray's tile is among the first tile_rows * tiles_x of the identity order, and the last ray's tile row is the last one
        last = m - 1
        assert ((last // w) // 8) == tile_rows - 1
    if n == 1:
        assert shim.query_tiles_covered(1, w) == tiles_x  # one ray: one tile row, not a frame


def test_the_records_sizes(shim):
    assert shim.query_sizeof_ray() == C.sizeof(abi.PtRay) == 32 and shim.query_sizeof_hit() == C.sizeof(abi.PtRayHit) == 64 == Q.HIT_DTYPE.itemsize


@pytest.mark.parametrize("plane,m", [(1, 1), (64, 63), (65, 65), (777, 200)])
def test_pack_and_unpack_round_trip(shim, plane, m):
    rng = np.random.default_rng(2310 + plane)
    rays = rng.standard_normal((m, 8)).astype(np.float32)
    planes = np.full((4, plane, 4), -7.0, np.float32)
    shim.query_pack(rays.ctypes.data, m, planes.ctypes.data, plane)
    assert np.array_equal(planes[abi.PT_FEAT_POINT, :m, :3], rays[:, 0:3]) and np.array_equal(planes[abi.PT_FEAT_NORMAL, :m, :3], rays[:, 4:7])
    assert not planes[abi.PT_FEAT_POINT, :m, 3].view(np.uint32).any() and not planes[abi.PT_FEAT_NORMAL, :m, 3].view(np.uint32).any()
    assert (planes[abi.PT_FEAT_POINT, m:] == -7).all() and (planes[abi.PT_FEAT_NORMAL, m:] == -7).all()
    assert (planes[abi.PT_FEAT_ALBEDO] == -7).all() and (planes[abi.PT_FEAT_IDS] == -7).all()
    # records: random bits in every plane come out as the four texels side by side
    bits = rng.integers(0, 2 ** 32, (4, plane, 4), dtype=np.uint64).astype(np.uint32)
    hits = np.zeros((m + 1, 16), np.uint32)
    hits[m] = 0xa5a5a5a5
    shim.query_unpack(bits.ctypes.data, plane, m, hits.ctypes.data)
    assert np.array_equal(hits[:m], np.concatenate([bits[k, :m] for k in range(4)], axis=1))
    assert (hits[m] == 0xa5a5a5a5).all()
    rec = hits[:m].view(Q.HIT_DTYPE).reshape(m)
    assert np.array_equal(rec["t"].view(np.uint32), bits[0, :m, 3]) and np.array_equal(rec["uuid"].view(np.uint32), bits[3, :m, 1])


def test_the_sentinel_texels(shim):
    planes = np.full((4, 5, 4), -7.0, np.float32)
    shim.query_invalid(planes.ctypes.data, 5, 3)
    u = planes.view(np.uint32)
    got = np.concatenate([u[k, 3] for k in range(4)])
    want = np.zeros(16, np.uint32)
    want[12:15] = 0xfffffffe
    assert np.array_equal(got, want) and (np.delete(planes, 3, axis=1) == -7).all()


def test_the_predicate_against_the_numpy_one(shim):
    fp = C.POINTER(C.c_float)
    o, d = Q.invalid_rays()
    more_o = np.float32([[0, 0, 0], [0, 0, 0], [3e38, 0, 0], [2e15, 1, 1], [0, 0, 0], [0, 0, 0], [1, 1, 1]])
    more_d = np.float32([[0, -0.0, -1], [1e-45, 0, 0], [0, 0, -1], [1, 0, 0], [3.2e-7, 0, 0], [3200, 0, 0], [-0.0, -0.0, -0.0]])
    o, d = np.concatenate([o, more_o]), np.concatenate([d, more_d])
    want = Q.valid(o, d)
    assert list(want[-7:]) == [True] * 6 + [False] and not want[:19].any()
    for k in range(len(o)):
        ok, dk = np.ascontiguousarray(o[k]), np.ascontiguousarray(d[k])
        assert bool(shim.query_ray_valid(ok.ctypes.data_as(fp), dk.ctypes.data_as(fp))) == bool(want[k]), (k, o[k], d[k])


def test_query_arithmetic_under_address_and_undefined_behaviour_sanitizers():
    """tests/query_main.cpp: a stand-alone program (its own main) over pack, unpack, split and the predicate, built with
    -fsanitize=address,undefined and run as a child; nothing sanitized is loaded into this process"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "query_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(HERE, "query_main.cpp"), "-o", exe])
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and "query plan: ok" in out.stdout, out.stdout[-2000:]
