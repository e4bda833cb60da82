"""What pt_set_spheres derives from a sphere list on the host (csrc/pt_scene_image.hpp), on the CPU.

The library, its host exports (pt_build_grid, pt_build_bvh, pt_grid_walk_constants) and the other tests' shims all call the one
`split`; `per_slot` makes the per-slot materials of both culling structures and the debug overlay's per-slot uuids; `build_grid`
decides in which layout a grid is uploaded.  Checked through a shim compiled from the header itself (g++ -ffp-contract=off,
like the library):

  (a) split: the padded length is PT_LDS_ENTRIES(n) of csrc/pt_kernel_args.h (asked of the shim, not restated) and every padding
      record has the bits of {1e15f, 1e15f, 1e15f, 0}, at the list lengths around the padding's steps;
  (b) split: r*r, 1 / ri and both r0 values are numpy float32's, the same operation sequence, compared as uint32 bits (a NaN
      compares equal by bits) — on random spheres and on refraction indices 1, 1.5, a denormal and 0 (-> inf, then NaN in r0);
  (c) regular: false for a NaN centre, an infinite radius and a coordinate of exactly 1e15f, true one float below;
  (d) per_slot: an index that names no sphere (0xffffffff, n_src itself) gives a zeroed element, for both element types;
  (e) build_grid: a grid that fits the LDS beside its entries keeps pt_build_grid's layout, one that does not gets
      pt_build_grid_runs' — the decision that so far only whole-frame GPU tests exercised.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from ray_tracer_webgl_amd import _lib, abi, scenes
from test_grid import build as class_build

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_SRC = os.path.join(HERE, "scene_image_shim.cpp")
MAT_DTYPE = np.dtype([("albedo", "<f4", 3), ("fuzz", "<f4"), ("refraction_index", "<f4"), ("type", "<i4"), ("radius", "<f4"),
                      ("inv_ri", "<f4")])  # PtMatRec, csrc/pt_kernel_args.h
assert MAT_DTYPE.itemsize == 32
EDGE_SIZES = [0, 1, 7, 8, 9, 16, 17]
_LIB = []


def shim():
    if not _LIB:
        so = os.path.join(tempfile.mkdtemp(prefix="scene_image_"), "libscene_image_shim.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", SHIM_SRC, "-o", so])
        lib = C.CDLL(so)
        u32, vp, sz, sph = C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(abi.PtSphere)
        for name, res, args in (("scene_lds_entries", u32, [u32]),
                                ("scene_split", C.c_int, [sph, u32, vp, vp, sz, vp, sz, vp, sz, vp, sz, vp, sz]),
                                ("scene_per_slot_mat", None, [vp, sz, vp, sz, vp]), ("scene_per_slot_i32", None, [vp, sz, vp, sz, vp]),
                                ("scene_build_grid", C.c_int, [sph, u32, C.c_double, vp, vp, sz, vp, sz, vp, sz])):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _LIB.append(lib)
    return _LIB[0]


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def split(spheres):
    lib = shim()
    ptr, n, keep = abi.spheres_as_ctypes(spheres)
    sizes = np.zeros(5, np.uintp)
    regular = lib.scene_split(ptr, n, _vp(sizes), None, 0, None, 0, None, 0, None, 0, None, 0)
    out = dict(geom=np.zeros(sizes[0], np.float32), mat=np.zeros(sizes[1], MAT_DTYPE), radii=np.zeros(sizes[2], np.float32),
               r0=np.zeros(sizes[3], np.float32), uuid=np.zeros(sizes[4], np.int32))
    args = []
    for k in ("geom", "mat", "radii", "r0", "uuid"):
        args += [_vp(out[k]), out[k].size]
    assert lib.scene_split(ptr, n, _vp(sizes), *args) == regular
    out["geom"] = out["geom"].reshape(-1, 4)
    out["r0"] = out["r0"].reshape(-1, 2)
    out["regular"] = bool(regular)
    return out


def random_spheres(n, seed):
    rng = np.random.default_rng(seed)
    s = np.zeros(n, abi.SPHERE_DTYPE)
    s["center"] = rng.uniform(-50, 50, (n, 3))
    s["radius"] = rng.uniform(0.05, 40.0, n) * rng.choice([1.0, -1.0], n, p=[0.9, 0.1])
    s["type"] = rng.integers(0, 5, n)
    s["albedo"] = rng.uniform(0, 1, (n, 3))
    s["fuzz"] = rng.uniform(0, 1, n)
    s["refraction_index"] = rng.choice([1.5, 1.33, 2.4, 0.8], n) * rng.uniform(0.5, 2.0, n)
    s["uuid"] = rng.permutation(n) * 7 + 100
    return s


# ---- (a) the padding ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_split_pads_the_geometry_to_the_staged_length(n):
    s = random_spheres(n, 100 + n)
    sp = split(s)
    n_pad = shim().scene_lds_entries(n)
    assert n_pad >= n + 4 and n_pad % 4 == 0  # (a prefetch group always follows the list)
    assert sp["geom"].shape == (n_pad, 4)
    assert len(sp["mat"]) == len(sp["radii"]) == len(sp["uuid"]) == len(sp["r0"]) == n
    pad = np.array([1e15, 1e15, 1e15, 0.0], np.float32)
    assert np.array_equal(u32(sp["geom"][n:]), np.broadcast_to(u32(pad), (n_pad - n, 4)))
    assert np.array_equal(u32(sp["geom"][:n, :3]), u32(s["center"]))
    assert sp["regular"]


# ---- (b) the arithmetic ---------------------------------------------------------------------------------------------
def test_split_arithmetic_is_float32_operation_by_operation():
    s = random_spheres(300, 7)
    denormal = np.float32(1e-40)
    assert 0.0 < float(denormal) < float(np.finfo(np.float32).tiny)
    special = np.array([1.0, 1.5, denormal, 0.0], np.float32)
    s["refraction_index"][:4] = special
    sp = split(s)
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        r, ri = s["radius"].astype(np.float32), s["refraction_index"].astype(np.float32)
        rr = r * r
        inv_ri = one / ri
        r0 = []
        for ratio in (inv_ri, ri):  # front face: 1 / ri; back: ri
            q = (one - ratio) / (one + ratio)
            r0.append(q * q)
    for a in (rr, inv_ri, r0[0], r0[1]):
        assert a.dtype == np.float32
    assert np.array_equal(u32(sp["geom"][:300, 3]), u32(rr))
    assert np.array_equal(u32(sp["mat"]["inv_ri"]), u32(inv_ri))
    assert np.array_equal(u32(sp["r0"][:, 0]), u32(r0[0]))
    assert np.array_equal(u32(sp["r0"][:, 1]), u32(r0[1]))
    # the special indices did what they are there for: ri = 1 -> r0 = 0; 0 -> inf, then inf / inf = NaN in the front r0
    assert sp["r0"][0, 0] == 0.0 and sp["r0"][0, 1] == 0.0
    assert np.isinf(sp["mat"]["inv_ri"][2]) and np.isinf(sp["mat"]["inv_ri"][3])
    assert np.isnan(sp["r0"][3, 0]) and sp["r0"][3, 1] == 1.0
    # the rest of the records are copies
    for f in ("albedo", "fuzz", "refraction_index", "type", "radius"):
        assert np.array_equal(sp["mat"][f].view(np.uint32), np.ascontiguousarray(s[f]).view(np.uint32)), f
    assert np.array_equal(u32(sp["radii"]), u32(s["radius"]))


def test_split_keeps_the_uuids_in_list_order():
    s = random_spheres(41, 9)
    assert len(set(s["uuid"])) == 41 and not np.array_equal(s["uuid"], np.sort(s["uuid"]))
    assert np.array_equal(split(s)["uuid"], s["uuid"])


# ---- (c) regular ----------------------------------------------------------------------------------------------------
def test_regular_is_every_coordinate_and_radius_below_1e15():
    base = random_spheres(9, 11)
    limit = np.float32(1e15)
    below = np.nextafter(limit, np.float32(0.0))
    assert below < limit and below.dtype == np.float32

    def with_(field, where, value):
        s = base.copy()
        if field == "center":
            s["center"][where[0], where[1]] = value
        else:
            s["radius"][where] = value
        return split(s)["regular"]

    assert split(base)["regular"]
    assert not with_("center", (3, 1), np.float32("nan"))
    assert not with_("radius", 5, np.float32("inf"))
    assert not with_("radius", 5, np.float32("-inf"))
    assert not with_("radius", 8, np.float32("nan"))
    for k in range(3):
        assert not with_("center", (8, k), limit)
        assert not with_("center", (0, k), -limit)
        assert with_("center", (8, k), below)
        assert with_("center", (0, k), -below)
    assert not with_("radius", 0, limit)
    assert with_("radius", 0, -below)


# ---- (d) per_slot ---------------------------------------------------------------------------------------------------
def test_per_slot_gathers_and_zeroes_the_slots_that_name_no_sphere():
    lib = shim()
    n_src = 13
    sp = split(random_spheres(n_src, 21))
    index = np.array([5, 0xFFFFFFFF, 0, n_src, 12, 12, n_src + 1, 3, 0x80000000], np.uint32)
    named = index < n_src
    assert named.sum() == 5
    mat = np.full(index.size, 0xAB, np.uint8).repeat(32).view(MAT_DTYPE)
    lib.scene_per_slot_mat(_vp(index), index.size, _vp(sp["mat"]), n_src, _vp(mat))
    uuid = np.full(index.size, -1, np.int32)
    lib.scene_per_slot_i32(_vp(index), index.size, _vp(sp["uuid"]), n_src, _vp(uuid))
    assert sp["uuid"].min() > 0
    for k, i in enumerate(index):
        if i < n_src:
            assert mat[k].tobytes() == sp["mat"][i].tobytes() and uuid[k] == sp["uuid"][i]
        else:
            assert mat[k].tobytes() == bytes(32) and uuid[k] == 0
    # no slots at all
    lib.scene_per_slot_i32(_vp(index), 0, _vp(sp["uuid"]), n_src, _vp(uuid))


# ---- (e) the grid's layout ------------------------------------------------------------------------------------------
MAX_SPHERES_LDS = 10232  # csrc/pt_kernel_args.h
WALK_LDS_ROOM = (((MAX_SPHERES_LDS + 7) & ~7) + 4) * 16 - 15 * 4 * 1024  # csrc/pt_geom_plan.hpp walk_lds_room


def image_grid(spheres, factor):
    lib = shim()
    ptr, n, keep = abi.spheres_as_ctypes(spheres)
    counts = np.zeros(8, np.uint32)
    rc = lib.scene_build_grid(ptr, n, factor, _vp(counts), None, 0, None, 0, None, 0)
    if rc != 0:
        return rc, None
    cells = np.zeros(int(counts[0]) * int(counts[1]) * int(counts[2]), np.uint32)
    entries = np.zeros(int(counts[5]) * 4, np.float32)
    index = np.zeros(int(counts[5]), np.uint32)
    assert lib.scene_build_grid(ptr, n, factor, _vp(counts), _vp(cells), cells.size, _vp(entries), entries.size, _vp(index), index.size) == 0
    return 0, dict(counts=counts, cells=cells, entries=entries, index=index)


def export_grid(spheres, runs):
    lib = _lib.load()
    fn = lib.pt_build_grid
    if runs:
        fn = lib.pt_build_grid_runs
        fn.restype, fn.argtypes = lib.pt_build_grid.restype, lib.pt_build_grid.argtypes
    ptr, n, keep = abi.spheres_as_ctypes(spheres)
    counts = np.zeros(8, np.uint32)
    rc = fn(ptr, n, _vp(counts), None, None, None, None, 0, None, 0, None, 0)
    if rc != 0:
        return rc, None
    cells = np.zeros(int(counts[0]) * int(counts[1]) * int(counts[2]), np.uint32)
    entries = np.zeros(int(counts[5]) * 4, np.float32)
    index = np.zeros(int(counts[5]), np.uint32)
    assert fn(ptr, n, _vp(counts), None, None, None, _vp(cells), cells.size, _vp(entries), entries.size, _vp(index), index.size) == 0
    return 0, dict(counts=counts, cells=cells, entries=entries, index=index)


def same_grid(a, b):
    return all(np.array_equal(a[k].view(np.uint32), np.asarray(b[k]).reshape(-1).view(np.uint32)) for k in ("counts", "cells", "entries", "index"))


def staged_bytes(g):
    """what bind_grid would stage of the grid: the cell records (a one-layer grid's in the ring layout), 16 B at a time, and the entries"""
    nx, ny, nz = (int(v) for v in g["counts"][:3])
    n_cells = (nx + 2) * (nz + 2) if ny == 1 else nx * ny * nz
    return (n_cells + 3) // 4 * 16 + int(g["counts"][5]) * 16


def test_a_scene_without_a_grid_gets_none_here_either():
    """State::default's nine spheres: too few for a grid, for pt_build_grid and for build_grid alike"""
    sph = scenes.default_scene(64, 36, 1, 8).spheres
    assert export_grid(sph, False)[0] == abi.PT_ERR_NOT_READY
    assert image_grid(sph, 3.0)[0] == abi.PT_ERR_NOT_READY
    sph = random_spheres(40, 3)
    sph["center"][7, 2] = 2e15  # irregular: no structure
    assert image_grid(sph, 3.0)[0] == abi.PT_ERR_NOT_READY


def test_a_grid_that_fits_the_lds_keeps_the_plain_layout():
    """the cover scene (the benchmark's default configuration, 484 spheres): staged whole, so its entries stay x-fastest"""
    sph = scenes.config2(96, 54, 2, 2, 12).spheres
    rc, got = image_grid(sph, 3.0)
    assert rc == 0
    rc, plain = export_grid(sph, False)
    assert rc == 0
    rc, runs = export_grid(sph, True)
    assert rc == 0 and not same_grid(plain, runs)  # (the two layouts differ on this scene: the comparison can fail)
    assert staged_bytes(got) <= WALK_LDS_ROOM
    assert same_grid(got, plain)


@pytest.mark.parametrize("factor", [3.0, 2.5])
def test_a_grid_beyond_the_lds_is_laid_out_as_morton_runs(factor):
    """config 5's field (10 001 spheres).  At the default class the expectation is pt_build_grid_runs' export; the export builds
    class 3 only, so at 2.5 it is the same builder and layout through grid_class_shim.cpp, which test_grid.py pins to the
    exports at class 3."""
    sph = scenes.config5(96, 54, 2, 2, 12).spheres
    rc, got = image_grid(sph, factor)
    assert rc == 0
    assert staged_bytes(got) > WALK_LDS_ROOM
    if factor == 3.0:
        rc, runs = export_grid(sph, True)
        assert rc == 0
        rc, plain = export_grid(sph, False)
        assert rc == 0
    else:
        rc, g = class_build(sph, runs=True, near_factor=factor)
        assert rc == 0
        runs = dict(counts=got["counts"], cells=g["cells"], entries=g["entries"], index=g["index"])
        assert [int(v) for v in got["counts"][:3]] == [int(v) for v in g["n"]] and int(got["counts"][5]) == g["n_entries"]
        rc, g = class_build(sph, runs=False, near_factor=factor)
        assert rc == 0
        plain = dict(counts=got["counts"], cells=g["cells"], entries=g["entries"], index=g["index"])
    assert not same_grid(plain, runs)
    assert same_grid(got, runs)


# ---- under sanitizers -----------------------------------------------------------------------------------------------
def test_the_scene_image_under_address_and_undefined_behaviour_sanitizers():
    """tests/scene_image_main.cpp: a stand-alone program (its own main) over the same list lengths, built with
    -fsanitize=address,undefined and run as a child; nothing sanitized is loaded into this process"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "scene_image_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(HERE, "scene_image_main.cpp"), "-o", exe])
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and "scene image: ok" in out.stdout, out.stdout[-2000:]
