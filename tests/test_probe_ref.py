"""Probe lattices on the CPU (pt_bake_lattice, pt_shade_probes; include/ptrace.h has the contract): the restatement
tests/probe_ref.py the device tests compare with, and csrc/pt_probe.hpp, which the kernels compile.

  1. the shading      csrc/pt_probe.hpp through tests/probe_shim.cpp equals the restatement's numpy statements bit for bit over the
                      sweep of tests/probe_sweep.hpp: g exactly on nodes, one ulp either side, below 0 and beyond the last node; f
                      of 0 and 1 with zero-weight corners not kept (and not read); each type and an unknown one; a miss; records
                      with samples == 0 in each corner and in all eight; the half-space test at dot == 0 and one ulp either side;
                      negative blends, which clamp; normal_bias 0 and 0.05.  tests/probe_main.cpp walks the same sweep under the
                      sanitizers;
  2. the nodes        positions, abi.probe_lattice_positions, and the buried rule at d2 == r * r and one ulp either side, glass, a
                      NaN centre, the flag off;
  3. the surface      the lattice and option checks and their wording, the ProbeSet in place or refused, struct sizes, symbols,
                      ABI version 5, the header's, Python's and Rust's agreement, and that no option key 14 appeared.
CPU only."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import probe_ref as P
from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd._lib import ADDED_WITHIN_ABI_5, LIB_PATH, SIGNATURES

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "ptrace.h")
F = np.float32
NAMES = ("pt_bake_lattice", "pt_shade_probes")
SET_MIXED, SET_INNER_EMPTY, SET_ALL_EMPTY, SET_NEGATIVE = range(4)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(tempfile.mkdtemp(prefix="probe_"), "libprobe_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror", os.path.join(HERE, "probe_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    fp, u32, u64, vp, lat = C.POINTER(C.c_float), C.c_uint32, C.c_uint64, C.c_void_p, C.POINTER(abi.PtProbeLattice)
    lib.prb_lattice_error.restype, lib.prb_lattice_error.argtypes = C.c_char_p, [lat]
    lib.prb_options_error.restype, lib.prb_options_error.argtypes = C.c_char_p, [u32, C.c_float]
    lib.prb_slice_valid.argtypes = [lat, u32, u32]
    lib.prb_node_count.restype, lib.prb_node_count.argtypes = u32, [lat]
    lib.prb_node_position.restype, lib.prb_node_position.argtypes = None, [lat, u32, fp]
    lib.prb_buried_by.argtypes = [fp, fp, C.c_int32]
    lib.prb_shade.restype, lib.prb_shade.argtypes = None, [lat, fp, u32, C.c_float, fp, u32, fp, C.POINTER(C.c_int32), fp, C.POINTER(u64)]
    lib.prb_sweep_lattice.restype, lib.prb_sweep_lattice.argtypes = None, [lat, fp]
    lib.prb_sweep_sets.restype = u32
    lib.prb_sweep_records.restype, lib.prb_sweep_records.argtypes = None, [C.c_int, fp]
    lib.prb_sweep_pixels.restype, lib.prb_sweep_pixels.argtypes = u32, [fp, C.POINTER(C.c_int32)]
    lib.alloc_fail_at.argtypes = [C.c_long]
    lib.alloc_live.restype = C.c_long
    lib.set_new.restype = vp
    for f in (lib.set_delete, lib.set_release_points, lib.set_release_stage, lib.set_points_capacity, lib.set_stage_capacity):
        f.argtypes = [vp]
    for f in (lib.set_fit_points, lib.set_fit_stage, lib.set_points_in_place, lib.set_stage_in_place):
        f.argtypes = [vp, u64]
    lib.set_points_capacity.restype = lib.set_stage_capacity.restype = u64
    return lib


@pytest.fixture(scope="module")
def sweep(shim):
    """(lattice, camera, f9 (n, 9), i2 (n, 2), [records per set])"""
    lat, cam = abi.PtProbeLattice(), np.zeros(3, F)
    shim.prb_sweep_lattice(C.byref(lat), _fp(cam))
    n = shim.prb_sweep_pixels(None, None)
    f9, i2 = np.zeros((n, 9), F), np.zeros((n, 2), np.int32)
    shim.prb_sweep_pixels(_fp(f9), i2.ctypes.data_as(C.POINTER(C.c_int32)))
    sets = []
    for s in range(shim.prb_sweep_sets()):
        r = np.zeros((lat.nodes, 28), F)
        shim.prb_sweep_records(s, _fp(r))
        sets.append(r)
    return lat, cam, f9, i2, sets


def shim_shade(shim, lat, records, flags, bias, cam, f9, i2):
    out, loads = np.zeros((len(f9), 4), F), C.c_uint64()
    shim.prb_shade(C.byref(lat), _fp(records), flags, bias, _fp(cam), len(f9), _fp(f9), i2.ctypes.data_as(C.POINTER(C.c_int32)), _fp(out), C.byref(loads))
    return out, loads.value


def ref_shade(lat, records, flags, bias, cam, f9, i2, stats=None):
    ids = np.zeros((len(f9), 4), np.int32)
    ids[:, 0], ids[:, 2] = i2[:, 0], i2[:, 1]
    return P.shade(f9[:, 0:3], f9[:, 3:6], f9[:, 6:9], ids, lat, records, flags, bias, cam, stats)


# ------------------------------------------------------------------------------------- 1. the shading
def test_the_sweep_holds_what_it_promises(sweep):
    lat, cam, f9, i2, sets = sweep
    assert (lat.nx, lat.ny, lat.nz) == (3, 3, 4) and len(sets) == 4 and P.lattice_error(lat) is None
    hp, typ = f9[:, 6:9], i2[:, 1]
    pos = P.node_positions(lat)
    g = (hp.astype(np.float64) - np.array(list(lat.origin))) / np.array(list(lat.step))
    gx = (hp[:, 0] - F(lat.origin[0])) / F(lat.step[0])  # (the dyadic axis: g is exact)
    on = (hp[:, None, :] == pos[None, :, :]).all(axis=2).any(axis=1)
    assert on.any() and (gx == 0).any() and (gx == 2).any() and (gx == 1).any(), "g exactly on the first, the last and an inner node"
    assert (gx == np.nextafter(F(2), F(9))).any() and (gx == np.nextafter(F(2), F(-9))).any() and (gx == np.nextafter(F(1), F(9))).any(), "g one ulp either side of an index"
    assert ((gx > 0) & (gx < 1e-6)).any() and ((gx < 0) & (gx > -1e-6)).any(), "hp one ulp either side of the first node"
    assert (hp[:, 0] == np.nextafter(pos[0, 0], F(-np.inf))).any() and (hp[:, 0] == np.nextafter(pos[0, 0], F(np.inf))).any()
    assert (g < 0).any(axis=0).all() and (g > np.array([2, 2, 3])).any(axis=0).all(), "below 0 and beyond the last node on every axis"
    assert set(typ.tolist()) >= {abi.PT_DIFFUSE, abi.PT_METAL, abi.PT_GLASS, abi.PT_EMISSIVE, 7} and (i2[:, 0] < 0).any()
    assert (sets[SET_MIXED][:, :27] < 0).any() and (sets[SET_MIXED][:, :27] > 0).any() and (sets[SET_MIXED][:, 27] > 0).all()
    assert (sets[SET_INNER_EMPTY][:, 27] == 0).sum() == 1 and sets[SET_INNER_EMPTY][13, 27] == 0 and not sets[SET_ALL_EMPTY][:, 27].any()
    # the eight cells around node (1, 1, 1) see it as each of their corners
    inner = np.nonzero((np.abs(g - 1.0) < 0.9).all(axis=1) & ~(np.abs(g - 1.0) < 1e-5).any(axis=1))[0]
    corners = {tuple((g[k] < 1.0).astype(int)) for k in inner}
    assert len(corners) == 8
    # the half-space test at dot == 0 and either side: an axis normal at a point on a node, and one ulp off it along that axis
    n = f9[:, 3:6]
    for k in np.nonzero(on & (n[:, 1] == 1) & (typ == abi.PT_DIFFUSE))[0][:1]:
        e = pos[:, 1].astype(np.float64) - float(hp[k, 1])
        assert (e == 0).any()
    up = (n[:, 1] == 1) & (typ == abi.PT_DIFFUSE)
    dy = hp[up, 1][:, None].astype(np.float64) - pos[None, :, 1].astype(np.float64)
    ulp = float(np.spacing(F(0.4)))
    assert (dy == 0).any() and ((dy > 0) & (dy <= ulp)).any() and ((dy < 0) & (dy >= -ulp)).any()


@pytest.mark.parametrize("bias", [0.0, 0.05])
@pytest.mark.parametrize("flags", [0, 1], ids=["all-corners", "halfspace"])
@pytest.mark.parametrize("which", [SET_MIXED, SET_INNER_EMPTY, SET_ALL_EMPTY, SET_NEGATIVE], ids=["mixed", "inner-empty", "all-empty", "negative"])
def test_the_header_equals_the_restatement_over_the_sweep(shim, sweep, which, flags, bias):
    lat, cam, f9, i2, sets = sweep
    got, loads = shim_shade(shim, lat, sets[which], flags, bias, cam, f9, i2)
    stats = {}
    want = ref_shade(lat, sets[which], flags, bias, cam, f9, i2, stats)
    assert not np.isnan(got).any() and not np.isnan(want).any()
    assert np.array_equal(bits(got), bits(want)), np.nonzero((bits(got) != bits(want)).any(axis=1))[0][:10]
    typ, index = i2[:, 1], i2[:, 0]
    flat = (index < 0) | ~np.isin(typ, (abi.PT_DIFFUSE, abi.PT_METAL, abi.PT_GLASS))
    assert (got[flat, 3] == 1).all()
    miss = index < 0
    assert np.array_equal(bits(got[miss, :3]), bits(f9[miss, 0:3])), "a miss: the background in the albedo plane"
    emissive = ~miss & (typ == abi.PT_EMISSIVE)
    assert np.array_equal(bits(got[emissive, :3]), bits(f9[emissive, 0:3]))
    unknown = ~miss & ~np.isin(typ, (0, 1, 2, 3))
    assert unknown.any() and not got[unknown, :3].any(), "a type outside the four absorbs"
    assert set(np.unique(got[:, 3]).tolist()) <= {0.0, 1.0} and (got[:, :3] >= 0).all()
    assert not got[got[:, 3] == 0].any(), "alpha 0: all +0"
    kept = stats["kept"]
    assert ((kept > 0) == (got[:, 3] == 1))[~flat].all()
    if which == SET_ALL_EMPTY:
        assert not got[~flat].any(), "samples == 0 in all eight corners: no usable probe"
    else:
        assert (got[~flat, 3] == 1).any()
        if which == SET_INNER_EMPTY and bias == 0.0:
            assert (got[~flat, 3] == 0).any(), "the pixels ON the empty node have no other corner (a bias moves them off it)"
        else:
            assert (got[~flat, 3] == 0).any() == bool(flags), "with every record usable only the half-space test leaves a pixel without a probe"
    if which == SET_NEGATIVE:
        d = ~flat & (typ == abi.PT_DIFFUSE) & (got[:, 3] == 1)
        assert d.any() and not got[d, :3].any(), "negative blends clamp at 0, alpha stays 1"
    if which == SET_MIXED:
        # zero-weight corners are not kept AND not read: the records fetched are the corners with w > 0 that pass the half-space test
        wanted = 0
        for k in np.nonzero(~flat)[0]:
            s = {}
            ref_shade(lat, np.where(np.arange(28) == 27, F(1.0), sets[which]).astype(F), flags, bias, cam, f9[k:k + 1], i2[k:k + 1], s)
            wanted += int(s["kept"][0])
        assert loads == wanted
        if flags == 0 and bias == 0.0:
            on_node = ~flat & (f9[:, 6:9] == P.node_positions(lat)[13]).all(axis=1)
            assert on_node.any() and (kept[on_node] == 1).all(), "f of 0 on every axis: one corner, weight 1"


def test_an_empty_corner_is_dropped_and_the_rest_renormalised(shim, sweep):
    """the pixels of the eight cells around node (1, 1, 1) with that node's samples 0: its weight leaves W, the others' stay"""
    lat, cam, f9, i2, sets = sweep
    full, empty = {}, {}
    a = ref_shade(lat, sets[SET_MIXED], 0, 0.0, cam, f9, i2, full)
    b = ref_shade(lat, sets[SET_INNER_EMPTY], 0, 0.0, cam, f9, i2, empty)
    fewer = empty["kept"] < full["kept"]
    assert fewer.any() and ((full["kept"] - empty["kept"])[fewer] == 1).all()
    assert np.array_equal(bits(a[~fewer]), bits(b[~fewer])) and (bits(a[fewer]) != bits(b[fewer])).any()
    only = fewer & (full["kept"] == 1)  # the pixel ON the node: its one corner is gone
    assert only.any() and not b[only].any()


def test_header_under_address_and_undefined_behaviour_sanitizers():
    """tests/probe_main.cpp: a stand-alone program (its own main) over csrc/pt_probe.hpp on the sweep and exactly sized heap
    arrays, built with -fsanitize=address,undefined and run as a child; nothing sanitized is loaded into this process"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "probe_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                               os.path.join(HERE, "probe_main.cpp"), "-o", exe])
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and "probe: ok" in out.stdout, out.stdout[-2000:]


# ------------------------------------------------------------------------------------- 2. the nodes
def test_node_positions_three_ways(shim, sweep):
    lat = sweep[0]
    for L in (lat, abi.PtProbeLattice(origin=(0.1, -7.3, 1e-3), step=(0.7, 1.0 / 3.0, 123.456), n=(5, 2, 7)),
              abi.PtProbeLattice(origin=(-1.0000001, 3.3333333, 0.1), step=(0.1, 0.1, 0.013), n=(256, 2, 3))):
        want = P.node_positions(L)
        got = np.zeros((L.nodes, 3), F)
        for i in range(L.nodes):
            shim.prb_node_position(C.byref(L), i, _fp(got[i]))
        assert shim.prb_node_count(C.byref(L)) == L.nodes == len(want)
        assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(bits(abi.probe_lattice_positions(L)), bits(want)), "the package's numpy fma"
        i = (1 * L.ny + 1) * L.nx + 2
        assert np.array_equal(want[i], [P.fma(F(2), F(L.step[0]), F(L.origin[0])), P.fma(F(1), F(L.step[1]), F(L.origin[1])), P.fma(F(1), F(L.step[2]), F(L.origin[2]))])


def test_the_buried_rule(shim):
    pos = np.array([0.3, -1.2, 2.5], F)
    centre = np.array([0.3, -1.2, 2.0], F)   # w = (0, 0, 0.5): d2 = 0.25 exactly
    rr = F(0.25)
    for value, want in ((rr, False), (np.nextafter(rr, F(1)), True), (np.nextafter(rr, F(0)), False)):
        geom = np.array([*centre, value], F)
        assert bool(shim.prb_buried_by(_fp(pos), _fp(geom), abi.PT_DIFFUSE)) == want, "strict: d2 == r * r is on the surface"
    inside = np.array([*centre, 1.0], F)
    for typ, want in ((abi.PT_DIFFUSE, True), (abi.PT_METAL, True), (abi.PT_EMISSIVE, True), (9, True), (abi.PT_GLASS, False)):
        assert bool(shim.prb_buried_by(_fp(pos), _fp(inside), typ)) == want
    for bad in (np.array([np.nan, -1.2, 2.0, 1e30], F), np.array([0.3, -1.2, 2.0, np.nan], F)):
        assert not shim.prb_buried_by(_fp(pos), _fp(bad), abi.PT_DIFFUSE), "a NaN centre never buries"
    # ... and the restatement, through PtSphere lists: r * r is the fp32 product, a negative radius buries as its square
    def sphere(c, r, typ):
        s = abi.PtSphere()
        s.center[:] = c
        s.radius, s.type = r, typ
        return s
    lat = abi.PtProbeLattice(origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), n=(3, 2, 2), flags=abi.PT_LATTICE_SKIP_BURIED)
    spheres = [sphere((1.0, 0.0, 0.0), -0.5, abi.PT_METAL), sphere((2.0, 1.0, 1.0), 0.5, abi.PT_GLASS), sphere((np.nan, 0.0, 0.0), 50.0, abi.PT_DIFFUSE),
               sphere((0.0, 1.0, 1.0), 1.0, abi.PT_DIFFUSE)]
    pts = P.lattice_points(lat, spheres)
    nan = np.isnan(pts).all(axis=1)
    assert np.array_equal(np.nonzero(nan)[0], [1, 9]) and np.isnan(pts).any(axis=1).sum() == 2, "node (1,0,0) and node (0,1,1); (0,0,1) is ON the last sphere"
    lat.flags = 0
    assert not np.isnan(P.lattice_points(lat, spheres)).any(), "the flag off"
    assert np.array_equal(bits(P.lattice_points(lat, spheres, 3, 5)), bits(P.node_positions(lat)[3:8]))
    for p, s in ((pts_k, s) for pts_k in P.node_positions(lat) for s in spheres):
        geom = np.array([*list(s.center), F(s.radius) * F(s.radius)], F)
        assert bool(shim.prb_buried_by(_fp(p.copy()), _fp(geom), int(s.type))) == bool(P.buried(p, [s])[0])


# ------------------------------------------------------------------------------------- 3. the surface
def test_the_lattice_and_option_checks_and_their_wording(shim):
    def lat(**kw):
        L = abi.PtProbeLattice(origin=kw.pop("origin", (0.0, 0.0, 0.0)), step=kw.pop("step", (1.0, 1.0, 1.0)), n=kw.pop("n", (2, 2, 2)), flags=kw.pop("flags", 0))
        return L
    inf, nan = np.inf, np.nan
    cases = [(lat(), None), (lat(n=(256, 256, 16)), None), (lat(n=(2, 2, 256), flags=1), None),
             (lat(n=(1, 2, 2)), "nx, ny and nz lie in [2, 256]"), (lat(n=(2, 257, 2)), "nx, ny and nz lie in [2, 256]"), (lat(n=(2, 2, 0)), "nx, ny and nz lie in [2, 256]"),
             (lat(n=(256, 256, 17)), "nx * ny * nz is at most 2^20"), (lat(n=(256, 256, 256)), "nx * ny * nz is at most 2^20"),
             (lat(step=(0.0, 1.0, 1.0)), "every step is finite and > 0"), (lat(step=(1.0, -1.0, 1.0)), "every step is finite and > 0"),
             (lat(step=(1.0, 1.0, inf)), "every step is finite and > 0"), (lat(step=(nan, 1.0, 1.0)), "every step is finite and > 0"),
             (lat(origin=(0.0, inf, 0.0)), "every origin component is finite"), (lat(origin=(0.0, 0.0, nan)), "every origin component is finite"),
             (lat(flags=2), "flags holds PT_LATTICE_SKIP_BURIED or nothing"), (lat(step=(1e-45, 1.0, 1.0)), None)]
    for L, want in cases:
        got = shim.prb_lattice_error(C.byref(L))
        assert (got.decode() if got else None) == want == P.lattice_error(L), (list(L.step), want)
    L = lat(n=(3, 2, 5))
    for first, count, want in ((0, 30, True), (0, 31, False), (29, 1, True), (30, 0, True), (30, 1, False), (2 ** 32 - 1, 1, False), (2 ** 32 - 1, 2 ** 32 - 1, False)):
        assert bool(shim.prb_slice_valid(C.byref(L), first, count)) == want == P.slice_valid(L, first, count)
    for flags, bias, want in ((0, 0.0, None), (1, 0.05, None), (1, -3.0, None), (2, 0.0, "flags holds PT_PROBE_HALFSPACE or nothing"),
                              (1, inf, "normal_bias is finite"), (0, nan, "normal_bias is finite")):
        got = shim.prb_options_error(flags, bias)
        assert (got.decode() if got else None) == want == P.options_error(flags, bias)
    api = open(os.path.join(ROOT, "ray_tracer_webgl_amd", "csrc", "pt_api.hip")).read()
    body = api[api.index("PT_API int pt_bake_lattice("):api.index("PT_API int pt_shade_probes(")]
    order = ["ptprobe::lattice_error", "estimator %d", "ptprobe::slice_valid", "count == 0", "gather_ready(c, who, next_event, lattice", "c->probe.fit_points",
             "call(ptsig::ProbePoints{}", "return gather_batches(c, who, ptgather::PROBE"]
    at = [body.index(s) for s in order]
    assert at == sorted(at), "the lattice's own checks, the gather call's, the point buffer, the generator, then the one bake loop"
    assert body.count("call(ptsig::") == 1 and "query_ready" not in body and "passes_ready" not in body, "no second copy of the bake loop or of the gather calls' checks"
    ready = api[api.index("static int gather_ready("):api.index("static int gather_batches(")]
    order = ["query_ready(c, who", "passes_ready(c, who", "directions (a multiple of 64 in", "are more than 2^32 - 1 rays", "estimator_ready(c, who"]
    at = [ready.index(s) for s in order]
    assert at == sorted(at), "what pt_bake_lattice refuses before its generator runs: the gather calls' checks in their order"
    body = api[api.index("PT_API int pt_shade_probes("):]
    order = ["ptprobe::lattice_error", "ptprobe::options_error", "not with PT_OPT_COUNT_WORK", "SET_FEATURES", "c->feat.valid", "is_capturing", "c->local_rows == 0",
             "c->probe.fit_stage", "call(ptsig::ProbeShadeShared{}", "call(ptsig::ProbeShade{}"]
    at = [body.index(s) for s in order]
    assert at == sorted(at)
    assert "unknown key %d" in api and not re.search(r"#define\s+PT_OPT_\w+\s+14\b", open(HEADER).read()), "no new option key"
    assert 14 not in [v for k, v in vars(abi).items() if k.startswith("PT_OPT_")]
    state = open(os.path.join(ROOT, "ray_tracer_webgl_amd", "csrc", "pt_ctx_state.hpp")).read()
    assert "ProbeSet" not in state and "lattice" not in state.lower(), "no new validity bit: the shading reads the feature planes' validity"


def test_the_probe_set_is_in_place_or_refused(shim):
    s = shim.set_new()
    try:
        assert shim.set_points_in_place(s, 30) == 0 and shim.set_stage_in_place(s, 30) == 0 and shim.alloc_live() == 0
        shim.alloc_fail_at(1)
        assert shim.set_fit_points(s, 30) == 1 and shim.set_points_in_place(s, 30) == 0 and shim.set_points_capacity(s) == 0 and shim.alloc_live() == 0
        shim.alloc_fail_at(0)
        assert shim.set_fit_points(s, 30) == 0 and shim.set_points_in_place(s, 30) == 1 and shim.set_points_capacity(s) == 8 * 30
        assert shim.set_stage_in_place(s, 30) == 0 and shim.alloc_live() == 1, "the two buffers are fitted apart"
        assert shim.set_fit_stage(s, 30) == 0 and shim.set_stage_capacity(s) == 28 * 30 and shim.alloc_live() == 2
        assert shim.set_points_in_place(s, 8) == 1 and shim.set_fit_points(s, 8) == 0 and shim.set_points_capacity(s) == 8 * 30, "a smaller lattice keeps the buffer"
        assert shim.set_points_in_place(s, 31) == 0
        shim.alloc_fail_at(1)   # growing: the old buffer is freed first, the refused one leaves nothing
        assert shim.set_fit_stage(s, 64) == 1 and shim.set_stage_capacity(s) == 0 and shim.set_stage_in_place(s, 1) == 0 and shim.alloc_live() == 1
        assert shim.set_points_in_place(s, 30) == 1, "the other buffer stays"
        shim.alloc_fail_at(0)
        assert shim.set_fit_stage(s, 64) == 0 and shim.set_stage_in_place(s, 64) == 1 and shim.alloc_live() == 2
        shim.set_release_points(s)   # with PT_OPT_RAY_QUERIES
        assert shim.alloc_live() == 1 and shim.set_points_in_place(s, 1) == 0 and shim.set_stage_in_place(s, 64) == 1
        shim.set_release_stage(s)    # with PT_OPT_FEATURES
        assert shim.alloc_live() == 0 and shim.set_stage_in_place(s, 1) == 0
        assert shim.set_fit_points(s, 0) == 0 and shim.set_points_capacity(s) == 8, "0 counts as 1"
    finally:
        shim.set_delete(s)
    api = open(os.path.join(ROOT, "ray_tracer_webgl_amd", "csrc", "pt_api.hip")).read()
    assert "c->gather.release(); c->probe.release_points();" in api and "c->feat.release(); c->probe.release_stage();" in api


def test_symbols_signatures_and_the_abi_version(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB_PATH], text=True)
    exported = set(re.findall(r" T (pt_[a-z0-9_]+)", out))
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "ptrace_sys.rs")).read()
    want = {"pt_bake_lattice": ["ctx", "lattice", "first", "count", "directions", "n_passes", "estimator", "out"],
            "pt_shade_probes": ["ctx", "lattice", "probes", "options", "rgba_out"]}
    for name in NAMES:
        assert name in exported and hasattr(lib, name) and name in SIGNATURES and name in ADDED_WITHIN_ABI_5, name
        h = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        r = re.search(r"pub fn %s\(([^)]*)\)" % name, rust)
        assert h and r
        args_h = [a.split()[-1].lstrip("*") for a in h.group(1).split(",")]
        args_r = [a.split(":")[0].strip() for a in r.group(1).split(",")]
        assert args_h == args_r == want[name]
        assert len(SIGNATURES[name][1]) == len(want[name])
    assert lib.pt_abi_version() == 5 == abi.PT_ABI_VERSION and re.search(r"#define\s+PT_ABI_VERSION\s+5\b", header)
    assert "pt_lattice_kernel" not in exported, "the kernels' accessor stays inside the library"
    for const, value in (("PT_LATTICE_SKIP_BURIED", 1), ("PT_PROBE_HALFSPACE", 1)):
        assert re.search(r"#define\s+%s\s+%du\b" % (const, value), header) and getattr(abi, const) == value
        assert re.search(r"pub const %s: u32 = %d;" % (const, value), rust)


def test_the_structs_match_the_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "ptrace.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu %zu ", sizeof(PtProbeLattice), offsetof(PtProbeLattice, origin), offsetof(PtProbeLattice, nx), offsetof(PtProbeLattice, step),
        offsetof(PtProbeLattice, ny), offsetof(PtProbeLattice, nz), offsetof(PtProbeLattice, flags));
 printf("%zu %zu %zu\n", sizeof(PtProbeShadeOptions), offsetof(PtProbeShadeOptions, flags), offsetof(PtProbeShadeOptions, normal_bias));
 return 0; }'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got == [48, 0, 12, 16, 28, 32, 36, 16, 0, 4]
    L, O = abi.PtProbeLattice, abi.PtProbeShadeOptions
    assert got == [C.sizeof(L), L.origin.offset, L.nx.offset, L.step.offset, L.ny.offset, L.nz.offset, L.flags.offset, C.sizeof(O), O.flags.offset, O.normal_bias.offset]
    rust = open(os.path.join(ROOT, "bindings", "rust", "ptrace_sys.rs")).read()
    for name, fields in (("PtProbeLattice", ["origin", "nx", "step", "ny", "nz", "flags", "_pad"]), ("PtProbeShadeOptions", ["flags", "normal_bias", "_pad"])):
        body = re.search(r"pub struct %s \{(.*?)\n\}" % name, rust, flags=re.S).group(1)
        assert re.findall(r"pub (\w+):", body) == fields
    d = abi.PtProbeShadeOptions()
    assert d.flags == abi.PT_PROBE_HALFSPACE and d.normal_bias == 0.0, "the default is the call's NULL"


def test_the_header_carries_the_contract():
    text = " ".join(open(HEADER).read().split())
    for phrase in ("node i = (iz * ny + iy) * nx + ix", "position.c = fma(float(i_c), step.c, origin.c)", "d2 = fma(w.z, w.z, fma(w.y, w.y, w.x * w.x)); d2 < r * r",
                   "a NaN centre never buries", "AN ITEM'S INDEX, AND WITH IT ITS SEEDS, IS ITS INDEX IN THE CALL, NOT IN THE LATTICE",
                   "a sliced bake draws other samples than a whole one", "q.c = fma(normal_bias, n.c, hp.c)", "g.c = (q.c - origin.c) / step.c",
                   "i.c = clamp(int(floor(g.c)), 0, n_c - 2)", "f.c = min(max(g.c - float(i.c), 0), 1)", "b = (3.14159265f, 2.09439510f x3, 0.785398163f x5)",
                   "d = dot(v, n); k = 2 * d; m.c = k * n.c; r.c = v.c - m.c; omega = unit(r); b = 1", "GLASS: omega = unit(v); b = 1",
                   "fuzz and refraction do not enter", "w_k = (wx * wy) * wz", "dot(pos_k - hp, n) > 0", "E_k.c = fma(B_8, sh[8].c, ... fma(B_0, sh[0].c, +0))",
                   "S.c = fma(w_k, E_k.c, S.c)", "out.c = albedo.c * (v.c * 0.318309886f)", "alpha 0 is the mark of \"no usable probe\"",
                   "OUT OF SCOPE: visibility-weighted or octahedral-depth probes", "a FrameLoop mode", "nx, ny, nz lie in [2, 256] and nx * ny * nz is at most 2^20"):
        assert phrase in text, phrase


def test_errors_that_need_no_device(lib):
    lat, out = abi.PtProbeLattice(), (abi.PtProbeSH * 8)()
    img = (C.c_float * 16)()
    assert lib.pt_bake_lattice(None, C.byref(lat), 0, 8, 64, 1, 0, out) == abi.PT_ERR_INVALID
    assert lib.pt_shade_probes(None, C.byref(lat), out, None, img) == abi.PT_ERR_INVALID
    assert not bytes(out).strip(b"\0") and not bytes(img).strip(b"\0")
