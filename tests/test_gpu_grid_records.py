"""GPU parity of the grid kernels on the device cell records of csrc/pt_grid_records.hpp (every build: the leaf round takes a
short cell's valid mask from the record and sends long cells through a rare branch) and of the one-layer walk on the ring
layout (pt_trace_kernel_grid and its twin: a walk that leaves the grid sideways ends on a border record).

Small frames (64 x 48, 2 - 4 spp, depth 8), compared bit for bit, with segment counts, against the scalar list walk of the
same context and against the oracle:

  (a) a one-layer field whose cells hold 0, 1, 4, 5, 8 and 9 or more entries (clusters of small spheres inside one cell; the
      host build of the same grid says that such cells exist), seen from above;
  (b) the same field from a camera INSIDE it looking outward along +x, -x, +z, -z and up: primary and bounce rays leave the
      layer through each of its four sides and through the top (the centre ray's exit side is checked against the grid's box);
  (c) a grid of several layers with long cells: pt_trace_kernel_grid_layers;
  (d) a field at the smallest size (in steps of 250 spheres) whose entries no longer fit the LDS: pt_trace_kernel_grid_cells;
  and the measuring twin, the roulette build and the overlay build of the one-layer row on (a)'s field: the twin walks the ring,
  the other two walk the plain records along three axes.
Every case asserts PtStats.grid_kernel_build / grid_walk_flat, so that it runs the kernel it names.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from ray_tracer_webgl_amd import _lib, abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer
from test_bvh import random_field
from test_grid import build

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 64, 48
ORACLE_THREADS = min(16, os.cpu_count() or 1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert np.array_equal(g, r), "%s: %d of %d values differ" % (what, int((g != r).sum()), g.size)


def with_clusters(base, spots, sizes, seed, r=0.02, spread=0.05):
    """`base` plus, around each of `spots`, a cluster of sizes[k] small spheres (radius r, centres within `spread`)"""
    rng = np.random.default_rng(seed)
    extra = np.zeros(int(sum(sizes)), dtype=base.dtype)
    k = 0
    for spot, m in zip(spots, sizes):
        for _ in range(m):
            extra[k] = base[1 + k % (len(base) - 1)]  # (a material of the scene's own)
            extra[k]["center"] = np.asarray(spot, np.float32) + rng.uniform(-spread, spread, 3).astype(np.float32)
            extra[k]["radius"] = np.float32(r)
            k += 1
    return np.concatenate([base, extra])


def clustered_flat_field():
    """spheres standing on a ground, thinned on one side (empty cells), and clusters of 3 ... 12 small spheres on the ground"""
    s = random_field(90, 31, extent=6.0, rmax=0.3, giants=1)
    s["center"][0] = (0.0, -1000.0, 0.0)
    s["center"][1:, 1] = np.abs(s["radius"][1:])
    keep = np.ones(len(s), bool)
    keep[1:] = ~((s["center"][1:, 0] > 1.5) & (s["center"][1:, 2] > 1.5))  # a bare corner
    s = s[keep]
    rng = np.random.default_rng(7)
    sizes = [3, 4, 4, 5, 5, 7, 8, 8, 9, 10, 12, 12]
    spots = [(rng.uniform(-5.5, 1.0), 0.08, rng.uniform(-5.5, 5.5)) for _ in sizes]
    return with_clusters(s, spots, sizes, 8)


def clustered_layers_field():
    s = random_field(300, 1)
    rng = np.random.default_rng(9)
    c = s["center"][np.abs(s["radius"]) < 50.0]
    lo, hi = c.min(0), c.max(0)
    sizes = [5, 6, 8, 9, 11, 14]
    spots = [tuple(rng.uniform(lo + 0.2 * (hi - lo), hi - 0.2 * (hi - lo))) for _ in sizes]
    return with_clusters(s, spots, sizes, 10)


def counts_of(g):
    return (g["cells"] >> 24).astype(np.int64)


def look(w, h, spp, depth, eye, at, vfov, focus):
    p = scenes._base_params(spp, depth)
    scenes._look_at(_lib.load(), p, w, h, tuple(float(x) for x in eye), tuple(float(x) for x in at), vfov, 0.0, focus)
    return p


def render(t, p, n_passes=1):
    t.set_params(p)
    t.reserve_passes(n_passes)
    t.reset()
    t.render_passes(n_passes)
    return t.accum(), t.stats()


def check_against_list_and_oracle(ora, t, sph, p, what, build_kind, flat):
    """the grid walk's frame and segment count == the scalar list walk's of the same context == the oracle's"""
    t.set_geometry_path(abi.PT_GEOM_GRID)
    got, st = render(t, p)
    assert st.geometry_path == abi.PT_GEOM_GRID and st.grid_fit_stale != 1, (what, st.geometry_path, st.grid_fit_stale)
    assert st.grid_kernel_build == build_kind and st.grid_walk_flat == flat, (what, st.grid_kernel_build, st.grid_walk_flat)
    t.set_geometry_path(abi.PT_GEOM_SCALAR)
    lst, ls = render(t, p)
    assert ls.geometry_path == abi.PT_GEOM_SCALAR
    assert_bit_equal(got, lst, what + " (list walk)")
    assert st.segments == ls.segments, (what, st.segments, ls.segments)
    ref, seg = ora.render(sph, p, 1, nthreads=ORACLE_THREADS)
    assert_bit_equal(got, ref, what + " (oracle)")
    assert st.segments == seg and seg >= W * H * p.samples_per_pixel, (what, st.segments, seg)
    return got, st


@pytest.fixture(scope="module")
def flat():
    """the clustered one-layer field, its host grid and one context that holds it"""
    sph = clustered_flat_field()
    rc, g = build(sph)
    assert rc == 0 and int(g["n"][1]) == 1, g["n"]
    cnt = counts_of(g)
    have = set(int(c) for c in cnt)
    assert {0, 1, 4, 5, 8} <= have and cnt.max() >= 9, sorted(have)
    t = PathTracer(W, H)
    t.set_spheres(sph)
    yield sph, g, t
    t.close()


def test_a_one_layer_field_with_empty_short_full_and_long_cells(ora, flat):
    sph, g, t = flat
    c0, s0 = g["c0"].astype(np.float64), float(g["s0"])
    for spp, towards in ((2, (0.15, 0.95, 0.27)), (4, (0.8, 0.3, 0.6))):
        d = np.asarray(towards) / np.linalg.norm(towards)
        p = look(W, H, spp, 8, c0 + 1.5 * s0 * d, c0, 50.0, 2.0 * s0)
        _, st = check_against_list_and_oracle(ora, t, sph, p, "clustered flat field from %s" % (towards,), 1, 1)
        assert tuple(st.grid_cells) == tuple(int(x) for x in g["n"]) and st.grid_entries == g["n_entries"]


def exit_side(g, o, d):
    """(axis, sign) of the side through which the ray o + t d leaves the grid's box"""
    with np.errstate(divide="ignore"):
        t_far = np.where(d > 0, (g["hi"] - o) / d, np.where(d < 0, (g["lo"] - o) / d, np.inf))
    k = int(np.argmin(t_far))
    return k, 1 if d[k] > 0 else -1


OUTWARD = [("+x", (1.0, 0.02, 0.0), (0, 1)), ("-x", (-1.0, 0.02, 0.0), (0, -1)), ("+z", (0.0, 0.02, 1.0), (2, 1)),
           ("-z", (0.0, 0.02, -1.0), (2, -1)), ("up", (0.05, 1.0, 0.03), (1, 1))]


@pytest.mark.parametrize("case", OUTWARD, ids=[c[0] for c in OUTWARD])
def test_walks_that_leave_the_layer_through_each_side_and_the_top(ora, flat, case):
    name, towards, side = case
    sph, g, t = flat
    lo, hi = g["lo"].astype(np.float64), g["hi"].astype(np.float64)
    # inside the field and inside the layer: a third of the way across, at half the layer's height
    eye = np.array([lo[0] + 0.37 * (hi[0] - lo[0]), 0.5 * (lo[1] + hi[1]), lo[2] + 0.41 * (hi[2] - lo[2])])
    assert np.all(eye > lo) and np.all(eye < hi)
    d = np.asarray(towards, np.float64)
    assert exit_side(g, eye, d) == side, (name, exit_side(g, eye, d))
    p = look(W, H, 3, 8, eye, eye + d, 40.0, 1.0)
    check_against_list_and_oracle(ora, t, sph, p, "camera inside the field looking %s" % name, 1, 1)


def test_the_twin_walks_the_ring_and_the_roulette_and_overlay_builds_the_plain_records(flat):
    """the one-layer row's four builds on one grid: the timed kernel and its twin read the ring layout, the roulette and the
    overlay build (three axes) the plain records of the same cells"""
    sph, g, t = flat
    c0, s0 = g["c0"].astype(np.float64), float(g["s0"])
    d = np.asarray([0.8, 0.12, 0.6]) / np.linalg.norm([0.8, 0.12, 0.6])
    p = look(W, H, 4, 8, c0 + 0.5 * s0 * d, c0, 60.0, s0)
    t.set_geometry_path(abi.PT_GEOM_GRID)
    got, st = render(t, p)
    assert st.grid_kernel_build == 1 and st.grid_walk_flat == 1
    t.set_count_work(True)
    try:
        twin, sw = render(t, p)
    finally:
        t.set_count_work(False)
    assert sw.grid_kernel_build == 1 and sw.grid_walk_flat == 1 and sw.work[0] > 0 and sw.work[2] > 0
    assert_bit_equal(twin, got, "measuring twin")
    assert sw.segments == st.segments
    # the overlay (the cursor dot in the middle of the field): the overlay build against the list walk's overlay build
    t.set_debug_overlay(True, cursor_point=tuple(float(x) for x in c0))
    try:
        dbg, sd = render(t, p)
        assert sd.geometry_path == abi.PT_GEOM_GRID and sd.grid_kernel_build == 1
        t.set_geometry_path(abi.PT_GEOM_SCALAR)
        dl, sdl = render(t, p)
    finally:
        t.set_debug_overlay(False)
        t.set_geometry_path(abi.PT_GEOM_GRID)
    assert_bit_equal(dbg, dl, "overlay build (list walk)")
    assert sd.segments == sdl.segments
    # roulette changes the estimator: its frame is compared with the list walk's roulette frame
    t.set_russian_roulette(2)
    try:
        rr, sr = render(t, p)
        assert sr.geometry_path == abi.PT_GEOM_GRID and sr.grid_kernel_build == 1
        t.set_geometry_path(abi.PT_GEOM_SCALAR)
        rl, sl = render(t, p)
    finally:
        t.set_russian_roulette(0)
    assert_bit_equal(rr, rl, "roulette build (list walk)")
    assert sr.segments == sl.segments


def test_a_grid_of_several_layers_with_long_cells(ora):
    sph = clustered_layers_field()
    rc, g = build(sph)
    assert rc == 0 and int(g["n"][1]) > 1, g["n"]
    cnt = counts_of(g)
    assert cnt.max() >= 9 and ((cnt >= 5) & (cnt <= 8)).any() and (cnt == 0).any(), sorted(set(int(c) for c in cnt))
    c0, s0 = g["c0"].astype(np.float64), float(g["s0"])
    t = PathTracer(W, H)
    t.set_spheres(sph)
    try:
        for spp, rho, towards in ((2, 0.6, (0.8, 0.06, 0.6)), (3, 1.6, (0.15, 0.95, 0.27))):
            d = np.asarray(towards) / np.linalg.norm(towards)
            p = look(W, H, spp, 8, c0 + rho * s0 * d, c0, 55.0, 2.0 * s0)
            check_against_list_and_oracle(ora, t, sph, p, "several layers, rho %g" % rho, 1, 0)
    finally:
        t.close()


def staging_kind(n_cells, n_entries, n_layers_y):
    """pt_geom_plan.hpp grid_staging + grid_walk_flat through tests/grid_flat_shim.cpp: (build, flat)"""
    if not staging_kind.lib:
        so = os.path.join(tempfile.mkdtemp(prefix="grid_records_gpu_"), "grid_flat_shim.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I", os.path.join(os.path.dirname(HERE), "include"),
                               os.path.join(HERE, "grid_flat_shim.cpp"), "-o", so])
        lib = C.CDLL(so)
        lib.shim_flat_after_staging.restype = C.c_int
        lib.shim_flat_after_staging.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_int]
        staging_kind.lib.append(lib)
    v = staging_kind.lib[0].shim_flat_after_staging(n_cells, n_entries, n_layers_y, 0, 0)
    return v // 16, v % 16


staging_kind.lib = []


def big_field(n):
    s = random_field(n, 41, extent=0.32 * np.sqrt(n), rmax=0.3, giants=1)
    s["center"][0] = (0.0, -1000.0, 0.0)
    s["center"][1:, 1] = np.abs(s["radius"][1:])
    return s


def test_the_smallest_field_whose_entries_are_gathered(ora):
    """the cells build (cell records staged, entries gathered from L2) at the first size, in steps of 250 spheres, whose grid
    does not fit the LDS whole — a one-layer grid, whose staged records are counted in the ring layout"""
    found = None
    for n in range(1000, 9001, 250):
        sph = big_field(n)
        rc, g = build(sph, runs=True)
        assert rc == 0
        nn = [int(x) for x in g["n"]]
        staged = (nn[0] + 2) * (nn[2] + 2) if nn[1] == 1 else nn[0] * nn[1] * nn[2]
        if staging_kind(staged, g["n_entries"], nn[1])[0] == 2:
            found = (n, sph, g)
            break
    assert found is not None
    n, sph, g = found
    cnt = counts_of(g)
    assert cnt.max() >= 5 and (cnt == 0).any() and (cnt == 4).any()
    c0, s0 = g["c0"].astype(np.float64), float(g["s0"])
    t = PathTracer(W, H)
    t.set_spheres(sph)
    try:
        d = np.asarray([0.5, 0.5, 0.7]) / np.linalg.norm([0.5, 0.5, 0.7])
        p = look(W, H, 2, 8, c0 + 0.8 * s0 * d, c0, 45.0, 2.0 * s0)
        check_against_list_and_oracle(ora, t, sph, p, "field of %d spheres" % n, 2, 0)
    finally:
        t.close()
