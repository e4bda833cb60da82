"""The look-ahead refill (csrc/pt_deal.hpp, csrc/pt_refill.hpp) on the device, at the launch shapes where the dealing can go wrong.

Every lane of a trace kernel holds one decoded next item beside the one it works on; it takes it the moment its item ends
(promote), and the item decode runs — for every lane whose next slot is empty — only when some lane has neither.  That
only schedules, so every case here is held to the CPU oracle bit for bit (equal uint32 views of the accumulation buffer) and
to its segment count, and each names the kernel it ran (tests/trace_builds.py).  The shapes are the smallest at which a
branch of the dealing is taken, not a workload's:

  fewer items than a wave has lanes (5 x 3): most lanes never get an item, the next slots stay empty to the end;
  partial tiles on both edges (67 x 37): dropped items land in next slots, the item count is no multiple of a reservation;
  items of one to three segments (64 x 8, depth 3, 1 and 16 spp): every lane promotes almost every step;
  each queue mode — static, grouped, shared —, the mode taken from the launch plan (csrc/pt_launch_plan.hpp through
  tests/launch_plan_shim.cpp, the arithmetic the library calls) with the launch's own numbers;
  launches the plan does NOT fill ahead (items of 32 samples or more, few per lane: the decode serves lanes directly);
  a band partition (K.band_count > 1 in the decode);
  every kernel family once, and the roulette build against the oracle's roulette;
  PT_OPT_REFILL_MIN at 1, 4 and 64: the option is stored and read back, and inert;
  a replayed frame series (pt_render_frames) against host-issued frames: the decode reads the device's frame counter one item
  early, and the counter is constant within a launch (the advance kernel runs between trace launches).
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from ray_tracer_webgl_amd import abi, scenes
from test_gpu_fuzz import random_scene
from test_gpu_plain_builds import assert_bit_equal, assert_plain, context, gpu, oracle, with_lens_and_step
from trace_builds import build_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHARED, STATIC, GROUPED = 0, 1, 2  # PtKernelArgs.queue_static


def cover(w, h, spp, passes, depth=8):
    return scenes.config2(w, h, spp, passes, depth)


def run_case(ora, sc, path, row, passes=None, band=None):
    """one launch of every pass against the oracle; returns (uniforms, statistics)"""
    p = with_lens_and_step(sc.params)
    if band:
        p.band_rows, p.band_index, p.band_count = band
    n = passes or sc.n_passes
    ref, seg = oracle(ora, sc.spheres, p, n)
    t = context(sc.spheres, p.width, p.height, path)
    try:
        got, st = gpu(t, p, n)
        assert_plain(t, st, row)
        assert st.render_launches == 1
        assert_bit_equal(got, ref, "%s %dx%d, %d passes of %d spp" % (row, p.width, p.height, n, p.samples_per_pixel))
        assert st.segments == seg, (row, st.segments, seg)
    finally:
        t.close()
    return p, st


# ------------------------------------------------------------------------------------------- shapes of the dealing
@pytest.mark.parametrize("path,row", [(abi.PT_GEOM_GRID, "grid"), (abi.PT_GEOM_SCALAR, "scalar")], ids=["grid", "scalar"])
def test_fewer_items_than_a_wave_has_lanes(ora, path, row):
    """5 x 3 pixels, one pass: one tile, 64 items of which 15 lie in the image — most lanes never get an item, no next slot
    is ever filled twice, every wave ends on a dry queue"""
    run_case(ora, cover(5, 3, 2, 1), path, row)


@pytest.mark.parametrize("path,row", [(abi.PT_GEOM_GRID, "grid"), (abi.PT_GEOM_BVH, "bvh"), (abi.PT_GEOM_SCALAR, "scalar")],
                         ids=["grid", "hierarchy", "scalar"])
def test_partial_tiles_on_both_edges(ora, path, row):
    """67 x 37, three passes of 2 spp: 9 x 5 tiles, the last column 3 pixels wide and the last row 5 high — dropped items leave
    next slots empty; 8 640 items are 135 reservations of 64, no multiple of any larger reservation size"""
    p, _ = run_case(ora, cover(67, 37, 2, 3), path, row)
    assert (p.width % 8, p.height % 8) == (3, 5)


@pytest.mark.parametrize("spp", [1, 16])
def test_items_of_a_few_segments(ora, spp):
    """64 x 8, one pass, paths of at most three segments: at 1 spp an item is one to three wave steps, so every lane promotes
    almost every step and the decode runs almost every step; at 16 spp the same pixels with items sixteen times as long"""
    run_case(ora, cover(64, 8, spp, 1, depth=3), abi.PT_GEOM_GRID, "grid")
    run_case(ora, cover(64, 8, spp, 1, depth=3), abi.PT_GEOM_SCALAR, "scalar")


# ------------------------------------------------------------------------------------------- the three queue modes
@pytest.fixture(scope="module")
def plan_shim():
    so = os.path.join(tempfile.mkdtemp(prefix="refill_plan_"), "liblaunch_plan_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", os.path.join(HERE, "launch_plan_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.launch_plan.restype = C.c_int
    lib.launch_plan.argtypes = [C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_uint32,
                                C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]
    so = os.path.join(os.path.dirname(so), "libdeal_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", os.path.join(HERE, "deal_shim.cpp"), "-o", so])
    lib.deal = C.CDLL(so)
    lib.deal.deal_plan_refill_ahead.restype = C.c_uint32
    lib.deal.deal_plan_refill_ahead.argtypes = [C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_uint32]
    return lib


def queue_mode(lib, w, h, spp, passes):
    """the dealing mode of a grid-walk launch of this shape: 512-thread workgroups, three resident per CU (the launches here want
    fewer workgroups than two per CU, so the grid is the workgroups wanted whether two or three are resident)"""
    cus = 256  # an MI355X
    items = ((w + 7) // 8) * ((h + 7) // 8) * 64 * passes
    assert (items + 511) // 512 <= 2 * cus
    out = (C.c_uint32 * 7)()
    assert lib.launch_plan(items, spp, passes, 512, 3, cus, 1, 0, 0, (C.c_int * 9)(), out) == 0
    return out[1], lib.deal.deal_plan_refill_ahead(items, spp, passes, 512, 3, cus, 1, 0)


# (name, width, height, spp, passes, mode, filled ahead).  The first three are the shapes of the issue that asked for these tests; by the launch
# plan a launch reaches the SHARED queue from 448 samples per lane on, which 32 passes of 16 spp at 96 x 54 do not have (a launch
# below a full machine has as many lanes as items: 16 samples per lane, the grouped queue) — so that shape is kept and named for
# what it runs, and the shared queue gets the smallest launch that reaches it: 512 items of 448 spp, eight waves on one head
# counter with reservations of 32 items, half a wave's ballot — one 448-spp item per lane, which the plan does not fill ahead
# (the shared queue WITH filled slots needs a full machine's launch: tests/test_gpu_properties.py renders config 2 at its size
# against the oracle, and tests/test_deal.py runs that combination on the CPU).  Then launches of long items in the other two
# modes, served directly, one of them with partial tiles.
QUEUE_CASES = [
    ("static_4spp_frame", 96, 54, 4, 1, STATIC, 1),
    ("grouped_4x16", 96, 54, 16, 4, GROUPED, 1),
    ("grouped_32x16", 96, 54, 16, 32, GROUPED, 1),
    ("shared_1x448", 32, 16, 448, 1, SHARED, 0),
    ("grouped_direct_1x64", 96, 54, 64, 1, GROUPED, 0),
    ("grouped_direct_edges_2x32", 67, 37, 32, 2, GROUPED, 0),
    ("static_direct_1x32", 5, 3, 32, 1, STATIC, 0),
]


@pytest.mark.parametrize("case", QUEUE_CASES, ids=[c[0] for c in QUEUE_CASES])
def test_each_queue_mode(ora, plan_shim, case):
    name, w, h, spp, passes, mode, ahead = case
    assert queue_mode(plan_shim, w, h, spp, passes) == (mode, ahead), name
    run_case(ora, cover(w, h, spp, passes), abi.PT_GEOM_GRID, "grid")


def test_a_band_partition(ora):
    """band 1 of 3, four rows each, at 40 x 26: the decode's band arithmetic, on items decoded ahead"""
    p, st = run_case(ora, cover(40, 26, 2, 2), abi.PT_GEOM_GRID, "grid", band=(4, 1, 3))
    assert st.local_rows == len(abi.owned_rows(26, 4, 1, 3)) == 8


# ------------------------------------------------------------------------------------------- every kernel family
def field(n):
    return lambda: scenes.config5(96, 54, 4, 2, 8, n=n)


FAMILIES = [
    ("list_lds", lambda: cover(96, 54, 4, 2), abi.PT_GEOM_LDS),
    ("scalar", lambda: cover(96, 54, 4, 2), abi.PT_GEOM_SCALAR),
    ("small_t1", lambda: random_scene(np.random.default_rng(47100), 9, 96, 54, 4, 8, 2), abi.PT_GEOM_SMALL),
    ("bvh", lambda: cover(96, 54, 4, 2), abi.PT_GEOM_BVH),
    ("grid", lambda: cover(96, 54, 4, 2), abi.PT_GEOM_GRID),   # one layer of cells: the two-axis walk
    ("grid_layers", field(1500), abi.PT_GEOM_GRID),
    ("grid_cells", field(10000), abi.PT_GEOM_GRID),
    ("grid_gmem", field(52000), abi.PT_GEOM_GRID),             # cells and entries gathered from global memory
]


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_every_kernel_family(ora, case):
    """96 x 54, two passes of 4 spp, through each family of trace kernels: they share the body, each is a build of its own"""
    row, make, path = case
    sc = make()
    assert (sc.params.width, sc.params.height, sc.params.samples_per_pixel, sc.n_passes) == (96, 54, 4, 2)
    run_case(ora, sc, path, row)


def test_the_roulette_build(ora):
    """pt_trace_kernel_grid_rr against the oracle's roulette (k = 3): roulette ends items early, lanes promote more often"""
    from test_gpu_roulette_exact import gpu as gpu_rr, oracle as oracle_rr

    sc = cover(96, 54, 4, 2)
    p = with_lens_and_step(sc.params)
    ref, seg = oracle_rr(ora, sc.spheres, p, 2, 3)
    t = context(sc.spheres, 96, 54, abi.PT_GEOM_GRID)
    try:
        got, st = gpu_rr(t, p, 3, 2)
        assert build_of(st, "_rr") == "grid_rr" and t.last_trace_build() != abi.BUILD_PLAIN
        assert_bit_equal(got, ref, "grid_rr, k = 3")
        assert st.segments == seg
    finally:
        t.close()


# ------------------------------------------------------------------------------------------- the option is inert
def test_refill_min_is_kept_and_inert(ora):
    sc = cover(96, 54, 4, 2)
    p = with_lens_and_step(sc.params)
    ref, seg = oracle(ora, sc.spheres, p, 2)
    for lanes in (1, 4, 64):
        for path, row in ((abi.PT_GEOM_GRID, "grid"), (abi.PT_GEOM_SCALAR, "scalar")):
            t = context(sc.spheres, 96, 54, path)
            try:
                t.set_refill_min(lanes)
                got, st = gpu(t, p, 2)
                assert_plain(t, st, row)
                assert_bit_equal(got, ref, "%s, refill_min %d" % (row, lanes))
                assert st.segments == seg
            finally:
                t.close()


# ------------------------------------------------------------------------------------------- replayed frames
@pytest.mark.parametrize("which", ["grid", "small"])
def test_replayed_frames_equal_host_issued_frames(which):
    """eight ticks at 160 x 90: pt_render_frames (groups of frames traced as the passes of one launch, u_time counted on the
    device: frame_k in the item decode) against eight pt_render_frame calls whose uniforms the host steps — canvas, both
    textures and the segment count.  With the look-ahead the decode of a lane's NEXT item reads the frame counter while the lane
    still works on its current one; the counter is advanced by a kernel of its own between trace launches, never within one,
    so both series see the same u_time for every item."""
    n_ticks, t0, dt = 8, 100.0, 16.5
    if which == "grid":
        sc, path, row = cover(160, 90, 1, 1), abi.PT_GEOM_GRID, "grid"
    else:
        sc, path, row = scenes.default_scene(160, 90, 1, 8, 1), abi.PT_GEOM_SMALL, "small_t1"
    sph, (w, h) = sc.spheres, (160, 90)
    p = with_lens_and_step(sc.params)
    p.should_average, p.last_frame_weight, p.render_count = 1, 1.0, 1
    p.time, p.time_step, p.first_pass = t0, dt, 0
    rc_max = 100000
    a, b = context(sph, w, h, path), context(sph, w, h, path)
    try:
        for t in (a, b):
            t.clear_textures()
        for k in range(n_ticks):
            q = p.copy()
            q.time, q.render_count = t0 + dt * k, min(p.render_count + k, rc_max)
            a.set_params(q)
            a.render_frame(k)
            assert_plain(a, a.stats(), row)
        b.set_params(p)
        b.render_frames(0, rc_max, n_ticks)
        assert_plain(b, b.stats(), row)
        assert np.array_equal(a.read_canvas(), b.read_canvas()), "%s: canvas after %d replayed frames" % (row, n_ticks)
        for k in range(2):
            assert np.array_equal(a.read_texture(k), b.read_texture(k)), "%s: texture %d" % (row, k)
        assert a.stats().segments == b.stats().segments > 0
        assert len(np.unique(a.read_canvas()[..., :3])) > 16  # (a picture, not a constant)
    finally:
        a.close()
        b.close()
