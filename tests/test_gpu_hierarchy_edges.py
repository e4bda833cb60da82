"""The hierarchy walk (PT_GEOM_BVH) at the edges of what its kernels stage in the LDS, and at its 16-bit limits.

A walk kernel stages the scene into the LDS and parks every lane's path state right behind it (csrc/pt_scene.hpp stage, park_of:
lds_scene_bytes); links, leaf numbers and both per-lane queues of the walk are 16 bits wide (csrc/pt_bvh.hpp, pt_bvh_walk.hpp).
The sizes at which either can go wrong are prefixes of one field, found on the CPU and pinned there (tests/hierarchy_edges.py,
tests/test_bvh.py):

  M_BVH_FULL     pt_trace_kernel_bvh with nodes and slots filling the room beside the parked state (to the byte)
  M_NODES_FIRST  the smallest scene of pt_trace_kernel_bvh_nodes, one sphere more
  M_NODES_FULL   pt_trace_kernel_bvh_nodes with the packed nodes filling the room
  M_GMEM_FIRST   the smallest scene of pt_trace_kernel_bvh_gmem
  M_LIMIT        65 528 slots and 32 761 nodes: the largest numbers the queues and links ever hold
  M_OVER         no hierarchy any more: PT_GEOM_BVH renders through the list walk

Each at 48x27, 2 samples, 2 passes in one launch, depth 8, lens on: the row the launch was (tests/trace_builds.py), the whole
frame against PT_GEOM_SCALAR on the same scene (bits and segments), and a 16x10 window in the middle against the CPU oracle.
Where the staged scene fills the room the parked state ends at the end of the LDS: there also lockstep and always-carrying
walks (PT_OPT_CARRY_LANES 0 and 64) and PT_OPT_COUNT_WORK.  Tolerance: none."""
import os

import numpy as np
import pytest

import hierarchy_edges as E
from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd.tracer import PathTracer
from test_gpu_plain_builds import assert_bit_equal, describe, gpu, with_lens_and_step
from trace_builds import WALK_LDS_ROOM, hierarchy_staging, row_of, twin_of

pytestmark = pytest.mark.gpu

ORACLE_THREADS = min(16, os.cpu_count() or 1)
W, H, N_PASSES = 48, 27, 2
WINDOW = (16, 32, 8, 18)  # x0, x1, y0, y1
REPORT = {}


def context(sph, path, carry_lanes=None, count_work=False):
    t = PathTracer(W, H)
    t.set_geometry_path(path)
    if carry_lanes is not None:
        t.set_carry_lanes(carry_lanes)
    if count_work:
        t.set_count_work(True)
    t.set_spheres(sph)
    return t


@pytest.fixture(scope="module")
def listed():
    """per edge: the scene, its uniforms and the list walk's whole frame (PT_GEOM_SCALAR), made once and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            sc = E.scene(getattr(E, name), W, H, 2, N_PASSES, 8)
            p = with_lens_and_step(sc.params)
            t = context(sc.spheres, abi.PT_GEOM_SCALAR)
            try:
                ref, st = gpu(t, p, N_PASSES)
                assert st.geometry_path == abi.PT_GEOM_SCALAR and row_of(st) == ("scalar" if len(sc.spheres) <= 10232 else "scalar_nolds")
                ref.setflags(write=False)
                cache[name] = (sc.spheres, p, ref, int(st.segments))
            finally:
                t.close()
        return cache[name]
    return get


def assert_window_is_the_oracles(ora, sph, p, got, what):
    x0, x1, y0, y1 = WINDOW
    ref, _ = ora.render(sph, p, N_PASSES, window=WINDOW, nthreads=ORACLE_THREADS)
    assert_bit_equal(got[y0:y1, x0:x1], ref[y0:y1, x0:x1], "%s: window against the oracle" % what)
    assert np.all(ref[y0:y1, x0:x1, 3] == 2 * N_PASSES)


@pytest.mark.parametrize("name", ["M_BVH_FULL", "M_NODES_FIRST", "M_NODES_FULL", "M_GMEM_FIRST", "M_LIMIT"])
def test_the_hierarchy_at_an_edge_equals_the_list_walk_and_the_oracle(ora, listed, name):
    row = E.ROW_AT[name]
    sph, p, ref, seg = listed(name)
    assert len(sph) == getattr(E, name) + 1
    runs = [dict()]
    if name in ("M_BVH_FULL", "M_NODES_FULL"):  # parked state and staged scene meet at the end of the LDS
        runs += [dict(carry_lanes=0), dict(carry_lanes=64), dict(count_work=True)]
    for options in runs:
        what = "%s %s" % (name, options or "")
        t = context(sph, abi.PT_GEOM_BVH, **options)
        try:
            got, st = gpu(t, p, N_PASSES)
            assert st.geometry_path == abi.PT_GEOM_BVH and st.render_launches == 1
            assert row_of(st) == row, (what, row_of(st), describe(st))
            kind, staged = hierarchy_staging(st.bvh_nodes, st.bvh_slots)
            if name in ("M_BVH_FULL", "M_NODES_FULL"):
                assert WALK_LDS_ROOM - E.NEAR_BYTES <= staged <= WALK_LDS_ROOM, (what, staged)
            if name == "M_LIMIT":
                assert E.MAX_SLOTS - E.NEAR_SLOTS <= st.bvh_slots <= E.MAX_SLOTS and st.bvh_nodes <= E.MAX_NODES, describe(st)
            if options.get("count_work"):
                assert t.last_trace_build() == abi.BUILD_TWIN
                work = list(st.work)
                if twin_of(row) is not None:
                    assert work[6] > 0 and work[0] > 0 and work[1] <= 64 * work[0], work
                else:
                    assert sum(work) == 0, work
            else:
                assert t.last_trace_build() == abi.BUILD_PLAIN
            assert_bit_equal(got, ref, "%s: whole frame against the list walk" % what)
            assert st.segments == seg, (what, st.segments, seg)
            if not options:
                assert_window_is_the_oracles(ora, sph, p, got, what)
                REPORT[name] = "%s: %d spheres, %d nodes, %d slots, %d bytes staged" % (row, len(sph), st.bvh_nodes, st.bvh_slots, staged)
        finally:
            t.close()


def test_a_scene_beyond_the_limits_renders_through_the_list_walk(ora, listed):
    """M_OVER: 0x10000 slots and more get no hierarchy (csrc/pt_bvh.hpp); a context forced to PT_GEOM_BVH falls back to
    PT_GEOM_SCALAR (csrc/pt_geom_plan.hpp) and renders the list walk's frame, which is the oracle's."""
    sph, p, ref, seg = listed("M_OVER")
    t = context(sph, abi.PT_GEOM_BVH)
    try:
        got, st = gpu(t, p, N_PASSES)
        assert st.geometry_path == abi.PT_GEOM_SCALAR and st.bvh_nodes == 0 and st.bvh_slots == 0, describe(st)
        assert row_of(st) == "scalar_nolds" and t.last_trace_build() == abi.BUILD_PLAIN
        assert_bit_equal(got, ref, "M_OVER: PT_GEOM_BVH against the list walk")
        assert st.segments == seg
        assert_window_is_the_oracles(ora, sph, p, got, "M_OVER")
    finally:
        t.close()


def test_the_five_edges_were_rendered():
    """(runs after the tests above)"""
    print("the hierarchy at its edges\n" + "\n".join("  %-14s %s" % (k, REPORT.get(k, "-")) for k in E.ROW_AT))
    assert sorted(REPORT) == sorted(E.ROW_AT)
    assert [REPORT[k].split(":")[0] for k in ("M_BVH_FULL", "M_NODES_FIRST", "M_NODES_FULL", "M_GMEM_FIRST", "M_LIMIT")] == \
        ["bvh", "bvh_nodes", "bvh_nodes", "bvh_gmem", "bvh_gmem"]
