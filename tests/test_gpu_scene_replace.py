"""One context, a SEQUENCE of scenes: pt_set_spheres replaces the list, the hierarchy and the grid in buffers that only grow, so
after each call everything the kernels read must be the new scene's — a buffer, a head or a per-slot array left over from the
scene before would show here.

After every set_spheres the accumulation is bit-equal to the oracle's (with the debug overlay on: to tests/overlay_ref.c's),
PtStats.segments is the reference's count, and the stats that describe the structures in place — n_spheres, geometry_path,
bvh_nodes, bvh_slots, grid_cells, grid_kernel_build — are those of a fresh context given only that scene.  The sequences go
large -> small -> large (and one layer of cells -> several layers with FEWER cells -> one layer), so that every buffer is
reused below its capacity once.  96 x 54, 2 spp, depth 8, 2 passes; tolerance: none.
"""
import numpy as np
import pytest

import overlay_ref as R
from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer
from test_gpu_fuzz import random_scene

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH, PASSES = 96, 54, 2, 8, 2
STAT_FIELDS = ("n_spheres", "geometry_path", "bvh_nodes", "bvh_slots", "grid_cells", "grid_kernel_build")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rand(n, seed):
    return random_scene(np.random.default_rng(seed), n, W, H, SPP, DEPTH, PASSES)


def one_layer():
    """spheres on a ground plane (the cover scene): a grid of 16 x 1 x 16 cells, walked along two axes through the ring layout"""
    return scenes.config2(W, H, SPP, PASSES, DEPTH)


def volume():
    """a random scene whose grid has several layers of cells, and fewer cells than one_layer()'s"""
    sc = rand(130, 31010)
    sc.selected = 33  # (the overlay's selection: a sphere this camera sees the outline of; its middle ray starts inside one)
    return sc


def irregular():
    sc = rand(40, 31001)
    sc.spheres["center"][17] = (2e15, 0.0, 0.0)  # no structure for this scene; the kernels take the literal path
    return sc


def described(st):
    return tuple(tuple(int(v) for v in getattr(st, f)) if f == "grid_cells" else int(getattr(st, f)) for f in STAT_FIELDS)


def render(t, sc, overlay=None):
    """the scene through context t, from set_spheres on: (accumulation, stats)"""
    t.set_spheres(sc.spheres)
    if overlay is not None:
        t.set_debug_overlay(True, overlay[0], overlay[1])  # (on already: this scene's selection and cursor)
    t.set_params(sc.params)
    t.reserve_passes(PASSES)
    t.reset()
    t.render_passes(PASSES)
    return t.accum(), t.stats()


def pick(sc):
    """(selected uuid, cursor point) for the overlay: sphere sc.selected (where a scene names one) with the cursor on its top,
    else what the middle ray hits"""
    k = getattr(sc, "selected", None)
    if k is None:
        return R.center_pick(sc.spheres, sc.params)
    c, r = sc.spheres["center"][k], abs(float(sc.spheres["radius"][k]))
    return int(sc.spheres["uuid"][k]), (float(c[0]), float(c[1]) + r, float(c[2]))


def run_sequence(ora, path, seq, with_overlay=False):
    """seq: (name, scene) in order, a name that returns standing for the same scene.  Returns name -> stats of the kept context."""
    expected = {}
    for name, sc in seq:
        if name in expected:
            continue
        fresh = PathTracer(W, H)
        try:
            if path is not None:
                fresh.set_geometry_path(path)
            if with_overlay:
                overlay = pick(sc)
                fresh.set_debug_overlay(True, *overlay)
                ref, tally, _ = R.render(sc.spheres, sc.params, PASSES, overlay)
                plain, _ = ora.render(sc.spheres, sc.params, PASSES)
                assert tally["red_paths"] > 0 and not np.array_equal(bits(ref), bits(plain)), name  # the uuids matter to this image
                seg = tally["segments"]
            else:
                overlay = None
                ref, seg = ora.render(sc.spheres, sc.params, PASSES)
            got, st = render(fresh, sc, overlay)
            assert np.array_equal(bits(got), bits(ref)) and st.segments == seg, "a fresh context on %s" % name
            expected[name] = (ref, seg, described(st), overlay)
        finally:
            fresh.close()
    out = {}
    t = PathTracer(W, H)
    try:
        if path is not None:
            t.set_geometry_path(path)
        if with_overlay:
            t.set_debug_overlay(True, *expected[seq[0][0]][3])  # on before the first scene, and throughout
        for k, (name, sc) in enumerate(seq):
            ref, seg, want, overlay = expected[name]
            got, st = render(t, sc, overlay)
            g, r = bits(got), bits(ref)
            assert np.array_equal(g, r), "scene %d (%s): %d of %d values differ" % (k, name, (g != r).sum(), g.size)
            assert st.segments == seg, (k, name, st.segments, seg)
            assert described(st) == want, (k, name, described(st), want)
            if with_overlay:
                assert t.last_trace_build() == abi.BUILD_DEBUG_OVERLAY
            out[name] = st
    finally:
        t.close()
    return out


def test_the_list_shrinks_to_the_small_list_kernel_and_grows_again(ora):
    big, small = rand(40, 31001), rand(3, 31003)
    st = run_sequence(ora, None, [("40", big), ("3", small), ("40", big)])
    assert st["40"].n_spheres == 40 and st["40"].bvh_nodes > 0 and st["40"].grid_cells[0] > 0
    assert st["3"].n_spheres == 3 and st["3"].geometry_path == abi.PT_GEOM_SMALL
    assert st["3"].bvh_nodes == 0 and tuple(st["3"].grid_cells) == (0, 0, 0)  # no structures


def test_the_hierarchy_follows_the_scene(ora):
    big, small = rand(300, 31004), rand(20, 31005)
    st = run_sequence(ora, abi.PT_GEOM_BVH, [("300", big), ("20", small), ("300", big)])
    for name in ("300", "20"):
        assert st[name].geometry_path == abi.PT_GEOM_BVH and st[name].bvh_nodes > 0
    assert st["20"].bvh_slots < st["300"].bvh_slots and st["20"].bvh_nodes < st["300"].bvh_nodes


def grid_sequence():
    return [("one layer", one_layer()), ("volume", volume()), ("one layer", one_layer())]


def check_grid_shapes(st):
    flat, vol = st["one layer"], st["volume"]
    assert flat.geometry_path == abi.PT_GEOM_GRID and vol.geometry_path == abi.PT_GEOM_GRID
    assert flat.grid_cells[1] == 1  # the ring layout is in use
    assert vol.grid_cells[1] > 1
    assert int(np.prod(vol.grid_cells)) < int(np.prod(flat.grid_cells))


def test_the_grid_follows_the_scene_between_one_layer_and_several(ora):
    st = run_sequence(ora, abi.PT_GEOM_GRID, grid_sequence())
    check_grid_shapes(st)
    assert st["one layer"].grid_walk_flat == 1 and st["volume"].grid_walk_flat == 0


def test_the_per_slot_uuids_follow_the_scene(ora):
    """the grid sequence with the debug overlay on throughout; uuids that are not list indices, and not the other scene's"""
    seq = grid_sequence()
    flat, vol = seq[0][1], seq[1][1]
    flat.spheres["uuid"] = (50 + 11 * np.arange(len(flat.spheres))).astype(np.int32)
    vol.spheres["uuid"] = (7000 + 3 * np.random.default_rng(5).permutation(len(vol.spheres))).astype(np.int32)
    seq = [("one layer", flat), ("volume", vol), ("one layer", flat)]
    st = run_sequence(ora, abi.PT_GEOM_GRID, seq, with_overlay=True)
    check_grid_shapes(st)


def test_a_scene_without_structures_between_two_that_have_them(ora):
    regular = rand(40, 31001)
    st = run_sequence(ora, abi.PT_GEOM_GRID, [("regular", regular), ("irregular", irregular()), ("regular", regular)])
    assert st["regular"].geometry_path == abi.PT_GEOM_GRID and st["regular"].bvh_nodes > 0
    odd = st["irregular"]
    assert odd.n_spheres == 40 and odd.geometry_path not in (abi.PT_GEOM_GRID, abi.PT_GEOM_BVH)
    assert odd.bvh_nodes == 0 and tuple(odd.grid_cells) == (0, 0, 0)
