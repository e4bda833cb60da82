"""GPU parity of the one-layer grid walk (pt_trace_kernel_grid: the two-axis walk of csrc/pt_grid_walk.hpp on a grid of
nx x 1 x nz cells) and of its sibling for grids of several layers (pt_trace_kernel_grid_layers).

(a) Flat fields of three sizes — spheres standing on a ground, which pt_grid.hpp grids in ONE layer along y — at every margin
    class tests/test_gpu_grid_classes.py walks, seen from inside the field, from above, from just inside the rim of the class's
    near region and from just outside it (no refit: below the largest class the view is then stale and the launch goes to a
    gathering build, three axes; at the largest class both walk flat, the outside camera's primary rays on the far path).  The
    bar is the scalar list walk's frame and segment count, bit for bit.  PtStats says which kernel a launch gets
    (grid_kernel_build, grid_walk_flat): asserted for every render, and the other way round on a grid with n[1] > 1.
(b) The measuring twins (pt_trace_kernel_grid_count / _grid_layers_count) take the same walk as the kernels they measure.
"""
import math

import numpy as np
import pytest

from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd.tracer import PathTracer
from test_bvh import random_field
from test_gpu_grid_classes import assert_bit_equal, camera, need_factor
from test_grid import CLASSES, build, near_of

pytestmark = pytest.mark.gpu

W, H = 96, 54


def flat_field(n, seed, extent):
    """n - 1 small spheres standing on a ground (a giant under them): one layer of cells"""
    s = random_field(n, seed, extent=extent, rmax=0.3, giants=1)
    s["center"][0] = (0.0, -1000.0, 0.0)
    s["center"][1:, 1] = np.abs(s["radius"][1:])
    return s


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def render(t, p):
    t.set_params(p)
    t.reserve_passes(1)
    t.reset()
    t.render_passes(1)
    return t.accum(), t.stats()


FIELDS = [("field120", 120, 31, 6.0), ("field400", 400, 32, 12.0), ("field1500", 1500, 33, 20.0)]


@pytest.mark.parametrize("case", FIELDS, ids=[c[0] for c in FIELDS])
def test_flat_fields_at_every_class_from_inside_above_and_outside_equal_the_list_walk(case):
    name, n, seed, extent = case
    sph = flat_field(n, seed, extent)
    t = PathTracer(W, H)
    t.set_geometry_path(abi.PT_GEOM_GRID)
    t.set_grid_fit(True)  # the class the camera needs, unmeasured
    t.set_spheres(sph)
    lst = PathTracer(W, H)
    lst.set_geometry_path(abi.PT_GEOM_SCALAR)
    lst.set_spheres(sph)
    flat_launches = other_launches = 0
    try:
        for f in CLASSES:
            rc, g = build(sph, near_factor=f)
            assert rc == 0 and tuple(int(x) for x in g["n"])[1] == 1, (name, f, g["n"])
            c0, s0, rim = g["c0"].astype(np.float64), float(g["s0"]), math.sqrt(float(g["r2_near"]))
            rho_a = 0.98 * (f / 1.01 - 1.0) * 0.9999 * s0
            assert need_factor(rho_a, s0) == f
            above = unit([0.15, 0.95, 0.27])
            t.set_params(camera(W, H, 1, 1, c0, s0, rho_a, above))
            t.reserve_passes(1)
            t.tune(1)
            st = t.stats()
            assert st.grid_near_factor == f and st.grid_fit_stale == 0, (name, f, st.grid_near_factor)
            assert tuple(st.grid_cells) == tuple(int(x) for x in g["n"]) and st.grid_cells[1] == 1, (name, f, tuple(st.grid_cells))
            # (camera, distance from the grid's middle, direction to it, inside the near region?)
            views = [("inside", 0.45 * s0, unit([0.8, 0.06, 0.6]), True),
                     ("above", rho_a, above, True),
                     ("rim", rim * (1.0 - 2e-5), unit([0.62, 0.45, 0.64]), True),
                     ("outside", rim * (1.0 + 1e-4), unit([0.62, 0.45, 0.64]), False)]
            for cam, rho, towards, inside in views:
                for spp, depth in ((1, 1), (2, 8)):
                    p = camera(W, H, spp, depth, c0, s0, rho, towards)
                    o = np.asarray([list(p.camera_origin)], np.float32)
                    assert bool(near_of(g, o)[0]) == inside, (name, f, cam)
                    got, st = render(t, p)
                    what = "%s class %g camera %s spp %d depth %d" % (name, f, cam, spp, depth)
                    assert st.grid_near_factor == f and st.geometry_path == abi.PT_GEOM_GRID, what  # no refit
                    stale = st.grid_fit_stale == 1
                    # (at the rim the camera needs a larger class than the one in place — the need carries 1 % of slack —, so
                    # the host calls the view stale on either side of it; the largest class is the most any camera needs)
                    assert stale == (cam in ("rim", "outside") and f != CLASSES[-1]), (what, st.grid_fit_stale)
                    # the LDS-staged build of a one-layer grid IS the flat walk; a stale view goes to a gathering build
                    assert st.grid_kernel_build == (2 if stale else 1), (what, st.grid_kernel_build)
                    assert st.grid_walk_flat == (0 if stale else 1), (what, st.grid_walk_flat)
                    if depth == 1:
                        assert (st.far_rays > 0) == (not inside), (what, st.far_rays)
                    ref, rs = render(lst, p)
                    assert_bit_equal(got, ref, what + " (list walk)")
                    assert st.segments == rs.segments, (what, st.segments, rs.segments)
                    assert st.segments >= W * H * spp
                    flat_launches += int(st.grid_walk_flat)
                    other_launches += 1 - int(st.grid_walk_flat)
    finally:
        t.close()
        lst.close()
    assert flat_launches == 4 * len(CLASSES) + 4 and other_launches == 4 * (len(CLASSES) - 1), (flat_launches, other_launches)


def test_a_grid_of_several_layers_gets_the_three_axis_kernel():
    sph = random_field(300, 1)  # spheres spread along y too
    rc, g = build(sph)
    assert rc == 0 and g["n"][1] > 1, g["n"]
    c0, s0 = g["c0"].astype(np.float64), float(g["s0"])
    t = PathTracer(W, H)
    t.set_geometry_path(abi.PT_GEOM_GRID)
    t.set_spheres(sph)
    lst = PathTracer(W, H)
    lst.set_geometry_path(abi.PT_GEOM_SCALAR)
    lst.set_spheres(sph)
    try:
        for rho, towards in ((0.6 * s0, unit([0.8, 0.06, 0.6])), (1.6 * s0, unit([0.15, 0.95, 0.27]))):
            p = camera(W, H, 2, 8, c0, s0, rho, towards)
            got, st = render(t, p)
            assert st.geometry_path == abi.PT_GEOM_GRID and st.grid_cells[1] > 1 and st.grid_fit_stale != 1
            assert st.grid_kernel_build == 1 and st.grid_walk_flat == 0, (st.grid_kernel_build, st.grid_walk_flat)
            ref, rs = render(lst, p)
            assert_bit_equal(got, ref, "several layers, rho %g" % rho)
            assert st.segments == rs.segments
    finally:
        t.close()
        lst.close()


@pytest.mark.parametrize("layers", [False, True], ids=["one_layer", "several_layers"])
def test_the_measuring_twin_takes_the_walk_of_the_kernel_it_measures(layers):
    sph = random_field(300, 1) if layers else flat_field(400, 32, 12.0)
    rc, g = build(sph)
    assert rc == 0 and (g["n"][1] > 1) == layers
    c0, s0 = g["c0"].astype(np.float64), float(g["s0"])
    t = PathTracer(128, 72)
    t.set_geometry_path(abi.PT_GEOM_GRID)
    t.set_spheres(sph)
    try:
        for rho, towards in ((0.6 * s0, unit([0.8, 0.06, 0.6])), (1.6 * s0, unit([0.15, 0.95, 0.27]))):
            p = camera(128, 72, 4, 50, c0, s0, rho, towards)
            t.set_count_work(False)
            got, st = render(t, p)
            assert st.grid_kernel_build == 1 and st.grid_walk_flat == (0 if layers else 1) and sum(st.work) == 0
            t.set_count_work(True)
            twin, sw = render(t, p)
            assert sw.grid_kernel_build == 1 and sw.grid_walk_flat == st.grid_walk_flat
            assert_bit_equal(twin, got, "measuring twin vs timed kernel, rho %g" % rho)
            assert sw.segments == st.segments
            w = sw.work
            assert w[0] > 0 and w[2] > 0 and w[6] > 0 and w[6] * 64 >= sw.segments
            assert w[1] <= 64 * w[0] and w[3] <= 64 * w[2] and w[5] <= 64 * w[4]
    finally:
        t.close()
