"""GPU parity at the rim of every margin class of the grid walk (PT_GEOM_GRID).

pt_tune and pt_refit_grid rebuild the grid for the margin class d_near / s0 in {2.5, 3, 4, 5.5, 8, 12, 16} that the camera
needs (csrc/pt_geom_plan.hpp kNearFactors, view_need_factor); the registration margin grows with d_near^2 (csrc/pt_grid.hpp).
For each class and each of the three builds of the grid kernel (PtStats.grid_kernel_build: 1 cells and entries staged in
the LDS, 2 entries gathered from L2, 3 nothing staged) three cameras render the same scene:
  A  where the class is the one the camera needs (tune(1), unmeasured: set_grid_fit(True)),
  B  just inside the class's near region (|o - c0|^2 <= r2_near: primary rays walk the cells),
  C  just outside it (primary rays take the far path),
B and C without a refit: for every class below the largest the host then calls the view stale (grid_fit_stale 1), which
hands the launch to a build that gives far rays to the whole wave.  Each camera renders primary rays only (1 spp, depth 1:
the far-ray tally says which path they took) and full paths (2 spp, depth 8).  The bar is the oracle's bits.
"""
import math
import os

import numpy as np
import pytest

from ray_tracer_webgl_amd import _lib, abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer
from test_grid import CLASSES, build, near_of

pytestmark = pytest.mark.gpu

ORACLE_THREADS = min(16, os.cpu_count() or 1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert np.array_equal(g, r), "%s: %d of %d values differ" % (what, int((g != r).sum()), g.size)


def need_factor(rho, s0):
    """view_need_factor (csrc/pt_geom_plan.hpp) for a camera without a lens at distance rho from c0"""
    need = ((rho / 0.9999 + s0) / s0) * 1.01
    return next((f for f in CLASSES if f >= need), CLASSES[-1])


def camera(w, h, spp, depth, c0, s0, rho, towards):
    """a pinhole camera at distance rho from the grid's middle c0, looking at it, with a field of view that frames the scene.
    The focus distance (no lens: it only scales the directions) is 2 s0, so that the primary rays are regular
    (|d|^2 < 1e6) from every class's rim — a longer direction would send them to the literal loop before any walk."""
    p = scenes._base_params(spp, depth)
    eye = c0 + towards * rho
    vfov = math.degrees(2.0 * math.atan(s0 / rho))
    scenes._look_at(_lib.load(), p, w, h, tuple(float(x) for x in eye), tuple(float(x) for x in c0), vfov, 0.0, 2.0 * s0)
    llc, hor, ver, o = (np.asarray(list(v), np.float64) for v in (p.lower_left_corner, p.horizontal, p.vertical, p.camera_origin))
    for a in (0.0, 1.0):
        for b in (0.0, 1.0):
            dd = llc + a * hor + b * ver - o
            assert 1e-6 < float(dd @ dd) < 1e5, float(dd @ dd)
    return p


# (scene, width, height, the classes it is run at, window checked against the oracle or None = whole frame, build at camera A)
CASES = [
    ("cover", lambda: scenes.config2(96, 54, 1, 1, 8).spheres, 96, 54, CLASSES, None, 1),
    ("field10k", lambda: scenes.config5(128, 72, 1, 1, 8).spheres, 128, 72, CLASSES, (56, 72, 28, 40), 2),
    ("field60k", lambda: scenes.config5(96, 54, 1, 1, 8, n=60000).spheres, 96, 54, (3.0, 16.0), (42, 54, 22, 30), 3),
]
REACHED = set()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_margin_class_at_the_rim_of_its_near_region(ora, case):
    name, make, w, h, classes, window, build_a = case
    sph = make()
    towards = np.array([0.62, 0.45, 0.64])
    towards /= np.linalg.norm(towards)
    t = PathTracer(w, h)
    t.set_geometry_path(abi.PT_GEOM_GRID)
    t.set_grid_fit(True)  # the class the camera needs, unmeasured
    t.set_spheres(sph)
    lst = PathTracer(w, h) if window is not None else None  # the list walk: whole-frame yardstick of the large fields
    if lst is not None:
        lst.set_geometry_path(abi.PT_GEOM_SCALAR)
        lst.set_spheres(sph)
    try:
        for f in classes:
            rc, g = build(sph, near_factor=f)  # the host build of the same grid: its c0, s0 and near region
            assert rc == 0, (name, f, rc)
            c0, s0, rim = g["c0"].astype(np.float64), float(g["s0"]), math.sqrt(float(g["r2_near"]))
            rho = {"A": 0.98 * (f / 1.01 - 1.0) * 0.9999 * s0, "B": rim * (1.0 - 2e-5), "C": rim * (1.0 + 1e-4)}
            assert need_factor(rho["A"], s0) == f
            pa = camera(w, h, 1, 1, c0, s0, rho["A"], towards)
            t.set_params(pa)
            t.reserve_passes(1)
            t.tune(1)
            st = t.stats()
            assert st.grid_near_factor == f and st.grid_need_factor == f and st.grid_fit_stale == 0, (name, f, st.grid_near_factor, st.grid_need_factor)
            assert tuple(st.grid_cells) == tuple(int(x) for x in g["n"]) and st.grid_entries == g["n_entries"], (name, f)
            for cam in ("A", "B", "C"):
                for spp, depth in ((1, 1), (2, 8)):
                    p = camera(w, h, spp, depth, c0, s0, rho[cam], towards)
                    o = np.asarray([list(p.camera_origin)], np.float32)
                    assert bool(near_of(g, o)[0]) == (cam != "C"), (name, f, cam)
                    t.set_params(p)
                    t.reserve_passes(1)
                    t.reset()
                    t.render_passes(1)
                    got = t.accum()
                    st = t.stats()
                    assert st.grid_near_factor == f and st.geometry_path == abi.PT_GEOM_GRID  # no refit
                    stale = 0 if cam == "A" or f == CLASSES[-1] else 1  # the largest class is the most any camera needs
                    assert st.grid_fit_stale == stale, (name, f, cam, st.grid_fit_stale, st.grid_need_factor)
                    want_build = build_a if stale == 0 else max(build_a, 2)
                    assert st.grid_kernel_build == want_build, (name, f, cam, st.grid_kernel_build)
                    if depth == 1:
                        assert (st.far_rays > 0) == (cam == "C"), (name, f, cam, st.far_rays)
                    what = "%s class %g camera %s spp %d depth %d" % (name, f, cam, spp, depth)
                    ref, seg = ora.render(sph, p, 1, window=window, nthreads=ORACLE_THREADS)
                    if window is None:
                        assert_bit_equal(got, ref, what)
                        assert st.segments == seg, (what, st.segments, seg)
                    else:
                        x0, x1, y0, y1 = window
                        assert_bit_equal(got[y0:y1, x0:x1], ref[y0:y1, x0:x1], what + " (oracle window)")
                        lst.set_params(p)
                        lst.reserve_passes(1)
                        lst.reset()
                        lst.render_passes(1)
                        assert_bit_equal(got, lst.accum(), what + " (list walk, whole frame)")
                        assert st.segments == lst.stats().segments, (what, st.segments, lst.stats().segments)
                    REACHED.add((f, int(st.grid_kernel_build), cam))
    finally:
        t.close()
        if lst is not None:
            lst.close()


def test_the_class_by_build_matrix_was_covered():
    """(runs after the cases above) every class on builds 1 and 2, classes 3 and 16 on build 3"""
    rows = []
    for b in (1, 2, 3):
        rows.append("build %d: " % b + "  ".join("%g:%s" % (f, "".join(c for c in "ABC" if (f, b, c) in REACHED) or "-")
                                                  for f in CLASSES))
    print("class x build x camera reached\n" + "\n".join(rows))
    for f in CLASSES:
        assert any((f, 1, c) in REACHED for c in "ABC") and any((f, 2, c) in REACHED for c in "ABC"), f
    for f in (3.0, 16.0):
        assert any((f, 3, c) in REACHED for c in "ABC"), f
