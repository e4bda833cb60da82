"""The one-layer walk of the grid kernel (csrc/pt_grid_walk.hpp, S::FLAT_Y) against the three-axis walk, on the CPU.

pt_grid.hpp collapses a flat axis to one layer of cells: a field of spheres on a ground (config 2 and 3's cover scene) gets a
grid of nx x 1 x nz cells.  pt_trace_kernel_grid walks such a grid with a two-axis DDA over x and z that ends when the ray's
exit time from the layer is the smallest of the three times; pt_trace_kernel_grid_layers (and the builds that gather) walk
three axes.  `trace` below is tests/test_grid.py's emulation `walk` once more, formula for formula in fp32, with the two
things this file needs: it RECORDS every ray's visited cells and exit times, and it runs either walk.  Checked:

  (a) its three-axis mode IS test_grid.walk (same closest, hit, looked-at count, literal flag, bit for bit);
  (b) with the layer's own planes (lo, lo + h: the three-axis walk's y time at entry) the flat walk visits exactly the cells
      the three-axis walk visits, in the same order, with the same exit times — the step logic is the same walk;
  (c) with the plane the kernel really uses — the box test's far y plane, the slab the host has WIDENED — the three-axis
      visits are a prefix of the flat ones with equal exit times up to the last shared cell, where the flat exit is never
      earlier; whatever it visits in addition lies in the same layer; and the (closest, hit) pair is hit_world's (brute
      force), bit for bit;
  (d) the host-side choice of the walk (pt_geom_plan.hpp grid_walk_flat) through a shim.

Rays: the scenes' own (bounce, camera, far), origins across each class's near region, and hand-made ones: parallel to an
axis (+0 and -0 components), starting outside the box, leaving through y first, origins exactly on cell boundaries.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_bvh import f32, fma, rays_for
from test_grid import GRID_SCENES, MAX_T, PAD, _regular, brute_force, build, exact_root, near_of, rim_rays, walk

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# scenes whose grid has one layer along y (asserted), at these margin classes
FLAT_SCENES = ["config2", "flat", "flat_far", "config2_far"]
FLAT_CLASSES = (2.5, 3.0, 5.5, 16.0)


def trace(g, o, d, flat, y_plane="widened", to_the_end=False):
    """grid_walk's PHASE 1 (pt_grid_walk.hpp) in fp32, as test_grid.walk, recording per ray the list of (cell index, t_exit).
    flat: the one-layer walk; y_plane "widened": its exit time is the box test's max(t1y, t2y) (what the kernel does),
    "layer": the three-axis walk's own y time at entry.  to_the_end: ignore `closest` (pure geometry: every cell up to the
    grid's end).  Returns closest, hit, looked, literal, visits."""
    n = len(o)
    ent, index = g["entries"], g["index"].astype(np.int64)
    closest = np.full(n, MAX_T, np.float32)
    hit = np.full(n, -1, np.int64)
    looked = np.zeros(n, np.int64)
    visits = [[] for _ in range(n)]

    def test_entries(rays, pos):
        v, ok = exact_root(o[rays], d[rays], ent[pos, :3], ent[pos, 3])
        idx = index[pos]
        ok &= idx != PAD
        cur, cur_hit = closest[rays], hit[rays]
        wins = ok & ((v < cur) | ((v == cur) & ((cur_hit < 0) | (idx > cur_hit))))
        closest[rays] = np.where(wins, v, cur)
        hit[rays] = np.where(wins, idx, cur_hit)

    allr = np.arange(n)
    for k in range(g["n_cell_entries"], g["n_entries"]):
        test_entries(allr, np.full(n, k))
    with np.errstate(divide="ignore"):
        inv = np.clip(f32(1.0) / d, f32(-1e18), f32(1e18)).astype(np.float32)
    pos_dir = inv > 0
    H = np.broadcast_to(g["h"][None, :], d.shape)
    td = f32(H * np.abs(inv))
    p = f32(o - g["c0"][None, :])
    r2 = fma(p[:, 2], p[:, 2], fma(p[:, 1], p[:, 1], f32(p[:, 0] * p[:, 0])))
    near = r2 <= g["r2_near"]
    mm = np.where(near, np.float32(0), f32(np.float32(1.7e-3) * f32(np.sqrt(r2) + g["s0"]))).astype(np.float32)
    oi = f32(o * inv)
    lo_m = f32(g["lo_n"][None, :] - mm[:, None])
    hi_m = f32(g["hi_n"][None, :] + mm[:, None])
    t1 = fma(lo_m, inv, -oi)
    t2 = fma(hi_m, inv, -oi)
    tn = np.maximum(np.maximum(np.minimum(t1[:, 0], t2[:, 0]), np.minimum(t1[:, 1], t2[:, 1])),
                    np.maximum(np.minimum(t1[:, 2], t2[:, 2]), np.float32(0)))
    tf = np.minimum(np.minimum(np.maximum(t1[:, 0], t2[:, 0]), np.maximum(t1[:, 1], t2[:, 1])), np.maximum(t1[:, 2], t2[:, 2]))
    enter = tn <= np.minimum(tf, closest)
    literal = enter & ~near
    active = enter & near
    nn = g["n"]
    LO = np.broadcast_to(g["lo"][None, :], d.shape)
    fcell = f32(f32(fma(d, np.broadcast_to(tn[:, None], d.shape), o) - LO) * g["inv_h"][None, :])
    fcell = np.where(active[:, None], fcell, np.float32(0))
    cell3 = np.clip(np.floor(fcell).astype(np.int64), 0, nn[None, :] - 1)
    bnd = fma(f32(cell3 + pos_dir), H, LO)
    tm = np.maximum(fma(bnd, inv, -oi), tn[:, None])
    rem = np.where(pos_dir, nn[None, :] - 1 - cell3, cell3) + 1
    if flat:
        assert nn[1] == 1
        # the flat entry computes no cy (it is 0) and takes the layer's exit time once: it never changes
        if y_plane == "widened":
            tm[:, 1] = np.maximum(t1[:, 1], t2[:, 1])
            assert np.all(tm[active, 1] >= tn[active])  # (tn <= tf <= max(t1y, t2y): no clamp needed)
        cell3[:, 1] = 0
    first, count = (g["cells"] & 0xFFFFFF).astype(np.int64), (g["cells"] >> 24).astype(np.int64)
    for _ in range(int(nn.sum()) + 4):
        rays = np.nonzero(active)[0]
        if not len(rays):
            break
        tmin = tm[rays].min(1)
        isx = tm[rays, 0] == tmin
        if flat:
            cidx = cell3[rays, 2] * nn[0] + cell3[rays, 0]  # cell = cz * gnx + cx
            endy = ~isx & (tm[rays, 1] == tmin)             # x before y before z; y ends the walk
            ax = np.where(isx, 0, 2)
        else:
            cidx = (cell3[rays, 2] * nn[1] + cell3[rays, 1]) * nn[0] + cell3[rays, 0]
            isy = ~isx & (tm[rays, 1] == tmin)
            endy = np.zeros(len(rays), bool)
            ax = np.where(isx, 0, np.where(isy, 1, 2))
        t_exit = tmin
        for r, c, t in zip(rays.tolist(), cidx.tolist(), t_exit.tolist()):
            visits[r].append((c, np.float32(t)))
        tm[rays, ax] = f32(tm[rays, ax] + td[rays, ax])
        rem[rays, ax] -= 1
        out = (rem[rays, ax] == 0) | endy
        cell3[rays, ax] += np.where(pos_dir[rays, ax], 1, -1)
        cmax = int(count[cidx].max()) if len(cidx) else 0
        for k in range(cmax):
            sel = count[cidx] > k
            test_entries(rays[sel], first[cidx[sel]] + k)
            looked[rays[sel]] += 1
        done = out if to_the_end else out | (closest[rays] < t_exit)
        active[rays[done]] = False
    assert not active.any()
    return closest, hit, looked, literal, visits


def handmade_rays(g, seed):
    """axis-parallel rays (+0 and -0 components), origins outside the box, rays that leave through y first, origins
    exactly on cell boundaries (x, z and the layer's own y planes); all inside the near region"""
    rng = np.random.default_rng(seed)
    lo, h, nn = g["lo"].astype(np.float64), g["h"].astype(np.float64), g["n"]
    hi = lo + h * nn
    mid, ext = 0.5 * (lo + hi), hi - lo
    o, d = [], []
    inside = lambda k: lo + ext * rng.uniform(0.02, 0.98, (k, 3))
    # parallel to an axis, from inside and from beside the box
    for axis in range(3):
        for sgn in (1.0, -1.0):
            for zero in (0.0, -0.0):
                k = 12
                oo = inside(k)
                oo[k // 2:, axis] = (lo - 0.2 * ext)[axis] if sgn > 0 else (hi + 0.2 * ext)[axis]  # half start outside
                dd = np.full((k, 3), zero)
                dd[:, axis] = sgn * rng.choice([1e-2, 1.0, 25.0], k)
                o.append(oo); d.append(dd)
    # in a plane: one component zero
    for axis in range(3):
        k = 30
        dd = rng.normal(size=(k, 3))
        dd[:, axis] = rng.choice([0.0, -0.0], k)
        o.append(inside(k)); d.append(dd)
    # outside the box, aimed at it
    k = 150
    u = rng.normal(size=(k, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    oo = mid + u * 0.9 * np.sqrt(float(g["r2_near"]))
    o.append(oo); d.append((inside(k) - oo) * rng.choice([0.05, 1.0, 4.0], (k, 1)))
    # steep: leave through y before any x or z boundary; and shallow: y last
    k = 80
    dd = rng.normal(size=(k, 3)) * 0.05
    dd[:, 1] = rng.choice([-1.0, 1.0], k) * rng.uniform(0.5, 3.0, k)
    o.append(inside(k)); d.append(dd)
    dd = rng.normal(size=(k, 3))
    dd[:, 1] = rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(-9, -3, k)
    o.append(inside(k)); d.append(dd)
    # origins exactly on cell boundaries (the fp32 planes the walk itself computes: fma(k, h, lo))
    k = 120
    oo = inside(k)
    for axis in (0, 2):
        sel = rng.random(k) < 0.7
        kk = rng.integers(0, nn[axis] + 1, k).astype(np.float32)
        plane = fma(kk, np.full(k, g["h"][axis], np.float32), np.full(k, g["lo"][axis], np.float32))
        oo[sel, axis] = plane[sel]
    sel = rng.random(k) < 0.3
    oo[sel, 1] = np.where(rng.random(k) < 0.5, g["lo"][1], fma(f32(np.ones(k)), np.full(k, g["h"][1], np.float32), np.full(k, g["lo"][1], np.float32)))[sel]
    o.append(oo); d.append(rng.normal(size=(k, 3)) * rng.choice([0.01, 1.0, 30.0], (k, 1)))
    o, d = f32(np.concatenate(o)), f32(np.concatenate(d))
    ok = _regular(o, d) & near_of(g, o)
    assert ok.sum() > 0.8 * len(o), (int(ok.sum()), len(o))
    return o[ok], d[ok]


def ray_sets(g, sph, n_rays):
    for seed in range(2):
        o, d = rays_for(sph, n_rays, seed)
        ok = _regular(o, d)
        yield "scene %d" % seed, o[ok], d[ok]
        o, d, _ = rim_rays(g, sph, n_rays // 2, 90 + seed)
        ok = _regular(o, d)
        yield "rim %d" % seed, o[ok], d[ok]
    o, d = handmade_rays(g, 7)
    yield "handmade", o, d


@pytest.mark.parametrize("name", ["config2", "flat", "field300", "mixed_radii"])
def test_the_recording_emulation_in_three_axis_mode_is_test_grids_walk(name):
    sph = GRID_SCENES[name]()
    rc, g = build(sph)
    assert rc == 0
    for what, o, d in ray_sets(g, sph, 1200):
        ref = walk(g, o, d, sph)
        got = trace(g, o, d, flat=False)
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), (name, what)
        for k in (1, 2, 3):
            assert np.array_equal(got[k], ref[k]), (name, what, k)
        # one visit per cell looked at ... at least (empty cells are visited too)
        assert all(len(v) > 0 for v, l in zip(got[4], got[2]) if l > 0)


@pytest.mark.parametrize("f", FLAT_CLASSES)
@pytest.mark.parametrize("name", FLAT_SCENES)
def test_with_the_layers_own_planes_the_flat_walk_is_the_three_axis_walk(name, f):
    """same cells, same order, same exit times (bitwise), with and without early termination; same pair, same entries looked at"""
    sph = GRID_SCENES[name]()
    rc, g = build(sph, near_factor=f)
    assert rc == 0 and g["n"][1] == 1, (name, f, g["n"])
    n_walked = n_y_exit = 0
    for what, o, d in ray_sets(g, sph, 1500):
        for to_the_end in (False, True):
            a = trace(g, o, d, flat=False, to_the_end=to_the_end)
            b = trace(g, o, d, flat=True, y_plane="layer", to_the_end=to_the_end)
            assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]), (name, f, what)
            assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), (name, f, what)
            for r, (va, vb) in enumerate(zip(a[4], b[4])):
                assert [c for c, _ in va] == [c for c, _ in vb], (name, f, what, r, va, vb)
                assert [t.view(np.uint32) for _, t in va] == [t.view(np.uint32) for _, t in vb], (name, f, what, r, va, vb)
        n_walked += sum(1 for v in a[4] if v)
        nx, nz = int(g["n"][0]), int(g["n"][2])
        n_y_exit += sum(1 for v in a[4] if v and len(v) < max(nx, nz) // 2)
    assert n_walked > 1500 and n_y_exit > 200, (n_walked, n_y_exit)


@pytest.mark.parametrize("f", FLAT_CLASSES)
@pytest.mark.parametrize("name", FLAT_SCENES)
def test_with_the_widened_plane_the_flat_walk_ends_later_never_earlier_and_finds_hit_worlds_pair(name, f):
    """What the kernel runs.  Geometry (walks run to the grid's end): the three-axis visits are a prefix of the flat ones; exit
    times equal bitwise before the last shared cell, not earlier at it.  With early termination: the same, and (closest, hit)
    is brute force's pair, bit for bit."""
    sph = GRID_SCENES[name]()
    rc, g = build(sph, near_factor=f)
    assert rc == 0 and g["n"][1] == 1, (name, f, g["n"])
    # the widened slab contains the layer: what the argument in pt_grid_walk.hpp's header rests on
    top = fma(f32(np.ones(1)), f32(g["h"][1:2]), f32(g["lo"][1:2]))[0]
    assert g["lo_n"][1] <= g["lo"][1] and g["hi_n"][1] >= top, (g["lo_n"][1], g["lo"][1], g["hi_n"][1], top)
    n_cells = int(g["n"][0] * g["n"][2])
    n_same = n_longer = n_hits = 0
    for what, o, d in ray_sets(g, sph, 1500):
        for to_the_end in (True, False):
            a = trace(g, o, d, flat=False, to_the_end=to_the_end)
            b = trace(g, o, d, flat=True, to_the_end=to_the_end)
            assert np.array_equal(a[3], b[3]), (name, f, what)
            for r, (va, vb) in enumerate(zip(a[4], b[4])):
                where = (name, f, what, to_the_end, r, va, vb)
                assert len(vb) >= len(va), where
                assert [c for c, _ in vb[:len(va)]] == [c for c, _ in va], where
                assert all(0 <= c < n_cells for c, _ in vb), where
                if va:
                    k = len(va) - 1
                    assert [t.view(np.uint32) for _, t in vb[:k]] == [t.view(np.uint32) for _, t in va[:k]], where
                    assert vb[k][1] >= va[k][1], where
                    # exit times never decrease along a walk
                    assert all(vb[i][1] <= vb[i + 1][1] for i in range(len(vb) - 1)), where
                    n_same += len(vb) == len(va)
                    n_longer += len(vb) > len(va)
            if not to_the_end:
                ref_t, ref_i = brute_force(o, d, sph)
                chk = ~b[3]
                bad = chk & ((b[1] != ref_i) | (b[0].view(np.uint32) != ref_t.view(np.uint32)))
                assert not bad.any(), (name, f, what, np.nonzero(bad)[0][:5], b[1][bad][:5], ref_i[bad][:5])
                assert np.array_equal(a[0].view(np.uint32)[chk], b[0].view(np.uint32)[chk]) and np.array_equal(a[1][chk], b[1][chk])
                n_hits += int((ref_i[chk] >= 0).sum())
    print("%s class %g: walks with the same visits %d, with more %d, hits %d" % (name, f, n_same, n_longer, n_hits))
    assert n_same > 2000 and n_hits > 500, (n_same, n_longer, n_hits)
    assert n_longer < 0.05 * (n_same + n_longer), (n_same, n_longer)  # a hair later: rarely another cell


# ---- (d) the host's choice of the walk ---------------------------------------------------------------

SHIM_SRC = os.path.join(HERE, "grid_flat_shim.cpp")


def test_the_host_gives_the_flat_walk_to_the_lds_staged_build_of_a_one_layer_grid_only():
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "grid_flat_shim.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), SHIM_SRC, "-o", so])
        lib = C.CDLL(so)
        lib.shim_grid_walk_flat.restype = C.c_int
        lib.shim_grid_walk_flat.argtypes = [C.c_int, C.c_uint32]
        lib.shim_flat_after_staging.restype = C.c_int
        lib.shim_flat_after_staging.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_int]
        for kind in (0, 1, 2, 3):
            for ny in (1, 2, 6, 1000):
                assert lib.shim_grid_walk_flat(kind, ny) == int(kind == 1 and ny == 1), (kind, ny)
        # through grid_staging: config 2's grid (16 x 1 x 16, ~900 entries) is staged whole and walks flat; a stale view or
        # pt_tune's cells build, or entries beyond the LDS, get a gathering build and three axes; several layers never walk flat
        assert lib.shim_flat_after_staging(256, 900, 1, 0, 0) == 1 * 16 + 1
        assert lib.shim_flat_after_staging(256, 900, 1, 0, 1) == 2 * 16 + 0
        assert lib.shim_flat_after_staging(256, 900, 1, 1, 0) == 2 * 16 + 0
        assert lib.shim_flat_after_staging(256, 900, 1, 0, 2) == 1 * 16 + 1
        assert lib.shim_flat_after_staging(5400, 40000, 1, 0, 0) == 2 * 16 + 0
        assert lib.shim_flat_after_staging(512, 900, 2, 0, 0) == 1 * 16 + 0
        assert lib.shim_flat_after_staging(5400, 3000, 6, 0, 0) == 1 * 16 + 0
