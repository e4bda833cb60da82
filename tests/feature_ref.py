"""The first-hit feature planes of include/ptrace.h (pt_render_features), restated from the oracle's exported pieces only:
ora_v_position (the pixel centre), ora_camera_ray with the lens off and a throw-away seed (the pinhole ray), ora_hit_world
(the hit record) and, for a miss, ora_ray_color (what the path tracer returns for that ray).  TEST INFRASTRUCTURE ONLY.

OraHit.index is the sphere's uuid; the list index is looked up from it, so the scenes given to planes() carry unique uuids
(two identical spheres with different uuids are told apart by exactly that).  ora_camera_ray with the lens off returns
(dd - origin) - (+-0) and origin + (+-0), which differ from the contract's `dd - origin` and `origin` only where a
component is exactly -0 (direction) or -0 (origin): planes() asserts that neither happens for its inputs.
tests/test_feature_ref.py pins the uuid plane to ora_first_hit_map, an independent route through the oracle."""
import ctypes as C

import numpy as np

from oracle import oracle
from ray_tracer_webgl_amd import abi

_FP = C.POINTER(C.c_float)


def owned_rows(p):
    """the image rows of this band's local rows 0, 1, ... (include/ptrace.h pt_band_row)"""
    if p.band_count <= 1 or p.band_rows == 0:
        return [int(y) for y in range(p.height)]
    return [int(y) for y in abi.owned_rows(p.height, p.band_rows, p.band_index, p.band_count)]


def planes(spheres, params):
    """{"albedo", "normal", "point": float32, "ids": int32}, each (local_rows, width, 4), of the band `params` describes"""
    L = oracle.load()
    sph = np.ascontiguousarray(spheres, dtype=abi.SPHERE_DTYPE)
    uuids = [int(u) for u in sph["uuid"]]
    assert len(set(uuids)) == len(uuids), "the restatement finds the list index through the uuid: they must be unique"
    index_of = {u: i for i, u in enumerate(uuids)}
    ptr, n, keep = abi.spheres_as_ctypes(sph)
    p = params.copy()
    p.lens_radius = 0.0  # the contract's ray has no lens; nothing else of the lens enters (u, v only through a product with 0)
    p.max_depth = 1      # (a miss is decided by the first segment; ora_ray_color is only asked about misses)
    w, rows = int(p.width), owned_rows(p)
    alb = np.zeros((len(rows), w, 4), np.float32)
    nrm = np.zeros((len(rows), w, 4), np.float32)
    pnt = np.zeros((len(rows), w, 4), np.float32)
    ids = np.zeros((len(rows), w, 4), np.int32)
    ids[..., :3] = -1
    origin = np.asarray(list(p.camera_origin), np.float32)
    o, d, col = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)()
    hit = oracle.OraHit()
    half, one = np.float32(0.5), np.float32(1.0)
    vxs = [np.float32(L.ora_v_position(x, p.width)) for x in range(w)]
    for ly, y in enumerate(rows):
        vy = np.float32(L.ora_v_position(y, p.height))
        t = np.float32((vy + one) * half)
        for x in range(w):
            s = np.float32((vxs[x] + one) * half)
            seed = C.c_float(0.25)  # thrown away: the lens draws move it, nothing reads it
            L.ora_camera_ray(C.byref(p), float(s), float(t), C.byref(seed), o, d)
            od, dd = np.asarray(o[:], np.float32), np.asarray(d[:], np.float32)
            assert np.array_equal(od.view(np.uint32), origin.view(np.uint32)), "a -0 in the camera origin: outside the restatement"
            assert not (dd == 0).any(), "a zero direction component at (%d, %d): outside the restatement" % (x, y)
            if L.ora_hit_world(ptr, n, o, d, C.byref(hit)):
                i = index_of[int(hit.index)]
                alb[ly, x] = (sph["albedo"][i][0], sph["albedo"][i][1], sph["albedo"][i][2], hit.t)
                nrm[ly, x, :3] = hit.normal[:]
                pnt[ly, x, :3] = hit.point[:]
                ids[ly, x] = (i, int(hit.index), int(sph["type"][i]), int(hit.front_face))
            else:
                seg = C.c_uint64(0)
                L.ora_ray_color(ptr, n, C.byref(p), o, d, C.byref(seed), col, C.byref(seg))
                alb[ly, x, :3] = col[:]
    return {"albedo": alb, "normal": nrm, "point": pnt, "ids": ids}


def first_hit_map(spheres, params):
    """ora_first_hit_map: (height, width) int32, the uuid of the nearest sphere through each pixel centre or -1"""
    L = oracle.load()
    ptr, n, keep = abi.spheres_as_ctypes(spheres)
    p = params.copy()
    out = np.zeros((p.height, p.width), np.int32)
    L.ora_first_hit_map.argtypes = [C.POINTER(abi.PtSphere), C.c_uint32, C.POINTER(abi.PtParams), C.c_void_p]
    L.ora_first_hit_map(ptr, n, C.byref(p), out.ctypes.data_as(C.c_void_p))
    return out
