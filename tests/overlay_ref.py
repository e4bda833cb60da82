"""The debug overlay's expected values: tests/overlay_ref.c (a restatement of one pass with static/shader.frag:307-318 alive,
built on the CPU oracle's exported pieces) compiled and bound here, and the cases the CPU coverage test and the GPU tests
share.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import oracle
from ray_tracer_webgl_amd import _lib, abi, scenes

HERE = os.path.dirname(os.path.abspath(__file__))
THREADS = min(16, os.cpu_count() or 1)
_ref = None


class OvlTally(C.Structure):
    _fields_ = [("segments", C.c_uint64), ("blue_paths", C.c_uint64), ("red_paths", C.c_uint64),
                ("deep_overlay_paths", C.c_uint64), ("selected_plain_hits", C.c_uint64)]


def load():
    """tests/overlay_ref.c, compiled like the oracle (-ffp-contract=off, fmaf for the dot product) and linked against it"""
    global _ref
    if _ref is None:
        oracle.load()
        so = os.path.join(tempfile.mkdtemp(prefix="overlay_ref_"), "liboverlay_ref.so")
        ora_dir = os.path.dirname(oracle.LIB_PATH)
        subprocess.check_call(["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math",
                               "-fno-math-errno", "-Wall", "-Wextra", "-Werror", os.path.join(HERE, "overlay_ref.c"), "-o", so,
                               "-L" + ora_dir, "-l:libpt_oracle.so", "-Wl,-rpath," + ora_dir, "-lm"])
        L = C.CDLL(so)
        fp = C.POINTER(C.c_float)
        L.ovl_render_pass.restype = None
        L.ovl_render_pass.argtypes = [C.POINTER(abi.PtSphere), C.c_uint32, C.POINTER(abi.PtParams), C.c_float, C.c_int, C.c_int32, fp, fp,
                                      C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(OvlTally)]
        _ref = L
    return _ref


def pass_time(p, k):
    """u_time of pass k: time + float(first_pass + k) * time_step in fp32 (a step of 0 means 1), as oracle/pt_oracle.c forms it"""
    step = np.float32(p.time_step if p.time_step != 0.0 else 1.0)
    return float(np.float32(p.time) + np.float32(p.first_pass + k) * step)


def render(spheres, params, n_passes=1, overlay=None, window=None, accum=None):
    """n_passes passes of the owned rows, pass k at pass_time(k), added in pass order like oracle.render.
    overlay = (selected_object, cursor_point) or None (disabled).  Returns (accum (local_rows, width, 4) float32,
    tally dict, flags (local_rows, width) uint8: bit 0 the pixel got a blue contribution, bit 1 a red one)."""
    L = load()
    ptr, n, keep = abi.spheres_as_ctypes(spheres)
    p = params.copy()
    rows = abi.local_rows(p.height, p.band_rows, p.band_index, p.band_count)
    if accum is None:
        accum = np.zeros((rows, p.width, 4), dtype=np.float32)
    flags = np.zeros((rows, p.width), dtype=np.uint8)
    x0, x1, y0, y1 = window if window is not None else (0, p.width, 0, p.height)
    enable = 0 if overlay is None else 1
    selected = 0 if overlay is None else int(overlay[0])
    cursor = (C.c_float * 3)(*([0.0] * 3 if overlay is None else [float(x) for x in overlay[1]]))
    total = dict.fromkeys([f[0] for f in OvlTally._fields_], 0)
    step = max(1, (y1 - y0 + 4 * THREADS - 1) // (4 * THREADS))
    blocks = [(y, min(y + step, y1)) for y in range(y0, y1, step)]
    for k in range(n_passes):
        t = pass_time(p, k)

        def job(b):
            tally = OvlTally()
            L.ovl_render_pass(ptr, n, C.byref(p), t, enable, selected, cursor, accum.ctypes.data_as(C.POINTER(C.c_float)),
                              flags.ctypes.data_as(C.c_void_p), x0, x1, b[0], b[1], C.byref(tally))
            return tally

        with ThreadPoolExecutor(THREADS) as pool:  # (disjoint rows: the threads share nothing they write)
            for tally in pool.map(job, blocks):
                for f in total:
                    total[f] += getattr(tally, f)
    return accum, total, flags


def center_pick(spheres, p):
    """(uuid, hit point) of the ray through the image's middle — the fp32 counterpart of the State's pick ray — or None"""
    L = oracle.load()
    ptr, n, keep = abi.spheres_as_ctypes(spheres)
    o = np.asarray(list(p.camera_origin), np.float32)
    d = (np.asarray(list(p.lower_left_corner), np.float32) + np.float32(0.5) * np.asarray(list(p.horizontal), np.float32)
         + np.float32(0.5) * np.asarray(list(p.vertical), np.float32) - o).astype(np.float32)
    h = oracle.OraHit()
    fp = C.POINTER(C.c_float)
    if not L.ora_hit_world(ptr, n, o.ctypes.data_as(fp), d.ctypes.data_as(fp), C.byref(h)):
        return None
    return int(h.index), tuple(float(x) for x in h.point)


# ---------------------------------------------------------------------------------------------------------- the cases
class Case:
    def __init__(self, name, spheres, params, n_passes, overlay, paths):
        self.name, self.spheres, self.params, self.n_passes, self.overlay, self.paths = name, spheres, params, n_passes, overlay, paths


def state_overlay(w, h):
    """the State's own cursor and selection for State::default's camera: (selected_object, cursor_point)"""
    from ray_tracer_webgl_amd.state import State

    st = State(w, h)
    st.set_debugging(True)
    st.pick()
    en, sel, cur = st.debug_overlay()
    st.close()
    assert en
    return sel, cur


def default_case():
    """The reference's scene with the State's own cursor and selection: the crosshair is on the centre sphere (uuid 1), the
    cursor its nearest point (0, 0, -0.5).  The outline band of that sphere is a fraction of a pixel wide at this size for
    the camera's own rays (|d| ~ 0.75): four samples per pixel and two passes, and the short bounce rays, fill it."""
    sc = scenes.default_scene(320, 176, spp=4, max_depth=8, n_passes=2)
    p = sc.params.copy()
    p.time_step = abi.PT_TIME_STEP_DECORRELATED
    return Case("default", sc.spheres, p, 2, state_overlay(320, 176), [abi.PT_GEOM_SMALL])


def look_at(w, h, spp, depth, frm, at, vfov, focus, background=abi.PT_BG_SKY):
    p = scenes._base_params(spp, depth, background)
    scenes._look_at(_lib.load(), p, w, h, tuple(float(x) for x in frm), tuple(float(x) for x in at), vfov, 0.0, focus)
    p.time_step = abi.PT_TIME_STEP_DECORRELATED
    return p


def cover_case():
    """The cover scene (484 spheres; its grid has one layer of cells) with whatever its camera's middle ray hits selected."""
    sc = scenes.config2(192, 108, 4, 2, 8)
    p = sc.params.copy()
    p.time_step = abi.PT_TIME_STEP_DECORRELATED
    return Case("cover", sc.spheres, p, 2, center_pick(sc.spheres, p), [abi.PT_GEOM_SCALAR, abi.PT_GEOM_BVH, abi.PT_GEOM_GRID])


def field_spheres(n, remap_uuids):
    sph = scenes.field_spheres(n)
    if remap_uuids:  # the caller's values, not list indices: a permutation, shifted away from 0 .. n
        perm = np.random.default_rng(81000 + n).permutation(len(sph))
        sph["uuid"] = (7000 + 3 * perm).astype(np.int32)
    return sph


def field_case(n=1500, w=96, h=54, remap_uuids=True, paths=(abi.PT_GEOM_SCALAR, abi.PT_GEOM_BVH, abi.PT_GEOM_GRID)):
    """A random field on a ground (several layers of cells), seen from 1.6 units off one of its larger spheres near the
    ground (rays that bounce off the ground come back to it), which is selected; the cursor is that sphere's point nearest the camera.  Focus distance 0.25 (no lens: it only scales the
    camera rays' directions, and the outline test compares against the UNNORMALISED direction)."""
    sph = field_spheres(n, remap_uuids)
    c, r = sph["center"].astype(np.float64), np.abs(sph["radius"].astype(np.float64))
    cand = np.where((r > 0.4) & (r < 1.0) & (c[:, 1] > 0.6) & (c[:, 1] < 1.5))[0]
    k = int(cand[np.argmin(np.linalg.norm(c[cand] - np.array([0.0, 1.0, 0.0]), axis=1))])
    towards = np.array([0.48, 0.12, 0.8])
    towards /= np.linalg.norm(towards)
    p = look_at(w, h, 4, 8, c[k] + towards * (r[k] + 1.6), c[k], 60.0, 0.25)
    cursor = (c[k] + towards * r[k]).astype(np.float32)
    return Case("field%d" % n, sph, p, 2, (int(sph["uuid"][k]), tuple(float(x) for x in cursor)), list(paths))


def room_case():
    """The closed room with its EMISSIVE sphere selected and the cursor on it: the overlay comes before emission."""
    sc = scenes.config4(96, 96, 8, 2, 8)
    p = sc.params.copy()
    p.time_step = abi.PT_TIME_STEP_DECORRELATED
    k = int(np.where(sc.spheres["type"] == abi.PT_EMISSIVE)[0][0])
    c, r = sc.spheres["center"][k].astype(np.float64), float(sc.spheres["radius"][k])
    towards = np.asarray(list(p.camera_origin), np.float64) - c
    towards /= np.linalg.norm(towards)
    cursor = (c + towards * r).astype(np.float32)
    return Case("room", sc.spheres, p, 2, (int(sc.spheres["uuid"][k]), tuple(float(x) for x in cursor)), [abi.PT_GEOM_SMALL, abi.PT_GEOM_SCALAR])


CASES = {"default": default_case, "cover": cover_case, "field": field_case, "room": room_case}
