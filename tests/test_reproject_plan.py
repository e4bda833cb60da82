"""The host constants of temporal reprojection (csrc/pt_reproject_plan.hpp, what pt_reproject_constants computes) on the CPU,
through tests/reproject_plan_shim.cpp, against the float64 restatement tests/reproject_ref.py bit for bit, degenerate cameras
refused; then the stand-alone program tests/reproject_main.cpp under the address and undefined-behaviour sanitizers: the
per-pixel header the kernel runs (csrc/pt_reproject.hpp) over whole hand-made frames with every hostile operand class, every
buffer bounds-checked, compared with the restatement's output.  The gather's index guard is thus proven on the CPU before any
GPU sees those operands.  CPU only; nothing sanitized is loaded into this process."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import error_ref as ER
import reproject_ref as RR
from ray_tracer_webgl_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def shim():
    return RR.build_shim(tempfile.mkdtemp(prefix="reproject_plan_"))


def shim_constants(shim, p, tol):
    cam, out = RR.camera12(p), np.full(16, 123.0, np.float32)
    ok = shim.reproject_plan_constants(cam.ctypes.data_as(FP), int(p.width), float(tol), out.ctypes.data_as(FP))
    if not ok:
        assert np.all(out == 123.0)   # a refused camera writes nothing
        return None
    return out


def random_camera(rng, lib):
    cam = abi.PtCameraIn()
    cam.width, cam.height = int(rng.integers(1, 4000)), int(rng.integers(1, 2200))
    cam.camera_origin = abi.d3(*rng.normal(0, 5, 3))
    cam.yaw_degrees, cam.pitch_degrees = float(rng.uniform(-180, 180)), float(rng.uniform(-89, 89))
    cam.vup = abi.d3(0, 1, 0)
    cam.fov_radians, cam.focus_distance, cam.aperture = float(rng.uniform(0.05, 2.3)), float(rng.uniform(0.1, 20)), float(rng.uniform(0, 0.5))
    p = abi.PtParams()
    assert lib.pt_camera_from_state(C.byref(cam), C.byref(p)) == 0
    return p


def test_constants_against_the_float64_restatement(shim, lib):
    rng = np.random.default_rng(5)
    for _ in range(300):
        p = random_camera(rng, lib)
        tol = float(rng.choice([0.0, 0.5, 1.0, 2.0, 4.0, 8.0, 1000.0]))
        ref, got = RR.constants(p, tol), shim_constants(shim, p, tol)
        assert ref is not None and got is not None
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (list(got), list(ref))
        # ... and the library's entry point is the same header (no device needed)
        out = np.zeros(16, np.float32)
        assert lib.pt_reproject_constants(C.byref(p), tol, out.ctypes.data_as(FP)) == abi.PT_OK
        assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))


def test_constants_project_a_pixel_centre_back_onto_itself(shim):
    sph, p = ER.estimate_scene(160, 88)
    K = shim_constants(shim, p, 2.0).astype(np.float64)
    O, Hh, V = (np.array(list(v), np.float64) for v in (p.camera_origin, p.horizontal, p.vertical))
    e = np.array(list(p.lower_left_corner), np.float64) - O
    for s, t, lam in ((0.25, 0.75, 3.0), (0.9, 0.1, 0.2)):
        w = lam * (e + s * Hh + t * V)
        assert abs(w @ K[3:6] - lam) < 1e-6 * lam
        assert abs(w @ K[6:9] / lam - K[12] - s) < 1e-6 and abs(w @ K[9:12] / lam - K[13] - t) < 1e-6
    assert abs(K[14] - 4.0 * (Hh @ Hh) / 160.0 ** 2) < 1e-9


def degenerate_cameras():
    sph, p = ER.estimate_scene(96, 54)
    out = []
    for field in ("horizontal", "vertical"):
        q = p.copy()
        setattr(q, field, abi.f3(0.0, 0.0, 0.0))
        out.append(q)
    q = p.copy()
    q.vertical = q.horizontal               # n = 0
    out.append(q)
    q = p.copy()
    q.lower_left_corner = q.camera_origin   # e = 0
    out.append(q)
    for bad in (float("nan"), float("inf"), 1e30):
        q = p.copy()
        q.horizontal = abi.f3(bad, 0.0, 0.0)
        out.append(q)
    return p, out


def test_degenerate_cameras_are_refused(shim, lib):
    p, bad = degenerate_cameras()
    out = np.zeros(16, np.float32)
    for q in bad:
        assert RR.constants(q, 2.0) is None and shim_constants(shim, q, 2.0) is None
        assert lib.pt_reproject_constants(C.byref(q), 2.0, out.ctypes.data_as(FP)) == abi.PT_ERR_INVALID
    for tol in (-1.0, float("nan"), float("inf")):
        assert lib.pt_reproject_constants(C.byref(p), tol, out.ctypes.data_as(FP)) == abi.PT_ERR_INVALID
    assert lib.pt_reproject_constants(None, 2.0, out.ctypes.data_as(FP)) == abi.PT_ERR_INVALID
    assert lib.pt_reproject_constants(C.byref(p), 2.0, None) == abi.PT_ERR_INVALID
    assert not out.any()


def test_per_pixel_header_under_address_and_undefined_behaviour_sanitizers():
    """tests/reproject_main.cpp: a stand-alone program (its own main), built with -fsanitize=address,undefined and run as a
    child over the files written here: the 131x13 hand-made frame with every operand class at four settings, the same frame
    as three bands of four rows, one-texel and one-column frames, and a refused camera"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "reproject_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", os.path.join(HERE, "reproject_main.cpp"), "-o", exe])
        files = []

        def add(f, prev, params, caps, tol):
            files.append(os.path.join(tmp, "frame%d.bin" % len(files)))
            RR.write_main_file(files[-1], f["cur_ids"], f["cur_pnt"], f["hist_ids"], f["hist_pnt"], f["acc"], prev, params, caps[0], caps[1], tol)

        sph, p = ER.estimate_scene(131, 13)
        f = RR.hand_frame(p)
        for caps, tol in (((32.0, 8.0), 2.0), ((16777215.0, 0.0), 1000.0), ((0.0, 3.0), 0.0), ((1.0, 1.0), 0.5)):
            add(f, p, p, caps, tol)
        for r in range(3):
            q = p.copy()
            q.band_rows, q.band_index, q.band_count = 4, r, 3
            ys = abi.owned_rows(13, 4, r, 3)
            add({k: v[ys] for k, v in f.items()}, p, q, (32.0, 8.0), 2.0)
        for w, h in ((1, 1), (1, 9), (3, 2)):
            sph, q = ER.estimate_scene(w, h)
            add(RR.hand_frame(q, seed=w + h), q, q, (32.0, 8.0), 4.0)
        add(f, degenerate_cameras()[1][0], p, (32.0, 8.0), 2.0)
        out = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and "reproject: ok (%d files)" % len(files) in out.stdout, out.stdout[-2000:]
