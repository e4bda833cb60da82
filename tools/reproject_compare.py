"""Dev tool: what temporal reprojection costs and what it is worth, on an MI355X (profiles/r19_reproject.txt).

    python tools/reproject_compare.py cost [config2 config4 config5 default]
    python tools/reproject_compare.py quality [WIDTHxHEIGHT ...]        (default: 160x88 1280x702)

cost: per config at the bench size one context (tuned, on a stream of its own), samples_per_pixel = 1, and a camera that
steps sideways and back between two views.  Per run, in the order of a host's tick: pt_keep_history, (pt_set_params of the
other view, untimed host work), pt_render_features, pt_reproject, then the parent's only alternative for a moving camera, ONE
pt_render_passes(1) at 1 spp (trace + fold).  Four runs after a warm-up of all of them, HIP events on the context's stream
around each call; printed: the four times of each, median and spread (max - min), and steps 1 + 3 + 4 against the pass.

quality: the eight-frame flight of tests/test_reproject_ref.py (default scene, depth 6, 4 spp per frame; frame k: origin offset
(0.02 k, 0, -0.01 k), yaw + 0.5 degrees x k) on the device.  One context flies it with the tick above, a second one renders
each frame's fresh pass alone and a third the frame's truth, 16 x 64 spp at a clock of its own.  Printed per setting (tolerance,
caps) and frame 1 / 4 / 8: the squared error of history + fresh over the squared error of the fresh pass alone, and the kept
share of the frame."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ray_tracer_webgl_amd import abi, scenes  # noqa: E402
from ray_tracer_webgl_amd._lib import load  # noqa: E402
from ray_tracer_webgl_amd.tracer import PathTracer  # noqa: E402

CONFIGS = {
    "config2": lambda: scenes.config2(1920, 1080, 1, 1, 50),
    "config4": lambda: scenes.config4(1024, 1024, 1, 1, 50),
    "config5": lambda: scenes.config5(1920, 1080, 1, 1, 50),
    "default": lambda: scenes.default_scene(1280, 702, spp=1, max_depth=8),
}
RUNS = 4
SETTINGS = ((2.0, 32.0, 8.0), (4.0, 32.0, 8.0), (1.0, 32.0, 8.0), (2.0, 32.0, 0.0))   # (tolerance_px, cap_diffuse, cap_other)


def cost(names):
    import torch

    def timed(stream, call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    side = torch.cuda.Stream()
    opt = abi.PtReprojectOptions()
    for name in names:
        sc = CONFIGS[name]()
        views = [sc.params.copy(), sc.params.copy()]
        for k in range(3):   # a hundredth of the view's width sideways: the camera and its image plane move together
            views[1].camera_origin[k] += 0.01 * sc.params.horizontal[k]
            views[1].lower_left_corner[k] += 0.01 * sc.params.horizontal[k]
        with torch.cuda.stream(side):
            pt = PathTracer(sc.params.width, sc.params.height, use_torch=True)
            pt.set_spheres(sc.spheres)
            pt.set_params(views[0])
            pt.tune(1)
            pt.feature_planes(True)
            pt.reproject_option(True)
            pt.set_params(views[0])
            pt.render_features()
            pt.render_passes(1)
            times = {"keep_history": [], "render_features": [], "reproject": [], "pass (trace + fold)": []}
            for run in range(2 + RUNS):   # two warm-up ticks: every code object loaded, every launch planned once
                t = [timed(side, pt.keep_history)]
                views[(run + 1) % 2].time = sc.params.time + 10.0 * (run + 1)
                pt.set_params(views[(run + 1) % 2])
                t.append(timed(side, pt.render_features))
                t.append(timed(side, lambda: pt.reproject(opt)))
                t.append(timed(side, lambda: pt.render_passes(1)))
                if run >= 2:
                    for key, v in zip(times, t):
                        times[key].append(v)
            rs, st = pt.reproject_stats(), pt.stats()
            pt.close()
        med = lambda v: float(np.median(v))
        print("%s: %dx%d, %d spheres, geometry path %d, kept %.3f of the frame" % (
            name, sc.params.width, sc.params.height, len(sc.spheres), st.geometry_path, rs.pixels_kept / max(rs.pixels, 1)))
        for key, v in times.items():
            print("  %-20s ms: %s   median %.4f spread %.4f" % (key, " ".join("%.4f" % x for x in v), med(v), max(v) - min(v)))
        tick = med(times["keep_history"]) + med(times["render_features"]) + med(times["reproject"])
        print("  steps 1 + 3 + 4: %.4f ms = %.3f of the pass" % (tick, tick / med(times["pass (trace + fold)"])), flush=True)


def flight_params(p0, k):
    lib = load()
    cam = abi.PtCameraIn()
    assert lib.pt_default_camera(p0.width, p0.height, C.byref(cam)) == 0
    cam.camera_origin = abi.d3(cam.camera_origin[0] + 0.02 * k, cam.camera_origin[1], cam.camera_origin[2] - 0.01 * k)
    cam.yaw_degrees = cam.yaw_degrees + 0.5 * k
    p = p0.copy()
    assert lib.pt_camera_from_state(C.byref(cam), C.byref(p)) == 0
    p.time = p0.time + 1000.0 * k
    return p


def quality(sizes):
    for w, h in sizes:
        sc = scenes.default_scene(w, h, spp=4, max_depth=6)
        p0 = sc.params.copy()
        p0.time, p0.time_step, p0.first_pass = 200.0, abi.PT_TIME_STEP_DECORRELATED, 0
        frames = [flight_params(p0, k) for k in range(9)]
        fresh, truth = {}, {}
        pt = PathTracer(w, h)
        pt.set_spheres(sc.spheres)
        pt.reserve_passes(16)
        for k in (1, 4, 8):
            pt.reset()
            pt.set_params(frames[k])
            pt.render_passes(1)
            a = pt.accum()
            fresh[k] = a[..., :3].astype(np.float64) / a[..., 3:]
            q = frames[k].copy()
            q.samples_per_pixel, q.time = 64, 777777.0
            pt.reset()
            pt.set_params(q)
            pt.render_passes(16)
            a = pt.accum()
            truth[k] = a[..., :3].astype(np.float64) / a[..., 3:]
        pt.close()
        print("default scene %dx%d, depth 6, 4 spp per frame, truth 16 x 64 spp" % (w, h))
        for tol, cap_d, cap_o in SETTINGS:
            opt = abi.PtReprojectOptions(cap_d, cap_o, tol)
            pt = PathTracer(w, h)
            pt.set_spheres(sc.spheres)
            pt.feature_planes(True)
            pt.reproject_option(True)
            pt.set_params(frames[0])
            pt.render_features()
            pt.render_passes(1)
            out = []
            for k in range(1, 9):
                pt.keep_history()
                pt.set_params(frames[k])
                pt.render_features()
                pt.reproject(opt)
                pt.render_passes(1)
                if k in truth:
                    a, rs = pt.accum(), pt.reproject_stats()
                    both = a[..., :3].astype(np.float64) / a[..., 3:]
                    ratio = float(((both - truth[k]) ** 2).sum() / ((fresh[k] - truth[k]) ** 2).sum())
                    out.append("frame %d: %.3f (kept %.3f)" % (k, ratio, rs.pixels_kept / rs.pixels))
            pt.close()
            print("  tolerance %g px, caps %g / %g:  %s" % (tol, cap_d, cap_o, "   ".join(out)), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "cost":
        cost(args[1:] or list(CONFIGS))
    elif args and args[0] == "quality":
        quality([tuple(int(x) for x in a.split("x")) for a in args[1:]] or [(160, 88), (1280, 702)])
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
