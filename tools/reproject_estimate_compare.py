"""Dev tool: what carrying the error estimate through temporal reprojection costs and what it is worth, on an MI355X
(profiles/r21_reproject_estimate.txt).  A sibling of tools/reproject_compare.py.

    python tools/reproject_estimate_compare.py cost [default config2]
    python tools/reproject_estimate_compare.py quality [WIDTHxHEIGHT ...]        (default: 160x88 1280x702)

cost: per config at the bench size (default: 1280x702, config2: 1920x1080) one context with both options on, tuned, on a stream
of its own, samples_per_pixel = 1, a camera that steps sideways and back between two views, two passes per tick (so that the
state a call finds holds n >= 2 everywhere a pass was folded: what the gather has to read).  The tick is the header's; the call
in pt_reproject's place ALTERNATES between pt_reproject — kernel, staging copy and the state-sized memset of its clear: the
parent's call, its device code unchanged — and pt_reproject_estimate — kernel, staging copy, state copy.  A second context with
the estimate off times pt_reproject without the memset.  HIP events on the context's stream around the call alone; RUNS timed
calls of each after a warm-up of each; printed: the times, median and spread, and the bytes each moves per pixel.

quality: the eight-frame flight of tests/test_reproject_estimate_ref.py on the device (default scene, depth 6, 4 passes of 1 spp
per tick, tolerance 2 px, caps 32 / 8).  One context flies it with pt_reproject_estimate, a second renders each frame's fresh
passes alone (estimate on), a third the frame's truth, 16 x 64 spp at a clock of its own.  Printed at frames 1 / 4 / 8, squared
error over the squared error of the fresh samples unfiltered: the carried state through pt_resolve_filtered_patch(2, 1, 1.5), the
reprojected accumulation unfiltered, the fresh passes through the same filter; and the carried estimate's calibration,
sum (m - truth)^2 / sum se^2 over the known pixels."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ray_tracer_webgl_amd import abi, scenes  # noqa: E402
from ray_tracer_webgl_amd.tracer import PathTracer  # noqa: E402
from reproject_compare import flight_params  # noqa: E402

CONFIGS = {
    "default": lambda: scenes.default_scene(1280, 702, spp=1, max_depth=8),
    "config2": lambda: scenes.config2(1920, 1080, 1, 1, 50),
}
RUNS = 6
PASSES = 2


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
        for v in views:
            v.time_step = abi.PT_TIME_STEP_DECORRELATED
        for k in range(3):   # a hundredth of the view's width sideways: the camera and its image plane move together
            views[1].camera_origin[k] += 0.01 * sc.params.horizontal[k]
            views[1].lower_left_corner[k] += 0.01 * sc.params.horizontal[k]
        times = {"pt_reproject, estimate off": [], "pt_reproject + clear of the state": [], "pt_reproject_estimate": []}
        kept = known = 0.0
        with torch.cuda.stream(side):
            for estimate in (True, False):
                pt = PathTracer(sc.params.width, sc.params.height, use_torch=True)
                pt.set_spheres(sc.spheres)
                pt.set_params(views[0])
                pt.tune(1)
                pt.feature_planes(True)
                pt.reproject_option(True)
                if estimate:
                    pt.error_estimate(True)
                pt.reserve_passes(PASSES)
                pt.set_params(views[0])
                pt.render_features()
                pt.render_passes(PASSES)
                calls = (("pt_reproject + clear of the state", pt.reproject), ("pt_reproject_estimate", pt.reproject_estimate)) if estimate \
                    else (("pt_reproject, estimate off", pt.reproject),)
                for run in range((2 + RUNS) * len(calls)):   # two warm-up ticks of each: every code object loaded, every launch planned
                    key, call = calls[run % len(calls)]
                    pt.keep_history()
                    views[(run + 1) % 2].time = sc.params.time + 10.0 * (run + 1)
                    pt.set_params(views[(run + 1) % 2])
                    pt.render_features()
                    t = timed(side, lambda: call(opt))
                    if run >= 2 * len(calls):
                        times[key].append(t)
                    if key == "pt_reproject_estimate" and run == (2 + RUNS) * len(calls) - 1:
                        rs, st = pt.reproject_stats(), pt.error_state()
                        kept, known = rs.pixels_kept / max(rs.pixels, 1), float((st[..., 0, 3] >= 2).mean())
                    pt.render_passes(PASSES)
                pt.close()
        pix = sc.params.width * sc.params.height
        print("%s: %dx%d, %d spheres; the last pt_reproject_estimate kept %.3f of the frame's pixels, carried an estimate for %.3f" % (
            name, sc.params.width, sc.params.height, len(sc.spheres), kept, known))
        med = lambda v: float(np.median(v))
        for key, v in times.items():
            print("  %-34s ms: %s   median %.4f spread %.4f  (%.4f ns per pixel)" % (
                key, " ".join("%.4f" % x for x in v), med(v), max(v) - min(v), med(v) * 1e6 / pix))
        d = med(times["pt_reproject_estimate"]) - med(times["pt_reproject + clear of the state"])
        print("  pt_reproject_estimate - (pt_reproject + clear): %+.4f ms = %+.4f ns per pixel" % (d, d * 1e6 / pix), flush=True)


def quality(sizes):
    opt = abi.PtReprojectOptions()
    for w, h in sizes:
        sc = scenes.default_scene(w, h, spp=1, max_depth=6)
        p0 = sc.params.copy()
        p0.time, p0.time_step, p0.first_pass = 200.0, abi.PT_TIME_STEP_DECORRELATED, 0
        frames = [flight_params(p0, k) for k in range(9)]
        fresh, fresh_filtered, truth = {}, {}, {}
        pt = PathTracer(w, h)
        pt.set_spheres(sc.spheres)
        pt.error_estimate(True)
        pt.reserve_passes(16)
        for k in (1, 4, 8):
            pt.reset()
            pt.set_params(frames[k])
            pt.render_passes(4)
            a = pt.accum()
            fresh[k] = a[..., :3].astype(np.float64) / a[..., 3:]
            fresh_filtered[k] = pt.patch_filtered_image(2, 1, 1.5, gamma=False)[..., :3].astype(np.float64)
            q = frames[k].copy()
            q.samples_per_pixel, q.time = 64, 777777.0
            pt.reset()
            pt.set_params(q)
            pt.render_passes(16)
            a = pt.accum()
            truth[k] = a[..., :3].astype(np.float64) / a[..., 3:]
        pt.close()
        print("default scene %dx%d, depth 6, 4 passes of 1 spp per tick, tolerance %g px, caps %g / %g, truth 16 x 64 spp" % (
            w, h, opt.tolerance_px, opt.cap_diffuse, opt.cap_other))
        pt = PathTracer(w, h)
        pt.set_spheres(sc.spheres)
        pt.feature_planes(True)
        pt.reproject_option(True)
        pt.error_estimate(True)
        pt.reserve_passes(4)
        pt.set_params(frames[0])
        pt.render_features()
        pt.render_passes(4)
        for k in range(1, 9):
            pt.keep_history()
            pt.set_params(frames[k])   # (passes 0 .. 3 at the frame's own clock: the samples of `fresh`)
            pt.render_features()
            pt.reproject_estimate(opt)
            pt.render_passes(4)
            if k in truth:
                sq = lambda img: float(((img - truth[k]) ** 2).sum())
                a, st = pt.accum(), pt.error_state().astype(np.float64)
                carried = pt.patch_filtered_image(2, 1, 1.5, gamma=False)[..., :3].astype(np.float64)
                e_fresh = sq(fresh[k])
                n, kk = st[..., 0, 3], st[..., 1, 3]
                known = (n >= 2) & (kk > 0)
                qn = n[known] / kk[known]
                m = st[..., 0, :3][known] * qn[:, None]
                se2 = st[..., 1, :3][known] / (n[known] * (n[known] - 1))[:, None] * (qn * qn)[:, None]
                print("  frame %d: carried + filter %.3f   reprojected, unfiltered %.3f   fresh + filter %.3f   calibration %.2f   "
                      "(estimate known at %.3f of the frame)" % (
                          k, sq(carried) / e_fresh, sq(a[..., :3].astype(np.float64) / a[..., 3:]) / e_fresh,
                          sq(fresh_filtered[k]) / e_fresh, float(((m - truth[k][known]) ** 2).sum() / se2.sum()), known.mean()), flush=True)
        pt.close()


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
