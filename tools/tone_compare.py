#!/usr/bin/env python3
"""tone_compare.py — what exposure metering and the toned read-out cost beside pt_resolve_rgba8, and what they do to config 4.

    python3 tools/tone_compare.py --size 1920x1080 [--reps 20]     the three display kernels and pt_resolve_rgba8 on one frame
    python3 tools/tone_compare.py --config4 [--width W --height H --passes N]
                                                                  config 4's channel values at 255 under each read-out

The first form is meant to run under `rocprofv3 --kernel-trace --stats` (a run of its own): the kernels' device times are the
profiler's (pt_meter_kernel, pt_exposure_kernel, pt_tone_kernel beside pt_resolve_rgba8_kernel); what it prints itself are host
clocks around whole calls, which end in a synchronise and include the copy of the result to the host.  The frame is random linear
radiance over twelve octaves, so the histogram spreads over many bins; `--flat` meters a frame of one colour instead (every pixel in
one bin: the atomics' worst case)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ray_tracer_webgl_amd import abi, scenes  # noqa: E402
from ray_tracer_webgl_amd.tracer import PathTracer  # noqa: E402


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def frame_costs(w, h, reps, flat):
    sc = scenes.default_scene(w, h, spp=1, max_depth=4)
    t = PathTracer(w, h)
    t.set_spheres(sc.spheres)
    t.set_params(sc.params)
    t.tone_mapping(True)
    rng = np.random.default_rng(1)
    acc = np.empty((h, w, 4), np.float32)
    if flat:
        acc[..., :3] = np.float32([1.5, 0.75, 6.0])
    else:
        acc[..., :3] = (rng.random((h, w, 3)) * np.exp2(rng.integers(-6, 6, (h, w, 1)))).astype(np.float32) * 3.0
    acc[..., 3] = 3.0
    t.load_accum(acc)
    rows = []

    def meter():
        t.meter()
        t.synchronize()

    rows.append(("pt_meter + pt_synchronize (two kernels, no copy)", timed(meter, reps)))
    for name, curve in (("clamp", abi.PT_TONE_CLAMP), ("reinhard", abi.PT_TONE_REINHARD), ("filmic", abi.PT_TONE_FILMIC)):
        opt = abi.PtToneOptions(curve, 1, 0.0, 0.0)
        rows.append(("pt_resolve_toned_rgba8, %s, device record" % name, timed(lambda: t.toned_rgba8(opt), reps)))
    rows.append(("pt_resolve_toned (float), filmic", timed(lambda: t.toned_image(abi.PtToneOptions(abi.PT_TONE_FILMIC, 1, 0.0, 0.0)), reps)))
    rows.append(("pt_resolve_rgba8", timed(lambda: t.resolve_rgba8(True), reps)))
    rows.append(("pt_resolve (float)", timed(lambda: t.resolve(True), reps)))
    rec, hist = t.exposure()
    print("%dx%d, %s frame: %d bins in use, lit %d, below %d, exposure %g, white %g" % (
        w, h, "flat" if flat else "spread", int((hist > 0).sum()), rec.lit, rec.below, rec.exposure, rec.white))
    print("host clocks per call, ms (each call ends in a synchronise; the read-outs include the copy to host memory), %d calls each:" % reps)
    for name, ms in rows:
        print("  %-52s %8.3f" % (name, ms))
    t.close()


def config4_bytes(args):
    sc = scenes.config4() if not args.width else scenes.config4(width=args.width, height=args.height)
    if args.passes:
        sc.n_passes = args.passes
    p = sc.params
    t = PathTracer(p.width, p.height)
    t.set_spheres(sc.spheres)
    t.set_params(p)
    per = min(sc.n_passes, 16)
    t.reserve_passes(per)
    done = 0
    while done < sc.n_passes:
        k = min(per, sc.n_passes - done)
        q = p.copy()
        q.first_pass = done
        t.set_params(q)
        t.render_passes(k)
        done += k
    t.tone_mapping(True)
    t.meter()
    rec, hist = t.exposure()
    n = p.width * p.height * 3
    print("config 4, %dx%d, %d spp: metered exposure %g, white %g (key luminance %g, 99th percentile %g; %d lit pixels, %d below 2^-16)" % (
        p.width, p.height, t.stats().total_spp, rec.exposure, rec.white, rec.y_key, rec.y_high, rec.lit, rec.below))
    print("channel values at the byte 255 / at the bytes 0..3, of %d:" % n)
    outs = [("pt_resolve_rgba8 (sqrt, clamp)", t.resolve_rgba8(True))]
    for name, curve in (("clamp", abi.PT_TONE_CLAMP), ("reinhard", abi.PT_TONE_REINHARD), ("filmic", abi.PT_TONE_FILMIC)):
        outs.append(("pt_resolve_toned_rgba8 %s, metered exposure" % name, t.toned_rgba8(abi.PtToneOptions(curve, 1, 0.0, 0.0))))
    for name, img in outs:
        rgb = img[..., :3]
        print("  %-48s %8d  %8d" % (name, int((rgb == 255).sum()), int((rgb <= 3).sum())))
    t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--flat", action="store_true")
    ap.add_argument("--config4", action="store_true")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--passes", type=int)
    args = ap.parse_args()
    if args.config4:
        config4_bytes(args)
    else:
        w, h = (int(x) for x in args.size.split("x"))
        frame_costs(w, h, args.reps, args.flat)


if __name__ == "__main__":
    main()
