#!/usr/bin/env python3
"""glare_compare.py — what the glare pyramid costs beside the toned read-out's float kernel, and what it does to config 4.

    python3 tools/glare_compare.py --size 1920x1080 --levels 6 [--reps 20]   pt_glare and pt_resolve_toned (float) on one frame
    python3 tools/glare_compare.py --trace DIR --size 1920x1080 --levels 6   the kernel times of such a run from rocprofv3's trace
    python3 tools/glare_compare.py --config4 [--width W --height H --passes N]
                                                                            config 4's channel values at 255 with and without glare

The first form is meant to run under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR` (a run of its own per level
count); source and destination are device tensors, so a call is its kernels and one device-to-device copy.  The second form
reads DIR's kernel trace, groups the dispatches by kernel and grid (the down and gather launches of one call differ in their
grids, level by level) and sets each group beside the bytes it has to move and beside pt_tone_kernel's rate in the same run.
THE TRAFFIC MODEL, 16 bytes a texel: down k reads level k - 1 (the source for k = 1) and writes level k; gather k reads and
writes level k and reads level k + 1 (below the top); composite reads the source and level 1 and writes the frame.  Halo and
re-read texels are counted once: they are the caches' to serve."""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ray_tracer_webgl_amd import abi, scenes  # noqa: E402
from ray_tracer_webgl_amd.tracer import PathTracer  # noqa: E402


def default_weights(levels):
    """the header's weights over `levels` levels, rescaled to add up to 1 (render.py's rule)"""
    from ray_tracer_webgl_amd.render import glare_options

    return glare_options(abi.PT_GLARE_STRENGTH_DEFAULT, levels, 0.0)


def level_sizes(w, h, levels):
    out = [(w, h)]
    for _ in range(levels):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def frame_costs(w, h, levels, reps):
    import torch

    sc = scenes.default_scene(w, h, spp=1, max_depth=4)
    t = PathTracer(w, h, use_torch=True)
    t.set_spheres(sc.spheres)
    t.set_params(sc.params)
    t.glare(True)
    t.tone_mapping(True)
    rng = np.random.default_rng(1)
    lin = np.ones((h, w, 4), np.float32)
    lin[..., :3] = (rng.random((h, w, 3)) * np.exp2(rng.integers(-6, 6, (h, w, 1)))).astype(np.float32) * 3.0
    dev = torch.from_numpy(lin).cuda()
    opt = default_weights(levels)
    tone = abi.PtToneOptions(abi.PT_TONE_FILMIC, 1, 1.0, 1.0)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) / reps * 1e3

    rows = [("pt_glare, %d levels, device to device" % levels, timed(lambda: t.glared_image(dev, opt))),
            ("pt_resolve_toned (float), filmic, device to device", timed(lambda: t.toned_image(tone, dev)))]
    print("%dx%d, %d levels: host clocks per call, ms (each call ends in a synchronise), %d calls each:" % (w, h, levels, reps))
    for name, ms in rows:
        print("  %-56s %8.3f" % (name, ms))
    t.close()


def trace_summary(path, w, h, levels):
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit("no *kernel_trace.csv under %s" % path)
    groups = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0].replace(".kd", "")
            if not (name.startswith("pt_glare") or name == "pt_tone_kernel"):
                continue
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            groups.setdefault((name, int(r["Grid_Size_X"])), []).append(us)
    sizes = level_sizes(w, h, levels)
    texels = [a * b for a, b in sizes]
    grid_px = lambda n: min((n + 255) // 256, 2048) * 256
    grid_tiles = lambda a, b: min(((a + 15) // 16) * ((b + 15) // 16), 2048) * 256
    model = {("pt_tone_kernel", grid_px(texels[0])): ("frame in, frame out", 32 * texels[0]),
             ("pt_glare_composite_kernel", grid_px(texels[0])): ("source + level 1 in, frame out", 32 * texels[0] + 16 * texels[1])}
    for k in range(1, levels + 1):
        key = ("pt_glare_down_kernel", grid_tiles(*sizes[k]))
        what, b = model.get(key, ("", 0))
        model[key] = ((what + " + " if what else "") + "down %d" % k, b + 16 * (texels[k - 1] + texels[k]))
        key = ("pt_glare_gather_kernel", grid_px(texels[k]))
        what, b = model.get(key, ("", 0))
        model[key] = ((what + " + " if what else "") + "gather %d" % k, b + 16 * (2 * texels[k] + (texels[k + 1] if k < levels else 0)))
    tone = [v for (n, g), v in groups.items() if n == "pt_tone_kernel"]
    tone_rate = None
    if tone:
        tone_rate = 32 * texels[0] / (sum(tone[0][1:]) / max(len(tone[0]) - 1, 1)) / 1e3   # GB/s, the first (cold) launch left out
    print("%dx%d, %d levels; per kernel and grid (threads): launches, average / min / max us (the first launch of each left out of the "
          "average), the model's bytes, GB/s, and that rate over pt_tone_kernel's" % (w, h, levels))
    total = 0.0
    for (name, grid), v in sorted(groups.items(), key=lambda kv: (kv[0][0], -kv[0][1])):
        body = v[1:] if len(v) > 1 else v
        avg = sum(body) / len(body)
        what, b = model.get((name, grid), ("?", 0))
        rate = b / avg / 1e3 if b else 0.0
        # (a group that holds several levels' launches — small levels share the one-workgroup grid — averages over them all)
        per_call = len(v) / max(len(tone[0]) if tone else 1, 1)
        if name.startswith("pt_glare"):
            total += avg * per_call
        print("  %-28s %8d  %4d launches  %8.2f  %8.2f  %8.2f us   %-34s %11d B  %8.1f GB/s  %s" % (
            name, grid, len(v), avg, min(v), max(v), what, b, rate, ("%.2f" % (rate / tone_rate)) if tone_rate and b else "-"))
    whole = 16 * (3 * texels[0] + 4 * sum(texels[1:]))   # the source read twice, the frame written once, the pyramid written twice and read twice
    print("  the glare kernels of one call: %.2f us; the whole call's traffic (source read twice, frame written once, pyramid written and read "
          "twice: %d B) at pt_tone_kernel's rate: %s us" % (total, whole, ("%.2f" % (whole / tone_rate / 1e3)) if tone_rate else "-"))


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
    t.glare(True)
    n = p.width * p.height * 3
    print("config 4, %dx%d, %d spp; channel values at the byte 255, of %d, and the brightest linear channel value:" % (p.width, p.height, t.stats().total_spp, n))
    plain = t.resolve(False)
    variants = [("no glare", None)]
    variants.append(("default glare (strength 0.15, 6 levels)", abi.PtGlareOptions()))
    for s in (0.05, 0.3):
        variants.append(("glare strength %g, 6 levels" % s, abi.PtGlareOptions(strength=s)))
    variants.append(("glare strength 0.15, threshold 1", abi.PtGlareOptions(threshold=1.0)))
    for name, opt in variants:
        frame = plain if opt is None else t.glared_image(None, opt)
        t.meter(src=frame)
        rec, _ = t.exposure()
        line = "  %-42s exposure %-8g white %-8g max %-9.4g" % (name, rec.exposure, rec.white, float(frame[..., :3].max()))
        for cname, curve in (("reinhard", abi.PT_TONE_REINHARD), ("filmic", abi.PT_TONE_FILMIC)):
            img = t.toned_rgba8(abi.PtToneOptions(curve, 1, 0.0, 0.0), src=frame)
            line += "  %s %7d" % (cname, int((img[..., :3] == 255).sum()))
        print(line)
    # the veil itself, which a count of 255s cannot show: both frames toned with the exposure and white metered on the plain frame
    t.meter(src=plain)
    tone = abi.PtToneOptions(abi.PT_TONE_REINHARD, 1, 0.0, 0.0)
    base = t.toned_rgba8(tone, src=plain)[..., :3].astype(np.int32)
    print("the veil under Reinhard at the plain frame's exposure: channel bytes raised by >= 1 / >= 4 / >= 16, lowered by >= 1, of %d:" % n)
    for name, opt in variants[1:]:
        d = t.toned_rgba8(tone, src=t.glared_image(None, opt))[..., :3].astype(np.int32) - base
        print("  %-42s %8d %8d %8d  %8d" % (name, int((d >= 1).sum()), int((d >= 4).sum()), int((d >= 16).sum()), int((d <= -1).sum())))
    t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--levels", type=int, default=abi.PT_GLARE_LEVELS_DEFAULT)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace")
    ap.add_argument("--config4", action="store_true")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--passes", type=int)
    args = ap.parse_args()
    w, h = (int(x) for x in args.size.split("x"))
    if args.config4:
        config4_bytes(args)
    elif args.trace:
        trace_summary(args.trace, w, h, args.levels)
    else:
        frame_costs(w, h, args.levels, args.reps)


if __name__ == "__main__":
    main()
