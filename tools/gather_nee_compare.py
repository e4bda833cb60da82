#!/usr/bin/env python3
"""Dev tool: what the next-event estimator buys and costs at a GATHER point — pt_gather_irradiance_nee beside
pt_gather_irradiance — measured on one device: writes profiles/r32_gather_nee.txt.

    python3 tools/gather_nee_compare.py [--out FILE] [--trace-summary FILE]    the errors and the calls' times
    python3 tools/gather_nee_compare.py --once                      one call of each kind per scene after a warm-up: the run to trace
    python3 tools/gather_nee_compare.py --trace DIR                 the kernel times of such a run from rocprofv3's kernel trace
                                                                    (rocprofv3 --kernel-trace --output-format csv -d DIR -- ... --once)

Two scenes, BASELINE config 4 and the two-light room of tests/nee_scenes.py, at 256 x 256 (a batch is 65 536 rays: one launch
per call), depth as the scene has it.  256 points on the scene's DIFFUSE surfaces — first hits of the frame's own pixel rays
(pt_query_rays), spread over the frame, lifted 1e-3 along the normal — x 256 directions, PASSES passes of SPP samples per ray.
  squared error   the irradiance of the plain and of the lit gather at EQUAL SAMPLES against a PLAIN-estimator reference of 64 x
                  the samples (passes far from the ones under test), mean over points and channels; REPEATS disjoint runs
                  of passes after a warm-up, the median
  time            each call's wall time on the host (the calls are synchronous), the median; from the two the plain error at
                  EQUAL TIME, by the 1 / samples law of a mean's variance: plain error x (plain time / lit time)
  kernel share    the _rad_nee launch's time beside the _rad launch's on the same batch, from a traced run of --once"""
import argparse
import csv
import ctypes as C
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZE, N_ITEMS, DIRECTIONS, SPP, PASSES, REPEATS, REF_FACTOR = 256, 256, 256, 4, 2, 5, 64


def the_scenes():
    import nee_scenes
    from ray_tracer_webgl_amd import scenes

    return [("config 4", scenes.config4(SIZE, SIZE, SPP, PASSES, 50)), ("the two-light room", nee_scenes.two_light_room(SIZE, SIZE, SPP, PASSES, 6))]


def pinhole(p):
    """(origins, directions) of the frame's pixel centres, float32"""
    w, h = int(p.width), int(p.height)
    s = ((2.0 * np.arange(w) + 1.0) / w)[None, :] * 0.5
    t = ((2.0 * np.arange(h) + 1.0) / h)[:, None] * 0.5
    o, d = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)
    for c in range(3):
        o[..., c] = p.camera_origin[c]
        d[..., c] = p.lower_left_corner[c] + s * p.horizontal[c] + t * p.vertical[c] - p.camera_origin[c]
    return o.reshape(-1, 3), d.reshape(-1, 3)


def setup(sc):
    from ray_tracer_webgl_amd import abi
    from ray_tracer_webgl_amd.tracer import PathTracer

    p = sc.params.copy()
    p.samples_per_pixel, p.time_step = SPP, abi.PT_TIME_STEP_DECORRELATED
    pt = PathTracer(p.width, p.height)
    pt.set_spheres(sc.spheres)
    pt.set_params(p)
    pt.reserve_passes(16)
    pt.tune(1)
    pt.ray_queries(True)
    pt.next_event(True)
    pt.set_params(p)
    o, d = pinhole(p)
    hits = pt.query_rays(o, d)
    on = np.flatnonzero((hits["index"] >= 0) & (hits["type"] == abi.PT_DIFFUSE))
    pick = on[(np.arange(N_ITEMS) * 7919) % len(on)]
    items = np.zeros((N_ITEMS, 8), np.float32)
    items[:, 0:3] = hits["point"][pick] + np.float32(1e-3) * hits["normal"][pick]
    items[:, 4:7] = hits["normal"][pick]
    return pt, p, items


def gather(pt, p, items, fn, first_pass, n_passes):
    """(the irradiance (n, 3) float64, the call's seconds)"""
    q = p.copy()
    q.first_pass = first_pass
    pt.set_params(q)
    e = np.zeros((N_ITEMS, 4), np.float32)
    t0 = time.perf_counter()
    pt._check(fn(pt._ctx, items.ctypes.data_as(C.c_void_p), N_ITEMS, DIRECTIONS, n_passes, e.ctypes.data_as(C.c_void_p)))
    dt = time.perf_counter() - t0
    assert (e[:, 3] == DIRECTIONS * n_passes * SPP).all()
    return e[:, :3].astype(np.float64), dt


def measure(once, out):
    for name, sc in the_scenes():
        pt, p, items = setup(sc)
        try:
            plain_fn, lit_fn = pt.lib.pt_gather_irradiance, pt.lib.pt_gather_irradiance_nee
            for fn in (plain_fn, lit_fn):  # warm-up: both code objects loaded, both launches planned once
                gather(pt, p, items, fn, 0, PASSES)
            if once:
                for fn in (plain_fn, lit_fn):
                    gather(pt, p, items, fn, 0, PASSES)
                out.append("%s: one pt_gather_irradiance and one pt_gather_irradiance_nee of %d x %d rays, %d passes of %d samples, after a warm-up of each" % (
                    name, N_ITEMS, DIRECTIONS, PASSES, SPP))
                continue
            # the reference: plain, REF_FACTOR x the samples, in calls of 16 passes far from the passes under test
            calls = REF_FACTOR * PASSES // 16
            assert calls * 16 == REF_FACTOR * PASSES
            ref = np.mean([gather(pt, p, items, plain_fn, (1 << 20) + 16 * k, 16)[0] for k in range(calls)], axis=0)
            rows = []
            for r in range(REPEATS):
                first = 1000 + r * 4 * PASSES
                e_plain, t_plain = gather(pt, p, items, plain_fn, first, PASSES)
                e_lit, t_lit = gather(pt, p, items, lit_fn, first, PASSES)
                rows.append((float(np.mean((e_plain - ref) ** 2)), float(np.mean((e_lit - ref) ** 2)), t_plain * 1e3, t_lit * 1e3))
            m = np.median(np.asarray(rows), axis=0)
            st = pt.stats()
            out.append("%s: %d spheres, %dx%d, geometry path %d, %d points x %d directions, %d passes of %d samples, depth %d; reference: plain, %d x the samples" % (
                name, len(sc.spheres), p.width, p.height, st.geometry_path, N_ITEMS, DIRECTIONS, PASSES, SPP, p.max_depth, REF_FACTOR))
            out.append("  mean irradiance of the reference %s" % np.array2string(ref.mean(axis=0), precision=4))
            out.append("  squared error, equal samples (median of %d): plain %.4e, lit %.4e (plain / lit %.2f)" % (REPEATS, m[0], m[1], m[0] / m[1]))
            out.append("  time of a call (median of %d): plain %.3f ms, lit %.3f ms (x %.2f)" % (REPEATS, m[2], m[3], m[3] / m[2]))
            eq = m[0] * m[2] / m[3]
            out.append("  squared error, equal time (plain error x plain time / lit time): plain %.4e, lit %.4e (plain / lit %.2f)%s" % (
                eq, m[1], eq / m[1], "" if eq > m[1] else "  <- WORSE at equal time here"))
            out.append("  (the reference's own error is about 1/%d of the plain gather's: %.1e)" % (REF_FACTOR, m[0] / REF_FACTOR))
        finally:
            pt.close()


def trace_summary(path):
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit("no *kernel_trace.csv under %s" % path)
    groups = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0].replace(".kd", "")
            groups.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    lines = ["kernel times of the traced run of --once, per kernel over the whole run (us; launches; the warm-up's calls and the traced ones):"]
    for name in sorted(groups):
        if name.startswith("pt_gather") or name.endswith("_rad") or name.endswith("_rad_nee") or name == "pt_radiance_fold_kernel":
            v = groups[name]
            lines.append("  %-40s %12.1f us  %4d launches  %10.2f us each (median %.2f)" % (name, sum(v), len(v), sum(v) / len(v), float(np.median(v))))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--trace", help="print the kernel times from the rocprofv3 kernel trace under this directory")
    ap.add_argument("--trace-summary", help="a file holding such a summary, appended to the report")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32_gather_nee.txt"))
    args = ap.parse_args()
    if args.trace:
        print("\n".join(trace_summary(args.trace)))
        return
    out = []
    if not args.once:
        out += ["pt_gather_irradiance_nee beside pt_gather_irradiance (tools/gather_nee_compare.py), one MI355X.",
                "Host arrays; errors in linear irradiance, mean over points and channels; times are the synchronous calls' wall times after a warm-up.", ""]
    measure(args.once, out)
    if not args.once and args.trace_summary and os.path.exists(args.trace_summary):
        out += [""] + open(args.trace_summary).read().splitlines()
    text = "\n".join(out) + "\n"
    print(text)
    if not args.once:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
