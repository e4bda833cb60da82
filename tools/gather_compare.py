#!/usr/bin/env python3
"""Dev tool: what pt_gather_irradiance / pt_bake_probes save beside the old way — rays built on the host, pt_query_radiance,
a numpy reduce — on 4 096 items of 256 directions (profiles/r31_gather.txt).

    python3 tools/gather_compare.py [config4 default]             the calls, timed
    python3 tools/gather_compare.py --once [config4 default]      one call of each kind after a warm-up: the run to trace
    python3 tools/gather_compare.py --trace DIR                   the kernel times of such a run from rocprofv3's kernel trace

Per config one context (tuned, ray queries on, 1 pass of 4 samples per ray at the config's depth) and 4 096 items: first hits
of the frame's own pixel rays (pt_query_rays), spread over the frame, with their normals.  Timed, alternated, five runs of each
after a warm-up of all, HIP events on the context's stream around the whole of each (the host's work included):
  gather, host arrays       pt_gather_irradiance: 4 096 PtGatherPoint up (128 KiB), 4 096 PtIrradiance down (64 KiB)
  probes, host arrays       pt_bake_probes: the same up, 4 096 PtProbeSH down (448 KiB)
  gather, device arrays     pt_gather_irradiance with both arrays in device memory
  the old way, irradiance   the 4 096 x 256 rays built in numpy (the same set, vectorised in float32), pt_query_radiance with
                            host arrays (32 MiB up, 16 MiB down), the records reduced in numpy (sum / samples, mean over j)
  the old way, rays given   the same without the building of the rays (a baker that keeps its rays)
Printed: the five times of each, median and spread (max - min), and the ratios of the medians.  The kernel times — the
generator's and the reduce's beside the trace launch's and the fold's — come from a traced run of --once (a run of its own:
tracing slows the host), summed per kernel over that run: the warm-up's calls and the traced ones, with the launches counted."""
import csv
import ctypes as C
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ITEMS, DIRECTIONS, SPP, RUNS = 4096, 256, 4, 5


def configs():
    from ray_tracer_webgl_amd import scenes

    return {"config4": lambda: scenes.config4(1024, 1024, n_passes=1), "default": lambda: scenes.default_scene(1280, 702)}


def timed(torch, stream, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


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


def host_rays(pos, nrm, D):
    """the old way's rays: the header's set, vectorised in numpy float32 (timing only: numpy's sin and cos, no fma)"""
    j = np.arange(D, dtype=np.uint64)
    a = ((2 * j + 1).astype(np.float32) / np.float32(D))
    with np.errstate(over="ignore"):
        u = ((j * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    s, c = np.sin(np.float32(2 * np.pi) * u), np.cos(np.float32(2 * np.pi) * u)
    h = a * np.float32(0.5)
    lx, ly, lz = np.sqrt(h) * c, np.sqrt(h) * s, np.sqrt(np.float32(1.0) - h)
    z = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    sg = np.copysign(np.float32(1.0), z[:, 2])
    q = np.float32(-1.0) / (sg + z[:, 2])
    b = z[:, 0] * z[:, 1] * q
    t = np.stack([np.float32(1.0) + sg * z[:, 0] * z[:, 0] * q, sg * b, -sg * z[:, 0]], axis=1)
    bt = np.stack([b, sg + z[:, 1] * z[:, 1] * q, -z[:, 1]], axis=1)
    w = z[:, None, :] * lz[None, :, None] + bt[:, None, :] * ly[None, :, None] + t[:, None, :] * lx[None, :, None]
    rays = np.zeros((len(pos), D, 8), np.float32)
    rays[:, :, 0:3] = pos[:, None, :]
    rays[:, :, 4:7] = w
    return rays.reshape(-1, 8)


def setup(name):
    import torch

    from ray_tracer_webgl_amd.tracer import PathTracer

    sc = configs()[name]()
    p = sc.params.copy()
    p.samples_per_pixel = SPP
    pt = PathTracer(p.width, p.height, use_torch=True)
    pt.set_spheres(sc.spheres)
    pt.set_params(p)
    pt.tune(1)
    pt.ray_queries(True)
    pt.set_params(p)
    o, d = pinhole(p)
    hits = pt.query_rays(o, d)
    on = np.flatnonzero(hits["index"] >= 0)
    pick = on[(np.arange(N_ITEMS) * 7919) % len(on)]
    pos = (hits["point"][pick] + np.float32(1e-3) * hits["normal"][pick]).astype(np.float32)
    nrm = np.ascontiguousarray(hits["normal"][pick], np.float32)
    items = np.zeros((N_ITEMS, 8), np.float32)
    items[:, 0:3], items[:, 4:7] = pos, nrm
    dev_items = torch.from_numpy(items).cuda()
    dev_out = torch.zeros((N_ITEMS, 4), dtype=torch.float32, device="cuda")
    e, sh = np.zeros((N_ITEMS, 4), np.float32), np.zeros((N_ITEMS, 28), np.float32)
    rec = np.zeros((N_ITEMS * DIRECTIONS, 4), np.float32)
    kept = host_rays(pos, nrm, DIRECTIONS)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def old(rays):
        pt._check(pt.lib.pt_query_radiance(pt._ctx, vp(rays), len(rays), 1, vp(rec)))
        r = rec.reshape(N_ITEMS, DIRECTIONS, 4)
        return np.float32(np.pi / DIRECTIONS) * (r[:, :, :3] / r[:, :, 3:4]).sum(axis=1)

    calls = [
        ("gather, host arrays", lambda: pt._check(pt.lib.pt_gather_irradiance(pt._ctx, vp(items), N_ITEMS, DIRECTIONS, 1, vp(e)))),
        ("probes, host arrays", lambda: pt._check(pt.lib.pt_bake_probes(pt._ctx, vp(items), N_ITEMS, DIRECTIONS, 1, vp(sh)))),
        ("gather, device arrays", lambda: pt._check(pt.lib.pt_gather_irradiance(pt._ctx, C.c_void_p(dev_items.data_ptr()), N_ITEMS, DIRECTIONS, 1,
                                                                                C.c_void_p(dev_out.data_ptr())))),
        ("the old way, irradiance", lambda: old(host_rays(pos, nrm, DIRECTIONS))),
        ("the old way, rays given", lambda: old(kept)),
    ]
    return torch, pt, p, sc, calls, e, old, kept


def measure(names, once):
    import torch

    side = torch.cuda.Stream()
    for name in names:
        with torch.cuda.stream(side):
            torch, pt, p, sc, calls, e, old, kept = setup(name)
            for _, call in calls:  # warm-up: every code object loaded, every launch planned once
                call()
            if once:
                for _, call in calls[:2] + calls[4:]:
                    call()
                pt.close()
                print("%s: one pt_gather_irradiance, one pt_bake_probes and one pt_query_radiance of %d x %d rays after a warm-up" % (
                    name, N_ITEMS, DIRECTIONS))
                continue
            times = {what: [] for what, _ in calls}
            for _ in range(RUNS):
                for what, call in calls:
                    times[what].append(timed(torch, side, call))
            # the two ways estimate the same thing (the host's rays are made with numpy's sin and cos: a direction off by a unit in
            # the last place can take another path, so they agree to the noise, not to the bit)
            agree = float(np.abs(old(kept) - e[:, :3]).max() / max(float(np.abs(e[:, :3]).max()), 1e-30))
            st = pt.stats()
            batch = pt.query_batch()
            pt.close()
        med = lambda v: float(np.median(v))
        print("%s: %dx%d, %d spheres, geometry path %d, %d items x %d directions, 1 pass of %d samples, depth %d, batches of %d rays" % (
            name, p.width, p.height, len(sc.spheres), st.geometry_path, N_ITEMS, DIRECTIONS, SPP, p.max_depth, batch))
        for what, _ in calls:
            v = times[what]
            print("  %-26s ms: %s   median %.3f spread %.3f" % (what, " ".join("%.3f" % x for x in v), med(v), max(v) - min(v)))
        g = med(times["gather, host arrays"])
        print("  the old way / gather (host arrays): %.3f with the rays built, %.3f with the rays given; gather from device arrays / from host arrays: %.3f" % (
            med(times["the old way, irradiance"]) / g, med(times["the old way, rays given"]) / g, med(times["gather, device arrays"]) / g))
        print("  largest difference between the two ways' irradiance, relative to the largest value: %.3g" % agree)
        sys.stdout.flush()


def trace_summary(path):
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit("no *kernel_trace.csv under %s" % path)
    groups = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0].replace(".kd", "")
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            groups.setdefault(name, []).append(us)
    print("kernel times of the traced run, summed per kernel over the whole run (us; launches):")
    for name in sorted(groups):
        if name.startswith("pt_gather") or name.endswith("_rad") or name in ("pt_radiance_fold_kernel", "pt_query_pack_kernel"):
            v = groups[name]
            print("  %-32s %12.1f us  %6d launches  %9.2f us each" % (name, sum(v), len(v), sum(v) / len(v)))


def main():
    args = sys.argv[1:]
    if args and args[0] == "--trace":
        return trace_summary(args[1])
    once = bool(args) and args[0] == "--once"
    names = [a for a in args if not a.startswith("--")] or ["config4", "default"]
    measure(names, once)


if __name__ == "__main__":
    main()
