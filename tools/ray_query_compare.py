"""Dev tool: what the door of pt_query_rays costs, on the bench configs at the bench sizes (profiles/r23_ray_queries.txt).

    python tools/ray_query_compare.py [--parent-lib PATH] [config2 config4 config5 default]

Per config one context (tuned, on a stream of its own) and, alternated on it, four runs each after a warm-up of all:
  query, full batch    pt_query_rays on the frame's own pinhole rays, one batch (the local pixel count), rays and records in
                       device memory: the pack kernel, the query build of the kernel pt_render_features launches, the unpack kernel,
                       and the synchronisation the call ends with
  features             pt_render_features + a synchronisation on the same context: the same rays through the same walk without
                       the door
  features (parent)    the same on a context of the PARENT commit's library, when --parent-lib names one (a build of the
                       parent tree; its feature kernels are this tree's, byte for byte: profiles/r23_device_code.txt)
  query, n = 1         one ray from host memory — a pick — and from device memory
  query, n = 4096      from device memory
Times are HIP events recorded on the context's stream around each call.  Printed: the four times of each, median and spread
(max - min) of each, the ratio of the medians, and the door's memory traffic priced at the HBM rate: per ray the pack kernel
moves 32 + 32 bytes, the unpack kernel 64 + 64, and the query build reads its two texels twice (at the item's decode and at the
ray's start), 64 bytes that the feature build computes instead."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ray_tracer_webgl_amd import scenes, tracer  # noqa: E402
from ray_tracer_webgl_amd._lib import SIGNATURES  # noqa: E402
from ray_tracer_webgl_amd.tracer import PathTracer  # noqa: E402

CONFIGS = {
    "config2": lambda: scenes.config2(1920, 1080, 1, 1, 1),
    "config4": lambda: scenes.config4(1024, 1024, 1, 1, 1),
    "config5": lambda: scenes.config5(1920, 1080, 1, 1, 1),
    "default": lambda: scenes.default_scene(1280, 702, spp=1, max_depth=1),
}
RUNS = 4
HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s
DOOR_BYTES_PER_RAY = 64 + 128 + 64


def timed(stream, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def pinhole_rays(p):
    """(n, 8) float32 PtRay records of the frame's pixel centres (timing only: rounded once from float64)"""
    w, h = int(p.width), int(p.height)
    s = ((2.0 * np.arange(w) + 1.0) / w)[None, :] * 0.5
    t = ((2.0 * np.arange(h) + 1.0) / h)[:, None] * 0.5
    rays = np.zeros((h, w, 8), np.float32)
    for c in range(3):
        rays[..., c] = p.camera_origin[c]
        rays[..., 4 + c] = p.lower_left_corner[c] + s * p.horizontal[c] + t * p.vertical[c] - p.camera_origin[c]
    return rays.reshape(h * w, 8)


def other_library(path):
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def context(sc, p, lib=None, queries=True):
    if lib is not None:  # a context of another build of the library (the parent's): PathTracer asks tracer.load for it
        keep, tracer.load = tracer.load, (lambda: lib)
    try:
        pt = PathTracer(p.width, p.height, use_torch=True)
    finally:
        if lib is not None:
            tracer.load = keep
    pt.set_spheres(sc.spheres)
    pt.set_params(p)
    pt.tune(1)
    pt.feature_planes(True)
    if queries:
        pt.ray_queries(True)
    pt.set_params(p)
    return pt


def main():
    args = sys.argv[1:]
    parent = None
    if args and args[0] == "--parent-lib":
        parent = other_library(args[1])
        args = args[2:]
    names = args or list(CONFIGS)
    side = torch.cuda.Stream()
    med = lambda v: float(np.median(v))
    spread = lambda v: float(max(v) - min(v))
    fmt = lambda v: " ".join("%.4f" % x for x in v)
    for name in names:
        sc = CONFIGS[name]()
        p = sc.params.copy()
        with torch.cuda.stream(side):
            pt = context(sc, p)
            old = context(sc, p, parent, queries=False) if parent is not None else None
            host_rays = pinhole_rays(p)
            n = len(host_rays)
            assert pt.query_batch() == n
            rays = torch.from_numpy(host_rays).cuda()
            hits = torch.zeros((n, 16), dtype=torch.int32, device="cuda")
            one_ray, one_hit = host_rays[n // 2:n // 2 + 1].copy(), np.zeros((1, 16), np.int32)

            def query(count, host=False):
                if host:
                    pt._check(pt.lib.pt_query_rays(pt._ctx, one_ray.ctypes.data_as(C.c_void_p), 1, one_hit.ctypes.data_as(C.c_void_p)))
                else:
                    pt._check(pt.lib.pt_query_rays(pt._ctx, C.c_void_p(rays.data_ptr()), count, C.c_void_p(hits.data_ptr())))

            def features(t):
                t.render_features()
                t.synchronize()

            calls = [("query, full batch", lambda: query(n)), ("features", lambda: features(pt))]
            if old is not None:
                calls.append(("features (parent)", lambda: features(old)))
            calls += [("query, n = 1, host", lambda: query(1, True)), ("query, n = 1", lambda: query(1)), ("query, n = 4096", lambda: query(4096))]
            for _ in range(2):  # warm-up: every code object loaded, every launch planned once
                for _, call in calls:
                    call()
            times = {what: [] for what, _ in calls}
            for _ in range(RUNS):
                for what, call in calls:
                    times[what].append(timed(side, call))
            st = pt.stats()
            same = None
            if old is not None:  # the two libraries' planes, while both contexts are alive
                same = all(torch.equal(a, b) for a, b in zip(pt.features().values(), old.features().values()))
                old.close()
            pt.close()
        print("%s: %dx%d, %d spheres, geometry path %d, %d rays in a full batch" % (name, p.width, p.height, len(sc.spheres), st.geometry_path, n))
        for what, _ in calls:
            v = times[what]
            print("  %-20s ms: %s   median %.4f spread %.4f" % (what, fmt(v), med(v), spread(v)))
        door = n * DOOR_BYTES_PER_RAY / HBM_BYTES_PER_S * 1e3
        ref = "features (parent)" if old is not None else "features"
        print("  query, full batch / %s %.3f   difference %.4f ms   the door's %d bytes per ray at 8 TB/s: %.4f ms" % (
            ref, med(times["query, full batch"]) / med(times[ref]), med(times["query, full batch"]) - med(times[ref]), DOOR_BYTES_PER_RAY, door))
        if same is not None:
            print("  the parent library's feature planes equal this library's: %s" % same)
        sys.stdout.flush()


if __name__ == "__main__":
    main()
