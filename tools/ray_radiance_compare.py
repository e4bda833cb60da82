"""Dev tool: what pt_query_radiance costs beside a render pass, on the bench configs at the bench sizes
(profiles/r24_ray_radiance.txt).

    python tools/ray_radiance_compare.py [--parent-lib PATH] [config2 config4 config5 default]

Per config one context (tuned, on a stream of its own) and, alternated on it, four runs each after a warm-up of all:
  radiance, full batch   pt_query_radiance on the frame's own pinhole rays, one batch (the local pixel count), 1 pass of the
                         config's samples per pixel and depth, rays and records in device memory: the pack kernel, the radiance
                         build of the row, the fold kernel, and the synchronisation the call ends with
  passes(1)              pt_render_passes(1) + a synchronisation on the same context: the same number of paths from the same
                         pixels — with the jitter and the lens, without the door — and the accumulation's fold
  passes(1) (parent)     the same on a context of the PARENT commit's library, when --parent-lib names one (a build of the
                         parent tree; its trace kernels are this tree's, byte for byte: profiles/r24_kernel_identity.txt)
  radiance, n = 1        one ray from host memory — a probe — and from device memory
  radiance, n = 4096     from host memory and from device memory
Times are HIP events recorded on the context's stream around each call.  Printed: the four times of each, median and spread
(max - min) of each, the ratio of the medians, and the door's memory traffic priced at the HBM rate: per ray the pack kernel
moves 32 + 32 bytes, the item decode reads the ray's two texels (32), the fold reads them again with one slab texel and writes
the record (32 + 16 + 16); every sample start reads the two texels once more, from the cache.  Against that the render pass
folds its slab into the accumulation (16 + 16 + 16 bytes per pixel), which the radiance call does not."""
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
    "config2": lambda: scenes.config2(1920, 1080, n_passes=1),
    "config4": lambda: scenes.config4(1024, 1024, n_passes=1),
    "config5": lambda: scenes.config5(1920, 1080, n_passes=1),
    "default": lambda: scenes.default_scene(1280, 702),
}
RUNS = 4
HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s
DOOR_BYTES_PER_RAY = 64 + 32 + 64
FOLD_BYTES_PER_PIXEL = 48


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
            out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            host_out = np.zeros((4096, 4), np.float32)
            mid = host_rays[n // 2:n // 2 + 4096].copy()  # n = 1 and n = 4096: from the middle of the frame, the same rays from either memory
            mid_dev = rays[n // 2:n // 2 + 4096].contiguous()

            def radiance(count, host=False):
                if host:
                    pt._check(pt.lib.pt_query_radiance(pt._ctx, mid.ctypes.data_as(C.c_void_p), count, 1, host_out.ctypes.data_as(C.c_void_p)))
                else:
                    src = rays if count == n else mid_dev
                    pt._check(pt.lib.pt_query_radiance(pt._ctx, C.c_void_p(src.data_ptr()), count, 1, C.c_void_p(out.data_ptr())))

            def passes(t):
                t.render_passes(1)
                t.synchronize()

            calls = [("radiance, full batch", lambda: radiance(n)), ("passes(1)", lambda: passes(pt))]
            if old is not None:
                calls.append(("passes(1) (parent)", lambda: passes(old)))
            calls += [("radiance, n = 1, host", lambda: radiance(1, True)), ("radiance, n = 1", lambda: radiance(1)),
                      ("radiance, n = 4096, host", lambda: radiance(4096, True)), ("radiance, n = 4096", lambda: radiance(4096))]
            for _ in range(2):  # warm-up: every code object loaded, every launch planned once
                for _, call in calls:
                    call()
            times = {what: [] for what, _ in calls}
            for _ in range(RUNS):
                for what, call in calls:
                    times[what].append(timed(side, call))
            st = pt.stats()
            radiance(n)
            samples = float(out[:, 3].min().item()), float(out[:, 3].max().item())
            if old is not None:
                old.close()
            pt.close()
        print("%s: %dx%d, %d spheres, geometry path %d, %d spp, depth %d, %d rays in a full batch (samples per record %g .. %g)" % (
            name, p.width, p.height, len(sc.spheres), st.geometry_path, p.samples_per_pixel, p.max_depth, n, samples[0], samples[1]))
        for what, _ in calls:
            v = times[what]
            print("  %-24s ms: %s   median %.4f spread %.4f" % (what, fmt(v), med(v), spread(v)))
        door = n * DOOR_BYTES_PER_RAY / HBM_BYTES_PER_S * 1e3
        fold = n * FOLD_BYTES_PER_PIXEL / HBM_BYTES_PER_S * 1e3
        ref = "passes(1) (parent)" if old is not None else "passes(1)"
        full = med(times["radiance, full batch"])
        print("  radiance, full batch / %s %.3f   difference %+.4f ms   the door's %d bytes per ray at 8 TB/s: %.4f ms; the pass's own fold, %d bytes per pixel: %.4f ms" % (
            ref, full / med(times[ref]), full - med(times[ref]), DOOR_BYTES_PER_RAY, door, FOLD_BYTES_PER_PIXEL, fold))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
