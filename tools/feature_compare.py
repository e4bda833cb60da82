"""Dev tool: what pt_render_features costs beside the cheapest pass, on the bench configs at the bench sizes
(profiles/r15_features.txt).

    python tools/feature_compare.py [config2 config4 config5 default]

Per config one context (tuned, on a stream of its own) with samples_per_pixel = 1 and max_depth = 1, and two launches
alternated on it, four runs each after a warm-up of both:
  features   pt_render_features: one pinhole segment per pixel, four 16-byte texels written per pixel
  pass       pt_render_passes(1): the parent's way to spend one segment per pixel through the same walk — jitter and lens
             draws, one 16-byte slab texel per pixel; the span also holds the fold of the slab into the accumulation, so the
             trace kernel alone is printed beside it from the library's own events (PtStats.render_kernel_ms)
Times are HIP events recorded on the context's stream around each call.  Printed: the four times of each, median and spread
(max - min) of each, the ratio of the medians."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ray_tracer_webgl_amd import scenes  # noqa: E402
from ray_tracer_webgl_amd.tracer import PathTracer  # noqa: E402

CONFIGS = {
    "config2": lambda: scenes.config2(1920, 1080, 1, 1, 1),
    "config4": lambda: scenes.config4(1024, 1024, 1, 1, 1),
    "config5": lambda: scenes.config5(1920, 1080, 1, 1, 1),
    "default": lambda: scenes.default_scene(1280, 702, spp=1, max_depth=1),
}
RUNS = 4


def timed(stream, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def main():
    names = sys.argv[1:] or list(CONFIGS)
    side = torch.cuda.Stream()
    for name in names:
        sc = CONFIGS[name]()
        p = sc.params.copy()
        with torch.cuda.stream(side):
            pt = PathTracer(p.width, p.height, use_torch=True)
            pt.set_spheres(sc.spheres)
            pt.set_params(p)
            pt.tune(1)
            pt.feature_planes(True)
            pt.set_params(p)
            for _ in range(2):  # warm-up: both code objects loaded, both launches planned once
                pt.render_features()
                pt.render_passes(1)
            pt.synchronize()
            feat, whole, trace = [], [], []
            for _ in range(RUNS):
                feat.append(timed(side, pt.render_features))
                ms0 = pt.stats().render_kernel_ms
                whole.append(timed(side, lambda: pt.render_passes(1)))
                trace.append(pt.stats().render_kernel_ms - ms0)
            st = pt.stats()
            pt.close()
        med = lambda v: float(np.median(v))
        spread = lambda v: float(max(v) - min(v))
        fmt = lambda v: " ".join("%.4f" % x for x in v)
        print("%s: %dx%d, %d spheres, geometry path %d" % (name, p.width, p.height, len(sc.spheres), st.geometry_path))
        print("  features            ms: %s   median %.4f spread %.4f" % (fmt(feat), med(feat), spread(feat)))
        print("  pass (trace + fold) ms: %s   median %.4f spread %.4f" % (fmt(whole), med(whole), spread(whole)))
        print("  pass (trace kernel) ms: %s   median %.4f spread %.4f" % (fmt(trace), med(trace), spread(trace)))
        print("  features / pass (trace + fold) %.3f   features / pass (trace kernel) %.3f" % (
            med(feat) / med(whole), med(feat) / med(trace)), flush=True)


if __name__ == "__main__":
    main()
