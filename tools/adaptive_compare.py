"""Dev tool: pt_render_adaptive against pt_render_until at one noise target per config, at the bench sizes
(profiles/r11_ab_runs.txt).  pt_render_until is the yardstick.

    python tools/adaptive_compare.py [config2 config4 config5 default]

Per config: (1) a context renders a quarter of the config's spp through pt_render_until with a target it cannot meet; the
rel_error it ends with is THE TARGET.  (2) A fresh context renders to that target with pt_render_until (it stops at the same
pass, being the same frame), (3) another with pt_render_adaptive, both with at most the config's whole spp.  Printed: passes,
rounds, camera samples traced against pixels x passes x spp, the summed kernel time of the library's HIP events, the wall
time of the call (after a warm-up render and a clear in the same context, so neither pays the first launch's set-up).
Every launch is the library's own synchronous loop; nothing here is timed across processes."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ray_tracer_webgl_amd import abi, scenes  # noqa: E402
from ray_tracer_webgl_amd.tracer import PathTracer  # noqa: E402

# name: (scene at the bench size with 16-spp passes, passes of the config's whole spp)
CONFIGS = {
    "config2": (lambda: scenes.config2(1920, 1080, 16, 64, 50), 64),
    "config4": (lambda: scenes.config4(1024, 1024, 16, 512, 50), 512),
    "config5": (lambda: scenes.config5(1920, 1080, 16, 16, 50), 16),
    "default": (lambda: scenes.default_scene(1280, 702, spp=16, max_depth=8), 64),
}


def context(sc, p, per_round):
    pt = PathTracer(p.width, p.height)
    pt.set_spheres(sc.spheres)
    pt.set_params(p)
    pt.reserve_passes(per_round)
    pt.tune(min(per_round, 8))
    pt.error_estimate(True)
    pt.render_passes(per_round)   # warm-up: code objects, the order kernel, the autotuner's cold launch
    pt.reset()
    pt.set_params(p)
    return pt


def main():
    names = sys.argv[1:] or list(CONFIGS)
    for name in names:
        make, whole = CONFIGS[name]
        sc = make()
        p = sc.params.copy()
        p.time_step, p.first_pass = abi.PT_TIME_STEP_DECORRELATED, 0
        quarter = whole // 4
        per_round = max(1, quarter // 8)
        pt = context(sc, p, per_round)
        es = pt.render_until(1e-30, per_round, quarter)
        # (the ABI's target is a float: the smallest one not below the figure, or the same frame would miss it by a rounding)
        t32 = np.float32(es.rel_error)
        target = float(t32 if float(t32) >= es.rel_error else np.nextafter(t32, np.float32(np.inf)))
        pt.close()
        print("%s: %dx%d, 16 spp per pass, %d passes per round; target = rel_error after %d passes = %.6f" % (
            name, p.width, p.height, per_round, quarter, target), flush=True)
        rows = []
        for kind in ("until", "adaptive"):
            pt = context(sc, p, per_round)
            t0 = time.perf_counter()
            if kind == "until":
                es, ad = pt.render_until(target, per_round, whole), None
            else:
                es, ad = pt.render_adaptive(target, per_round, whole)
            wall = (time.perf_counter() - t0) * 1e3
            st = pt.stats()
            uniform = es.pixels * es.passes_rendered * p.samples_per_pixel
            rows.append((kind, es, ad, st, wall, uniform))
            print("  %-8s passes %3d reached %d rel_error %.6f  launches %3d%s  samples %.4g of %.4g uniform (%.1f %%)  kernel %.3f ms  wall %.3f ms"
                  "  passes per pixel %d..%d  path %d" % (
                      kind, es.passes_rendered, es.reached, es.rel_error, st.render_launches,
                      "" if ad is None else " (%d partial, %d of %d tiles active at the end)" % (ad.partial_rounds, ad.tiles_active, ad.tiles),
                      st.samples, uniform, 100.0 * st.samples / max(uniform, 1), st.render_kernel_ms, wall, es.passes_min, es.passes_max,
                      st.geometry_path), flush=True)
            pt.close()
        (_, eu, _, su, wu, _), (_, ea, _, sa, wa, _) = rows
        print("  adaptive / until: samples %.3f  kernel time %.3f  wall %.3f" % (
            sa.samples / max(su.samples, 1), sa.render_kernel_ms / su.render_kernel_ms, wa / wu), flush=True)


if __name__ == "__main__":
    main()
