"""Dev tool: what pt_resolve_filtered is worth on the bench configs, at the bench sizes (profiles/r13_filter.txt).

    python tools/filter_compare.py [--patch] [config2 config4 config5 default]

Per config: (1) a context renders the config's whole spp in 16-spp decorrelated passes at a clock of its own: THE CONVERGED
FRAME, linear radiance.  (2) A fresh context renders a quarter of that spp at the config's clock with the error estimate on
and reads out the estimate's own mean (radius 0) and the filtered frame at radius 1 to 4, kappa PT_FILTER_KAPPA_DEFAULT, all
linear.  Printed: the mean squared error of each against the converged frame over the pixels both hold finite, the ratio to
the unfiltered one, the mean accepted taps, the wall time of the read-out call (kernel, 16 B per pixel to the host, the
synchronise).  Both frames come from this process; the converged frame's own noise is in every figure alike.

--patch adds, under each radius from 1 on, the patch-wise read-out (pt_resolve_filtered_patch, profiles/r17_filter_patch.txt) of
the same state: patch 0 at kappa PT_FILTER_KAPPA_DEFAULT, which must give the line above bit for bit, and patch 1 at kappa
PT_FILTER_PATCH_KAPPA_DEFAULT.  Without the option the output is what it was."""
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
CONVERGED_CLOCK = 9000.5   # added to the config's clock: other random numbers than the frame under test


def rendered(sc, p, passes):
    """A context that has rendered `passes` passes of `p` with the estimate on."""
    per = max(1, min(8, passes // 2))
    pt = PathTracer(p.width, p.height)
    pt.set_spheres(sc.spheres)
    pt.set_params(p)
    pt.reserve_passes(per)
    pt.tune(per)
    pt.error_estimate(True)
    pt.reset()
    pt.set_params(p)
    es = pt.render_until(1e-30, per, passes)   # (a target that cannot be met: exactly `passes` passes)
    assert es.passes_rendered == passes
    return pt, es


def measured(read_out, converged):
    """(mse over the pixels both frames hold finite, those pixels, the frame, wall ms of the second call) of a read-out."""
    read_out()   # (warm: the first call loads nothing new, but pays the first pinned copy)
    t0 = time.perf_counter()
    out = read_out()
    wall = (time.perf_counter() - t0) * 1e3
    d = out[..., :3].astype(np.float64) - converged
    ok = np.isfinite(d).all(axis=-1)
    return float((d[ok] ** 2).sum() / (3 * max(int(ok.sum()), 1))), ok, out, wall


def main():
    args = sys.argv[1:]
    with_patch = "--patch" in args
    names = [a for a in args if a != "--patch"] or list(CONFIGS)
    for name in names:
        make, whole = CONFIGS[name]
        sc = make()
        p = sc.params.copy()
        p.time_step, p.first_pass = abi.PT_TIME_STEP_DECORRELATED, 0
        quarter = max(2, whole // 4)
        q = p.copy()
        q.time = p.time + CONVERGED_CLOCK
        pt, es = rendered(sc, q, whole)
        converged = pt.filtered_image(0, gamma=False)[..., :3].astype(np.float64)
        pt.close()
        print("%s: %dx%d, converged frame %d passes of 16 spp (rel_error %.5f); under test: %d passes" % (
            name, p.width, p.height, whole, es.rel_error, quarter), flush=True)
        pt, es = rendered(sc, p, quarter)
        base = None
        for radius in range(0, abi.PT_FILTER_MAX_RADIUS + 1):
            pt.filtered_image(radius, gamma=False)   # (warm: the first call loads nothing new, but pays the first pinned copy)
            t0 = time.perf_counter()
            out = pt.filtered_image(radius, abi.PT_FILTER_KAPPA_DEFAULT, gamma=False)
            wall = (time.perf_counter() - t0) * 1e3
            d = out[..., :3].astype(np.float64) - converged
            ok = np.isfinite(d).all(axis=-1)
            mse = float((d[ok] ** 2).sum() / (3 * max(int(ok.sum()), 1)))
            base = mse if radius == 0 else base
            print("  radius %d kappa %g: mse %.6g  filtered / unfiltered %.3f  mean taps %.2f  pixels compared %d of %d  call %.3f ms%s" % (
                radius, abi.PT_FILTER_KAPPA_DEFAULT, mse, mse / base if base > 0 else float("nan"), float(out[..., 3].mean()),
                int(ok.sum()), ok.size, wall, "  (rel_error %.5f)" % es.rel_error if radius == 0 else ""), flush=True)
            if with_patch and radius > 0:
                for patch, kappa in ((0, abi.PT_FILTER_KAPPA_DEFAULT), (1, abi.PT_FILTER_PATCH_KAPPA_DEFAULT)):
                    pmse, pok, pout, pwall = measured(lambda: pt.patch_filtered_image(radius, patch, kappa, gamma=False), converged)
                    same = "" if patch else ("  same bits as the line above" if pout.tobytes() == out.tobytes() else "  BITS DIFFER from the line above")
                    print("  radius %d patch %d kappa %g: mse %.6g  filtered / unfiltered %.3f  mean taps %.2f  pixels compared %d of %d  call %.3f ms%s" % (
                        radius, patch, kappa, pmse, pmse / base if base > 0 else float("nan"), float(pout[..., 3].mean()),
                        int(pok.sum()), pok.size, pwall, same), flush=True)
        pt.close()


if __name__ == "__main__":
    main()
