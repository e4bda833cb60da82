"""Dev tool: what pt_filter_patch_kernel costs beside pt_filter_kernel (profiles/r17_filter_patch.txt).

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/filter_patch_time.py     (the kernel times)
    python tools/filter_patch_time.py --trace DIR                                                 (... read back, in call order)
    python tools/filter_patch_time.py                                                             (the wall times of the calls)

The state: config 2's scene at 1920x1080, 8 passes of 16 spp, decorrelated step, every pixel counted.  The calls, three each, in
this order: for radius 1 to 4 pt_resolve_filtered(radius, kappa 2) and pt_resolve_filtered_patch(radius, patch 1, kappa 1.5);
then pt_resolve_filtered_patch(radius 2, patch 0, kappa 2).  All with gamma, into a host array.  Without the profiler the tool
prints the wall time of each call (kernel, 33 MB to the host, the synchronise) and the mean accepted taps."""
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEAT = 3
# (label, radius, patch or None for pt_resolve_filtered, kappa)
CALLS = [c for radius in (1, 2, 3, 4) for c in (("radius %d pixel test" % radius, radius, None, 2.0),
                                                ("radius %d patch 1" % radius, radius, 1, 1.5))] + [("radius 2 patch 0", 2, 0, 2.0)]


def read_trace(directory):
    rows = []
    for f in glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if r["Kernel_Name"].startswith("pt_filter")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == REPEAT * len(CALLS), (len(rows), REPEAT * len(CALLS))
    for i, (label, radius, patch, kappa) in enumerate(CALLS):
        mine = rows[REPEAT * i:REPEAT * (i + 1)]
        name = "pt_filter_kernel" if patch is None else "pt_filter_patch_kernel"
        assert all(r["Kernel_Name"].split("(")[0].split(".")[0] == name for r in mine), (label, [r["Kernel_Name"] for r in mine])
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine]
        print("%-22s %-24s kappa %-4g us: %s" % (label, name, kappa, " ".join("%.1f" % u for u in us)))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--trace":
        return read_trace(sys.argv[2])
    from ray_tracer_webgl_amd import abi, scenes
    from ray_tracer_webgl_amd.tracer import PathTracer

    sc = scenes.config2(1920, 1080, 16, 8, 50)
    p = sc.params.copy()
    p.time_step, p.first_pass = abi.PT_TIME_STEP_DECORRELATED, 0
    pt = PathTracer(p.width, p.height)
    pt.set_spheres(sc.spheres)
    pt.set_params(p)
    pt.reserve_passes(8)
    pt.error_estimate(True)
    pt.render_passes(8)
    state = pt.error_state()
    assert np.all(state[..., 0, 3] == 8.0)
    for label, radius, patch, kappa in CALLS:
        walls = []
        for _ in range(REPEAT):
            t0 = time.perf_counter()
            out = pt.filtered_image(radius, kappa) if patch is None else pt.patch_filtered_image(radius, patch, kappa)
            walls.append((time.perf_counter() - t0) * 1e3)
        print("%-22s kappa %-4g wall ms: %s  mean taps %.2f" % (label, kappa, " ".join("%.3f" % w for w in walls), float(out[..., 3].mean())),
              flush=True)
    pt.close()


if __name__ == "__main__":
    main()
