"""What next-event estimation (PT_OPT_NEXT_EVENT) buys and costs on BASELINE config 4, measured on one device: writes
profiles/r30_next_event.txt.

Two scenes at the bench's size (1024 x 1024, depth 50): config 4 as it is, and config 4 with its light at a quarter of the
radius.  For each: a PLAIN reference frame of at least 64 times the samples of the frames under test, then — over REPEATS
disjoint runs of passes, after one warm-up launch each way — the mean squared error (linear radiance, all pixels and channels)
of the plain frame and of the next-event frame at EQUAL SAMPLES, and of the plain frame at EQUAL KERNEL TIME (as many passes as
fit into the next-event frame's kernel time; the figure is interpolated between the two neighbouring pass counts).  Times are
the trace kernel's HIP-event times (PtStats.render_kernel_ms), medians of the repeats.  The shadow segments' share of all
segments comes from the two segment counts.  The twelve builds' registers, scratch and waves are read from a cross-compile's
resource report (tools/kernel_resources.sh) when --resources names its table.

    python tools/next_event_compare.py [--size 1024] [--spp 8] [--passes 8] [--repeats 5] [--resources FILE] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ray_tracer_webgl_amd import abi, scenes  # noqa: E402
from ray_tracer_webgl_amd.tracer import PathTracer  # noqa: E402


def context(sc, p, next_event, reserve):
    t = PathTracer(p.width, p.height)
    t.set_spheres(sc.spheres)
    t.next_event(next_event)
    t.set_params(p)
    t.reserve_passes(reserve)
    return t


def run(t, p, first_pass, n_passes, per_launch):
    """(mean radiance frame, kernel ms, segments) of n_passes passes starting at first_pass"""
    t.reset()
    done = 0
    while done < n_passes:
        q = p.copy()
        q.first_pass = first_pass + done
        t.set_params(q)
        k = min(per_launch, n_passes - done)
        t.render_passes(k)
        done += k
    st = t.stats()
    acc = t.accum().astype(np.float64)
    return acc[..., :3] / np.maximum(acc[..., 3:4], 1.0), st.render_kernel_ms, st.segments


def mse(a, b):
    return float(np.mean((a - b) ** 2))


def measure(name, sc, args, out):
    p = sc.params.copy()
    p.samples_per_pixel = args.spp
    p.time_step = abi.PT_TIME_STEP_DECORRELATED
    n = args.passes
    ref_passes = 64 * n
    reserve = max(16, 8 * n)  # (room for the equal-time frame's launch: the next-event kernel costs a few times the plain one)
    plain = context(sc, p, False, reserve)
    nee = context(sc, p, True, reserve)
    try:
        # the reference: plain, passes far from the ones under test
        ref, ref_ms, _ = run(plain, p, 1 << 20, ref_passes, 16)
        rows = []
        for r in range(args.repeats + 1):  # (repeat 0 is the warm-up: first launches, PT_GEOM_AUTO's trials)
            first = r * 4 * n
            f_nee, ms_nee, seg_nee = run(nee, p, first, n, n)
            f_plain, ms_plain, seg_plain = run(plain, p, first, n, n)
            # equal kernel time: the plain frame of n_eq passes, n_eq = n * ms_nee / ms_plain (interpolated)
            n_eq = n * ms_nee / ms_plain
            lo = min(max(1, int(np.floor(n_eq))), reserve - 1)
            f_lo, ms_lo, _ = run(plain, p, first, lo, lo)
            f_hi, ms_hi, _ = run(plain, p, first, lo + 1, lo + 1)
            e_lo, e_hi = mse(f_lo, ref), mse(f_hi, ref)
            w = min(max(n_eq - lo, 0.0), 1.0)
            if r:
                rows.append((mse(f_plain, ref), mse(f_nee, ref), e_lo * (1 - w) + e_hi * w, ms_plain, ms_nee, seg_plain, seg_nee, n_eq))
        m = np.median(np.asarray(rows), axis=0)
        shadow_share = (m[6] - m[5]) / m[6]
        out.append("%s: %d spheres, %d x %d, %d passes of %d samples, depth %d; reference: plain, %d samples (%d x), %.1f ms of kernel" % (
            name, len(sc.spheres), p.width, p.height, n, args.spp, p.max_depth, ref_passes * args.spp, ref_passes // n, ref_ms))
        out.append("  kernel time (median of %d): plain %.3f ms, next-event %.3f ms (x %.2f)" % (args.repeats, m[3], m[4], m[4] / m[3]))
        out.append("  segments: plain %d, next-event %d; shadow segments' share of all segments %.3f (difference of the counts: the paths' own"
                   " segments change too where emission is skipped)" % (m[5], m[6], shadow_share))
        out.append("  squared error against the reference, equal samples: plain %.4e, next-event %.4e (plain / next-event %.2f)" % (m[0], m[1], m[0] / m[1]))
        out.append("  squared error, equal kernel time (plain with %.2f passes): plain %.4e, next-event %.4e (plain / next-event %.2f)%s" % (
            m[7], m[2], m[1], m[2] / m[1], "" if m[2] > m[1] else "  <- WORSE at equal time here"))
        out.append("  (the reference's own error is about 1/%d of the plain frame's: %.1e)" % (ref_passes // n, m[0] * n / ref_passes))
    finally:
        plain.close()
        nee.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--resources", help="the table tools/kernel_resources.sh printed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_next_event.txt"))
    args = ap.parse_args()
    out = ["Next-event estimation (PT_OPT_NEXT_EVENT) against the plain estimator on BASELINE config 4 (tools/next_event_compare.py), one MI355X.",
           "Device-event kernel times after a warm-up, medians of %d repeats over disjoint passes; errors in linear radiance, mean over pixels and channels." % args.repeats,
           ""]
    room = scenes.config4(args.size, args.size, args.spp, args.passes, 50)
    measure("config 4", room, args, out)
    out.append("")
    small = scenes.config4(args.size, args.size, args.spp, args.passes, 50)
    light = int(np.flatnonzero(small.spheres["type"] == abi.PT_EMISSIVE)[0])
    small.spheres[light]["radius"] = np.float32(float(small.spheres[light]["radius"]) / 4.0)
    measure("config 4, the light at a quarter of its radius (%g)" % float(small.spheres[light]["radius"]), small, args, out)
    if args.resources and os.path.exists(args.resources):
        out += ["", "The twelve next-event builds beside their namesakes (cross-compile's resource report, tools/kernel_resources.sh):"]
        lines = open(args.resources).read().splitlines()
        names = [ln.split()[0][:-4] for ln in lines if ln.split() and ln.split()[0].endswith("_nee")]
        out += [ln for ln in lines if ln.startswith("kernel") or (ln.split() and (ln.split()[0].endswith("_nee") or ln.split()[0] in names))]
    text = "\n".join(out) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
