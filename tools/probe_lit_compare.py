#!/usr/bin/env python3
"""probe_lit_compare.py — what a probe-lit frame costs and what it is worth (pt_bake_lattice, pt_shade_probes).

    python3 tools/probe_lit_compare.py [--out profiles/r33_probe_lit.txt] [--size 1920x1080] [--skip-quality]
    python3 tools/probe_lit_compare.py --kernels-only          section 1 alone: what a run under rocprofv3 --kernel-trace executes
    python3 tools/probe_lit_compare.py --trace DIR [--out F]   the kernel times of such a run from its trace, appended to F

Runs on one MI355X and writes three sections; the fourth, 1b, comes from a kernel trace of a run of its own:

  1. CALL TIME at the frame size: pt_shade_probes with the records and the frame on the device (the call is then its one kernel
     and its launch), lattices of 8^3, 32^3 and 64^3 over config 2 and config 4, BOTH kernel forms (include/ptrace_dev.h
     pt_debug_probe_form: 0 every lane loads its corners, 1 a coherent wave stages its cell in LDS), alternating, device events
     around `--reps` calls after a warm-up, the median of five such windows; with form 1 the share of waves that took the staged way.
 1b. THE KERNELS beside THE TRAFFIC FLOOR, case by case, from the trace: four planes in and one out is 80 bytes a pixel, the
     lattice (112 bytes a node) once, at pt_tone_kernel's OWN rate over the same texels (32 bytes a texel over the kernel's time in
     the trace: device memory only — a pt_resolve_toned call also copies the frame to the caller and is no yardstick).  The ratio
     is reported, not asserted.
  2. THE HOST WAY on the same frame: the four planes read out, the cell look-up and the eight-record blend in numpy (float32
     weights, abi.sh_irradiance in float64 for the DIFFUSE pixels; METAL and GLASS get the DIFFUSE treatment: a lower bound of the
     host's work), the picture uploaded again; a host clock, once.
  3. QUALITY on config 4 at 256 x 256: the probe-lit frame (lattice 8 x 8 x 10, D = 256, both estimators) against a converged
     path-traced frame (next-event estimation, 4 096 samples a pixel: the same expectation), squared error over the DIFFUSE
     first-hit pixels, beside the 1-, 4- and 16-pass path-traced frames (one sample a pass, plain estimator) and the times of all
     of them, the bake's included.  A record of what the approximation is worth; no test asserts it."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402  (before the package: one HIP runtime in the process)

from ray_tracer_webgl_amd import abi, scenes  # noqa: E402
from ray_tracer_webgl_amd.tracer import PathTracer  # noqa: E402

LINES = []
SCENES = (("config2", scenes.config2), ("config4", scenes.config4))
LATTICES = ((8, 8, 8), (32, 32, 32), (64, 64, 64))
TONE_CALLS = 100


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def scene_lattice(spheres, n):
    """the lattice of n = (nx, ny, nz) nodes over the bounding box of the spheres whose radius is below 100 (render.py's rule)"""
    from ray_tracer_webgl_amd.render import lattice_over

    return lattice_over(spheres, n)


def synthetic(nodes, seed=5):
    rng = np.random.default_rng(seed)
    r = rng.uniform(-0.3, 0.6, (nodes, 28)).astype(np.float32)
    r[:, 0:3] += np.float32(1.5)
    r[:, 27] = 256.0
    return r


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def kernel_times(w, h, reps):
    say("1. CALL TIME, %d x %d, device records and device frame; microseconds per call, median of five windows of %d calls "
        "(device events), the forms alternating window by window" % (w, h, reps))
    say("   %-8s %-10s %9s %9s %9s %8s" % ("scene", "lattice", "form 0", "form 1", "f1 / f0", "staged"))
    for name, make in SCENES:
        sc = make(w, h, 1, 1, 8)
        t = PathTracer(w, h, use_torch=True)
        t.set_spheres(sc.spheres)
        t.feature_planes(True)
        t.tone_mapping(True)
        t.set_params(sc.params)
        t.render_features()
        set_form = t.lib.pt_debug_probe_form
        frame = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        tiles = ((w + 7) // 8) * ((h + 7) // 8)
        paths = torch.zeros(tiles, dtype=torch.int32, device="cuda")
        # the yardstick's launches, for the kernel trace of a --kernels-only run: TONE_CALLS per scene
        tone = abi.PtToneOptions(abi.PT_TONE_FILMIC, 1, 1.0, 1.0)
        src = torch.rand((h, w, 4), dtype=torch.float32, device="cuda")
        for _ in range(TONE_CALLS):
            t.toned_image(tone, src)
        torch.cuda.synchronize()
        for dims in LATTICES:
            lat = scene_lattice(sc.spheres, dims)
            probes = torch.from_numpy(synthetic(lat.nodes)).cuda()
            opt = abi.PtProbeShadeOptions()
            call = lambda: t._check(t.lib.pt_shade_probes(t._ctx, C.byref(lat), C.c_void_p(probes.data_ptr()), C.byref(opt), C.c_void_p(frame.data_ptr())))
            out, ms = {}, {0: [], 1: []}
            for form in (0, 1):
                t._check(set_form(t._ctx, form, C.c_void_p(paths.data_ptr()) if form else None))
                call()
                torch.cuda.synchronize()
                out[form] = frame.clone()
            assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32)), "the two forms differ"
            staged = float((paths == 2).sum()) / max(float((paths > 0).sum()), 1.0)
            for _ in range(5):
                for form in (0, 1):
                    t._check(set_form(t._ctx, form, None))
                    call()
                    ms[form].append(window_ms(call, reps))
            t._check(set_form(t._ctx, -1, None))
            m0, m1 = float(np.median(ms[0])), float(np.median(ms[1]))
            say("   %-8s %-10s %9.1f %9.1f %9.2f %7.0f%%" % (name, "%dx%dx%d" % dims, m0 * 1e3, m1 * 1e3, m1 / m0, 100.0 * staged))
        t.close()


def host_way(w, h):
    say()
    say("2. THE HOST WAY, %d x %d, config 4, lattice 32^3: host clocks, ms, once" % (w, h))
    sc = scenes.config4(w, h, 1, 1, 8)
    t = PathTracer(w, h)
    t.set_spheres(sc.spheres)
    t.feature_planes(True)
    t.set_params(sc.params)
    t.render_features()
    t.synchronize()
    lat = scene_lattice(sc.spheres, (32, 32, 32))
    probes = synthetic(lat.nodes)
    t.probe_lit_image(lat, probes)
    t0 = time.perf_counter()
    call = t.probe_lit_image(lat, probes)
    t_call = time.perf_counter() - t0
    t0 = time.perf_counter()
    f = t.features()
    t_read = time.perf_counter() - t0
    t0 = time.perf_counter()
    hp, n, al = f["point"][..., :3].reshape(-1, 3), f["normal"][..., :3].reshape(-1, 3), f["albedo"][..., :3].reshape(-1, 3)
    dims = np.array([lat.nx, lat.ny, lat.nz])
    g = (hp - np.array(list(lat.origin), np.float32)) / np.array(list(lat.step), np.float32)
    i = np.clip(np.floor(g).astype(np.int64), 0, dims - 2)
    fr = np.clip(g - i, 0.0, 1.0).astype(np.float32)
    pos = abi.probe_lattice_positions(lat)
    S, W = np.zeros((len(hp), 3)), np.zeros(len(hp))
    for corner in range(8):
        b = np.array([(corner >> c) & 1 for c in range(3)])
        wgt = np.prod(np.where(b[None, :] == 1, fr, 1.0 - fr), axis=1)
        node = ((i[:, 2] + b[2]) * dims[1] + (i[:, 1] + b[1])) * dims[0] + (i[:, 0] + b[0])
        keep = (wgt > 0) & (probes[node, 27] > 0) & (np.einsum("pc,pc->p", pos[node] - hp, n) > 0)
        E = abi.sh_irradiance(probes[node, :27].reshape(-1, 9, 3), n)
        S += np.where(keep[:, None], wgt[:, None] * E, 0.0)
        W += np.where(keep, wgt, 0.0)
    img = np.zeros((h * w, 4), np.float32)
    ok = W > 0
    img[ok, :3] = (al[ok] * np.maximum(S[ok] / W[ok, None], 0.0) / np.pi).astype(np.float32)
    img[ok, 3] = 1.0
    t_numpy = time.perf_counter() - t0
    t0 = time.perf_counter()
    dev = torch.from_numpy(img.reshape(h, w, 4)).cuda()
    torch.cuda.synchronize()
    t_up = time.perf_counter() - t0
    d = (f["ids"][..., 0].reshape(-1) >= 0) & (f["ids"][..., 2].reshape(-1) == abi.PT_DIFFUSE)
    diff = np.abs(call.reshape(-1, 4)[d, :3] - img[d, :3]).max()
    say("   pt_shade_probes, host records in, host frame out (staging and both copies included)   %9.2f" % (t_call * 1e3))
    say("   the host way: planes read out %.2f + numpy look-up, blend and abi.sh_irradiance %.2f + upload %.2f = %9.2f" % (
        t_read * 1e3, t_numpy * 1e3, t_up * 1e3, (t_read + t_numpy + t_up) * 1e3))
    say("   (the two pictures agree on the DIFFUSE pixels to %.2g: float64 against the call's fp32)" % diff)
    del dev
    t.close()


def quality():
    say()
    w = h = 256
    say("3. QUALITY, config 4 at %d x %d: mean squared error over the DIFFUSE first-hit pixels against a converged frame (next-event, 4 096 spp); host clocks, ms" % (w, h))
    sc = scenes.config4(w, h, 1, 1, 50)
    p = sc.params.copy()
    p.time_step = abi.PT_TIME_STEP_DECORRELATED

    def tracer(spp, nee):
        t = PathTracer(w, h)
        t.set_spheres(sc.spheres)
        t.feature_planes(True)
        t.ray_queries(True)
        if nee:
            t.next_event(True)
        q = p.copy()
        q.samples_per_pixel = spp
        t.reserve_passes(16)
        t.set_params(q)
        return t, q

    t, q = tracer(64, True)
    for k in range(4):
        q.first_pass = 16 * k
        t.set_params(q)
        t.render_passes(16)
    acc = t.accum()
    ref = acc[..., :3] / acc[..., 3:4]
    t.render_features()
    f = t.features()
    d = (f["ids"][..., 0] >= 0) & (f["ids"][..., 2] == abi.PT_DIFFUSE)
    say("   %d DIFFUSE first-hit pixels of %d; the reference's mean over them %.4f" % (d.sum(), w * h, float(ref[d].mean())))
    mse = lambda img: float(((img[d][:, :3].astype(np.float64) - ref[d]) ** 2).mean())
    lat = scene_lattice(sc.spheres, (8, 8, 10))
    q.samples_per_pixel, q.first_pass = 1, 0
    t.set_params(q)
    for nee in (False, True):
        t.bake_lattice(lat, directions=64, next_event=nee)  # (warm-up: the code objects)
        t0 = time.perf_counter()
        rec = t.bake_lattice(lat, directions=256, passes=1, next_event=nee)
        t_bake = time.perf_counter() - t0
        t.render_features()
        t.synchronize()
        t0 = time.perf_counter()
        t.render_features()
        img = t.probe_lit_image(lat, rec)
        t_frame = time.perf_counter() - t0
        alpha0 = int((img[d][:, 3] == 0).sum())
        say("   probe-lit, lattice 8x8x10, D = 256, %-10s  mse %10.5f   bake %8.2f ms (once per scene), frame (features + shading, host records) %6.2f ms; %d pixels without a usable probe"
            % ("next-event" if nee else "plain", mse(img), t_bake * 1e3, t_frame * 1e3, alpha0))
        err = ((img[..., :3].astype(np.float64) - ref) ** 2).sum(axis=2) * d
        ys, xs = np.unravel_index(np.argsort(err.ravel())[-200:], err.shape)
        say("      the 200 worst pixels: rows %d .. %d (median %d), columns %d .. %d (median %d) of %d (row 0 the bottom)"
            % (ys.min(), ys.max(), int(np.median(ys)), xs.min(), xs.max(), int(np.median(xs)), h))
    t.close()
    for passes in (1, 4, 16):
        u, uq = tracer(1, False)
        u.render_passes(1)
        u.synchronize()
        u.reset()
        uq.first_pass = 0
        u.set_params(uq)
        t0 = time.perf_counter()
        u.render_passes(passes)
        u.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        a = u.accum()
        say("   path-traced, plain, %2d pass(es) of 1 sample                 mse %10.5f   %8.2f ms" % (passes, mse(a[..., :3] / a[..., 3:4]), ms))
        u.close()


def trace_summary(path, w, h, reps, out):
    """Section 1b from the kernel trace of a `--kernels-only --reps R` run.  The run's launches come in a known order: per scene
    TONE_CALLS of pt_tone_kernel, then per lattice 1 + 5 (1 + R) launches of each shading kernel; the trace's rows of a kernel,
    sorted by their start, are split into the cases by those counts."""
    import csv
    import glob

    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit("no *kernel_trace.csv under %s" % path)
    groups = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0].replace(".kd", "")
            if name.startswith("pt_probe_shade") or name == "pt_tone_kernel":
                groups.setdefault(name, []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    per_case = 1 + 5 * (1 + reps)
    cases = len(SCENES) * len(LATTICES)
    want = {"pt_tone_kernel": len(SCENES) * TONE_CALLS, "pt_probe_shade_kernel": cases * per_case, "pt_probe_shade_shared_kernel": cases * per_case}
    for name, n in want.items():
        if len(groups.get(name, ())) != n:
            sys.exit("%s: %d launches in the trace, %d expected of a --kernels-only --reps %d run" % (name, len(groups.get(name, ())), n, reps))
    us = {name: [d for _, d in sorted(v)] for name, v in groups.items()}
    say()
    say("1b. THE KERNELS beside THE TRAFFIC FLOOR, %d x %d, from rocprofv3 --kernel-trace over `--kernels-only --reps %d` (a run of its own): "
        "median microseconds of a case's launches; floor = (80 bytes a pixel + 112 bytes a node) at pt_tone_kernel's rate on the same scene's run "
        "(32 bytes a texel over its median time in the trace)" % (w, h, reps))
    say("   %-8s %-10s %9s %9s %9s %9s %9s %10s %10s" % ("scene", "lattice", "tone us", "tone GB/s", "floor us", "form 0", "form 1", "f0 / floor", "f1 / floor"))
    from ray_tracer_webgl_amd.render import lattice_over

    for si, (name, make) in enumerate(SCENES):
        tone_us = float(np.median(us["pt_tone_kernel"][si * TONE_CALLS:(si + 1) * TONE_CALLS]))
        rate = 32.0 * w * h / (tone_us * 1e-6) / 1e9
        spheres = make(w, h, 1, 1, 8).spheres
        for li, dims in enumerate(LATTICES):
            k = si * len(LATTICES) + li
            nodes = lattice_over(spheres, dims).nodes
            floor_us = (80.0 * w * h + 112.0 * nodes) / (rate * 1e9) * 1e6
            m0 = float(np.median(us["pt_probe_shade_kernel"][k * per_case:(k + 1) * per_case]))
            m1 = float(np.median(us["pt_probe_shade_shared_kernel"][k * per_case:(k + 1) * per_case]))
            say("   %-8s %-10s %9.1f %9.0f %9.1f %9.1f %9.1f %10.2f %10.2f" % (name, "%dx%dx%d" % dims, tone_us, rate, floor_us, m0, m1, m0 / floor_us, m1 / floor_us))
    with open(out, "a") as fh:
        fh.write("\n".join(LINES) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r33_probe_lit.txt")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--trace", metavar="DIR")
    args = ap.parse_args()
    w, h = (int(x) for x in args.size.split("x"))
    if args.trace:
        return trace_summary(args.trace, w, h, args.reps, args.out)
    if not torch.cuda.is_available():
        sys.exit("probe_lit_compare.py measures on a GPU and found none")
    say("tools/probe_lit_compare.py on %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    kernel_times(w, h, args.reps)
    if args.kernels_only:
        return
    host_way(w, h)
    if not args.skip_quality:
        quality()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
