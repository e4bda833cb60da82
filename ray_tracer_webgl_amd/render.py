"""Command-line renderer: one of the BASELINE scenes -> PNG (the reference's "Save Image" path,
src/dom.rs:126-143, without a browser).

    python -m ray_tracer_webgl_amd.render --config config2 --width 1920 --height 1080 --out cover.png
    python -m ray_tracer_webgl_amd.render --config default --debug-overlay --out overlay.png
    python -m ray_tracer_webgl_amd.render --config config2 --noise-target 0.02 --max-spp 4096 --error-out cover_error.png
    python -m ray_tracer_webgl_amd.render --config config2 --noise-target 0.02 --adaptive --samples-out cover_samples.png
    python -m ray_tracer_webgl_amd.render --config config2 --noise-target 0.05 --denoise --out cover_filtered.png
    python -m ray_tracer_webgl_amd.render --config config2 --noise-target 0.05 --denoise-patch --out cover_patch_filtered.png
    python -m ray_tracer_webgl_amd.render --config config4 --probe-lit 8,8,10 --next-event --tone filmic --out room_probe_lit.png
"""
import argparse
import math
import time

import numpy as np

from . import image_io, scenes
from . import abi
from .tracer import PathTracer, render_scene


def glare_options(strength, levels, threshold):
    """abi.PtGlareOptions of --glare / --glare-levels / --glare-threshold, or None when a value is out of range.  With fewer (or
    more) levels than the default's six, the default weights of the levels in use are rescaled to add up to 1 (levels 7 and 8
    take the last default weight before the rescaling)."""
    if not (0.0 <= strength <= 1.0) or not (1 <= levels <= abi.PT_GLARE_MAX_LEVELS) or not (0.0 <= threshold < float("inf")):
        return None
    base = list(abi.PT_GLARE_WEIGHTS_DEFAULT[:abi.PT_GLARE_LEVELS_DEFAULT])
    base += [base[-1]] * (abi.PT_GLARE_MAX_LEVELS - len(base))
    used = base[:levels]
    total = sum(used)
    return abi.PtGlareOptions(strength, threshold, levels, [w / total for w in used])


def lattice_over(spheres, n, flags=0):
    """abi.PtProbeLattice of n = (nx, ny, nz) nodes over the bounding box of the spheres whose radius is below 100 (the walls and
    the ground of the BASELINE scenes are spheres of radius 100 and more: they are what the lattice stands IN, not what it spans)."""
    small = [s for s in spheres if abs(float(s["radius"])) < 100.0]
    if not small:
        raise ValueError("no sphere of a radius below 100 to span a lattice over")
    lo = np.min([np.asarray(s["center"], np.float64) - abs(float(s["radius"])) for s in small], axis=0)
    hi = np.max([np.asarray(s["center"], np.float64) + abs(float(s["radius"])) for s in small], axis=0)
    step = np.maximum((hi - lo) / (np.asarray(n, np.float64) - 1.0), 1e-6)
    return abi.PtProbeLattice(origin=tuple(lo), step=tuple(step), n=tuple(int(v) for v in n), flags=flags)


def probe_lit(sc, args, geom, lattice_n, curve, exposure, glare):
    """--probe-lit: bake a lattice over the scene once, shade the camera's first hits from it (pt_bake_lattice, pt_shade_probes)
    and take the linear frame through the read-outs --tone / --glare name (without --tone: the square root and the clamp)."""
    p = sc.params.copy()
    p.time_step = abi.PT_TIME_STEP_DECORRELATED
    p.samples_per_pixel = 1
    pt = PathTracer(p.width, p.height, device=args.device)
    pt.set_geometry_path(geom)
    pt.set_spheres(sc.spheres)
    pt.feature_planes(True)
    pt.ray_queries(True)
    if args.next_event:
        pt.next_event(True)
    pt.set_params(p)
    lat = lattice_over(sc.spheres, lattice_n, abi.PT_LATTICE_SKIP_BURIED)
    t0 = time.perf_counter()
    rec = pt.bake_lattice(lat, directions=args.probe_directions, passes=1, next_event=args.next_event)
    t_bake = time.perf_counter() - t0
    t0 = time.perf_counter()
    pt.render_features()
    frame = pt.probe_lit_image(lat, rec)
    t_frame = time.perf_counter() - t0
    empty = int((frame[..., 3] == 0).sum())
    frame[..., 3] = 1.0  # (alpha 0 marked the pixels without a usable probe: they stay black)
    print("probe-lit: lattice %dx%dx%d from (%.3g, %.3g, %.3g) in steps of (%.3g, %.3g, %.3g), %d of %d nodes buried, %d directions, %s estimator: "
          "bake %.1f ms, frame (features + shading) %.2f ms, %d pixels without a usable probe" % (
              lat.nx, lat.ny, lat.nz, *lat.origin, *lat.step, int((rec["samples"] == 0).sum()), lat.nodes, args.probe_directions,
              "next-event" if args.next_event else "plain", t_bake * 1e3, t_frame * 1e3, empty))
    if curve is None:
        frame[..., :3] = np.sqrt(np.clip(frame[..., :3], 0.0, 1.0))
    else:
        pt.tone_mapping(True)
        if glare is not None:
            pt.glare(True)
            frame = pt.glared_image(src=frame, options=glare)
        pt.meter(abi.PtMeterOptions(), src=frame)
        rec_e, _ = pt.exposure()
        opt = abi.PtToneOptions(curve, 1, 0.0, 1.0)
        if exposure is not None:
            opt = abi.PtToneOptions(curve, 1, exposure, max(rec_e.y_high * exposure, 1.0))
        frame = pt.toned_image(opt, src=frame)
    image_io.write_png(args.out, frame)
    print("%s: %dx%d, %d spheres, probe-lit -> %s" % (sc.name, p.width, p.height, len(sc.spheres), args.out))
    pt.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", default="config2", choices=sorted(scenes.CONFIGS))
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--spp-per-pass", type=int)
    ap.add_argument("--passes", type=int)
    ap.add_argument("--max-depth", type=int)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--geometry", default="auto", choices=["auto", "lds", "scalar", "bvh", "grid", "small"],
                    help="how the kernel looks at the sphere list (same image bits on every path; auto: the library measures "
                         "the usable ones — the grid walk on scenes of hundreds of spheres, the small-list kernels up to 16)")
    ap.add_argument("--debug-overlay", action="store_true",
                    help="the shader's debug view of the default scene (static/shader.frag:307-318): the sphere under the "
                         "crosshair outlined in red, the point the crosshair hits a blue dot (--config default only)")
    ap.add_argument("--noise-target", type=float, metavar="X",
                    help="render until the frame's relative error (PtErrorStats.rel_error: the root of the summed squared standard "
                         "errors over the summed squared means) is at most X, instead of a fixed number of passes; prints spp "
                         "rendered, rel_error and reached.  Passes get the decorrelated time step: the estimate assumes independent passes")
    ap.add_argument("--max-spp", type=int, metavar="N", help="with --noise-target: stop after N samples per pixel (default: the config's spp)")
    ap.add_argument("--adaptive", action="store_true",
                    help="with --noise-target: after every look trace only the 8x8 tiles that still miss their share of the target "
                         "(pt_render_adaptive); prints rounds, partial rounds and the share of the uniform samples traced")
    ap.add_argument("--error-out", metavar="FILE", help="also write the per-pixel standard error (linear radiance, shown x 8) as an image")
    ap.add_argument("--samples-out", metavar="FILE",
                    help="also write the per-pixel sample counts (white = the frame's largest count) as an image")
    ap.add_argument("--denoise", nargs="?", const="2", metavar="R[,KAPPA]",
                    help="with --noise-target or --error-out: write the main image from the variance-guided filtered read-out "
                         "(pt_resolve_filtered: a pixel is averaged with the neighbours within R whose means differ by no more than "
                         "KAPPA standard errors; default 2,%g; R at most %d); prints the mean accepted taps"
                         % (abi.PT_FILTER_KAPPA_DEFAULT, abi.PT_FILTER_MAX_RADIUS))
    ap.add_argument("--denoise-patch", nargs="?", const="2", metavar="R[,KAPPA]",
                    help="like --denoise, with the patch-wise test (pt_resolve_filtered_patch: a neighbour is averaged in when the "
                         "3x3 neighbourhoods around the two pixels differ by no more than KAPPA standard errors; default 2,%g); "
                         "not together with --denoise" % abi.PT_FILTER_PATCH_KAPPA_DEFAULT)
    ap.add_argument("--features", metavar="PREFIX",
                    help="also write the first-hit feature planes of the frame's camera (pt_render_features: one pinhole ray per "
                         "pixel) as PREFIX_albedo.npy, PREFIX_normal.npy, PREFIX_point.npy (float32) and PREFIX_ids.npy (int32: list "
                         "index, uuid, type, front_face), each (rows, width, 4), row 0 = the image's lowest row")
    ap.add_argument("--tone", choices=["clamp", "reinhard", "filmic"],
                    help="read the frame out through a tone curve (pt_resolve_toned) instead of the reference's sqrt-and-clamp: for "
                         "frames with more range than a display (config4's light).  Composes with --denoise / --denoise-patch: the "
                         "filtered linear frame is what is metered and toned")
    ap.add_argument("--exposure", default="auto", metavar="auto|VALUE",
                    help="with --tone: auto meters the frame on the device (pt_meter: the median lit pixel is exposed to 0.18) and "
                         "reads out with that record; VALUE multiplies the radiance by VALUE (Reinhard's white is then the "
                         "metered 99th percentile exposed by VALUE, at least 1).  Default auto")
    ap.add_argument("--glare", type=float, metavar="STRENGTH",
                    help="with --tone: spread this share (0 .. 1; the header's default is 0.15) of the frame's light over a bloom "
                         "pyramid before metering and toning (pt_glare): the veil that tells a light from a white wall once both are at "
                         "byte 255.  Energy-conserving; composes with --denoise / --denoise-patch")
    ap.add_argument("--glare-levels", type=int, default=abi.PT_GLARE_LEVELS_DEFAULT, metavar="N",
                    help="with --glare: pyramid levels in use, 1 .. %d (default %d); the default weights of the levels in use are "
                         "rescaled to add up to 1" % (abi.PT_GLARE_MAX_LEVELS, abi.PT_GLARE_LEVELS_DEFAULT))
    ap.add_argument("--glare-threshold", type=float, default=0.0, metavar="T",
                    help="with --glare: only the luminance above T spills (default 0: every pixel, whole)")
    ap.add_argument("--next-event", action="store_true",
                    help="next-event estimation (PT_OPT_NEXT_EVENT): sample the scene's emissive spheres at every diffuse hit; the same "
                         "expectation as the plain estimator with far less noise where a lamp is small (config4); not with --debug-overlay")
    ap.add_argument("--probe-lit", metavar="NX,NY,NZ",
                    help="instead of path tracing the frame: bake an SH probe lattice of NX x NY x NZ nodes (each 2 .. 256) over the "
                         "bounding box of the spheres whose radius is below 100 (pt_bake_lattice; nodes inside a sphere are skipped) and "
                         "shade the camera's first hits from it (pt_render_features, pt_shade_probes): a noise-free picture of the "
                         "diffuse light transport.  With --next-event the bake uses that estimator; --tone, --exposure and --glare "
                         "read the linear frame out as they read a path-traced one")
    ap.add_argument("--probe-directions", type=int, default=256, metavar="D",
                    help="with --probe-lit: rays per probe, a multiple of 64 in 64 .. 4096 (default 256)")
    ap.add_argument("--out", default="render.png")
    ap.add_argument("--checkpoint", help="also save the fp32 accumulation buffer (.npz)")
    args = ap.parse_args(argv)

    make = scenes.CONFIGS[args.config]
    sc = make()
    if args.width and args.height:
        sc = make(args.width, args.height)
    p = sc.params
    if args.spp_per_pass:
        p.samples_per_pixel = args.spp_per_pass
    if args.max_depth:
        p.max_depth = args.max_depth
    if args.passes:
        sc.n_passes = args.passes
    overlay = None
    if args.debug_overlay and args.next_event:
        ap.error("--next-event and --debug-overlay exclude each other")
    if args.debug_overlay:
        if args.config != "default":
            ap.error("--debug-overlay shows the State's own cursor and selection: --config default")
        from .state import State

        st = State(p.width, p.height)  # State::default's camera is default_scene's; its pick ray is the crosshair
        st.set_debugging(True)
        st.pick()
        _, selected, cursor = st.debug_overlay()
        st.close()
        overlay = (selected, cursor)
    t0 = time.perf_counter()
    geom = {"auto": abi.PT_GEOM_AUTO, "lds": abi.PT_GEOM_LDS, "scalar": abi.PT_GEOM_SCALAR, "bvh": abi.PT_GEOM_BVH,
            "grid": abi.PT_GEOM_GRID, "small": abi.PT_GEOM_SMALL}[args.geometry]
    per = min(sc.n_passes, 16)
    if args.adaptive and args.noise_target is None:
        ap.error("--adaptive chooses tiles by the noise target: only with --noise-target")
    denoise = None
    if args.denoise is not None:
        if args.noise_target is None and not args.error_out:
            ap.error("--denoise filters by the error estimate: only with --noise-target or --error-out")
        try:
            denoise = parse_denoise(args.denoise)
        except ValueError as e:
            ap.error("--denoise: %s" % e)
    denoise_patch = None
    if args.denoise_patch is not None:
        if denoise is not None:
            ap.error("--denoise-patch takes --denoise's place: give one of them")
        if args.noise_target is None and not args.error_out:
            ap.error("--denoise-patch filters by the error estimate: only with --noise-target or --error-out")
        try:
            denoise_patch = parse_denoise(args.denoise_patch, abi.PT_FILTER_PATCH_KAPPA_DEFAULT)
        except ValueError as e:
            ap.error("--denoise-patch: %s" % e)
    exposure = None
    if args.tone is not None and args.exposure != "auto":
        try:
            exposure = float(args.exposure)
        except ValueError:
            exposure = float("nan")
        if not (0.0 < exposure < float("inf")):
            ap.error("--exposure: auto, or a finite positive value")
    glare = None
    if args.glare is not None:
        if args.tone is None:
            ap.error("--glare hands over linear radiance: only with --tone")
        glare = glare_options(args.glare, args.glare_levels, args.glare_threshold)
        if glare is None:
            ap.error("--glare: a strength in 0 .. 1, --glare-levels 1 .. %d, --glare-threshold finite and >= 0" % abi.PT_GLARE_MAX_LEVELS)
    if args.probe_lit is not None:
        try:
            lattice_n = tuple(int(v) for v in args.probe_lit.split(","))
        except ValueError:
            lattice_n = ()
        if len(lattice_n) != 3 or not all(abi.PT_LATTICE_MIN_NODES <= v <= abi.PT_LATTICE_MAX_NODES for v in lattice_n) or \
                lattice_n[0] * lattice_n[1] * lattice_n[2] > abi.PT_LATTICE_MAX_TOTAL:
            ap.error("--probe-lit: NX,NY,NZ, each 2 .. 256, at most 2^20 nodes in all")
        if not (abi.PT_GATHER_MIN_DIRECTIONS <= args.probe_directions <= abi.PT_GATHER_MAX_DIRECTIONS and args.probe_directions % 64 == 0):
            ap.error("--probe-directions: a multiple of 64 in 64 .. 4096")
        if overlay is not None or args.noise_target is not None or args.error_out or denoise is not None or denoise_patch is not None or args.checkpoint:
            ap.error("--probe-lit shades from probes: it has no accumulation to measure, filter, overlay or checkpoint")
        curve = None if args.tone is None else {"clamp": abi.PT_TONE_CLAMP, "reinhard": abi.PT_TONE_REINHARD, "filmic": abi.PT_TONE_FILMIC}[args.tone]
        return probe_lit(sc, args, geom, lattice_n, curve, exposure, glare)
    if args.noise_target is not None or args.error_out:
        if overlay is not None:
            ap.error("--noise-target / --error-out measure the frame's noise: not with --debug-overlay")
        pt, acc = render_to_target(sc, args, geom, per)
    else:
        # (pt_tune first, as bench.py does: the grid fitted to this camera, PT_GEOM_AUTO settled before the frame's launches)
        pt, acc = render_scene(sc, device=args.device, passes_per_launch=per, geometry_path=geom, tune=min(per, 8), overlay=overlay,
                              next_event=args.next_event)
    dt = time.perf_counter() - t0
    st = pt.stats()
    toned = args.tone is not None  # (the filters then hand over a LINEAR frame: the tone curve and the sqrt come after them)
    if denoise is not None:
        frame = pt.filtered_image(denoise[0], denoise[1], gamma=not toned)
        print("denoise: radius %d, kappa %g, %.2f accepted taps per pixel" % (denoise[0], denoise[1], float(frame[..., 3].mean())))
        frame[..., 3] = 1.0   # (the taps are no alpha)
    elif denoise_patch is not None:
        frame = pt.patch_filtered_image(denoise_patch[0], abi.PT_FILTER_MAX_PATCH, denoise_patch[1], gamma=not toned)
        print("denoise: radius %d, patch %d, kappa %g, %.2f accepted taps per pixel" % (
            denoise_patch[0], abi.PT_FILTER_MAX_PATCH, denoise_patch[1], float(frame[..., 3].mean())))
        frame[..., 3] = 1.0
    elif not toned:
        frame = pt.resolve(gamma=True)
    else:
        frame = None  # (the accumulation itself)
    if toned:
        curve = {"clamp": abi.PT_TONE_CLAMP, "reinhard": abi.PT_TONE_REINHARD, "filmic": abi.PT_TONE_FILMIC}[args.tone]
        pt.tone_mapping(True)
        if glare is not None:
            pt.glare(True)
            plain = pt.resolve(gamma=False) if frame is None else frame
            frame = pt.glared_image(src=frame, options=glare)
            print("glare: strength %g, %d levels, threshold %g; the frame's brightest channel value %g -> %g" % (
                glare.strength, glare.levels, glare.threshold, float(np.nanmax(plain[..., :3])), float(np.nanmax(frame[..., :3]))))
        pt.meter(abi.PtMeterOptions(), src=frame)
        rec, _ = pt.exposure()
        opt = abi.PtToneOptions(curve, 1, 0.0, 1.0)
        if exposure is not None:
            opt = abi.PtToneOptions(curve, 1, exposure, max(rec.y_high * exposure, 1.0))
        clipped = int((pt.resolve_rgba8(True)[..., :3] == 255).sum())
        frame = pt.toned_image(opt, src=frame)
        print("tone: %s, exposure %g (%s), white %g; key luminance %g, %d lit pixels, %d below 2^-16; %d channel values at 255, %d without the curve" % (
            args.tone, opt.exposure or rec.exposure, "given" if exposure is not None else "metered", opt.white if exposure is not None else rec.white,
            rec.y_key, rec.lit, rec.below, int((frame[..., :3] >= 1.0).sum()), clipped))
    image_io.write_png(args.out, frame)
    if args.error_out:
        err = pt.error_image()
        err[..., :3] *= 8.0
        err[..., 3] = 1.0
        image_io.write_png(args.error_out, err)
    if args.samples_out:
        n = pt.sample_counts()
        img = np.ones(n.shape + (4,), np.float32)
        img[..., :3] = (n / max(float(n.max()), 1.0))[..., None]
        image_io.write_png(args.samples_out, img)
    if args.checkpoint:
        image_io.save_accum(args.checkpoint, acc, st.total_spp)
    if args.features:
        pt.feature_planes(True)
        pt.render_features()
        planes = pt.features()
        for name in ("albedo", "normal", "point", "ids"):
            np.save("%s_%s.npy" % (args.features, name), planes[name])
        hit = planes["ids"][..., 0] >= 0
        print("features: %d of %d pixels hit, %d different spheres -> %s_{albedo,normal,point,ids}.npy" % (
            int(hit.sum()), hit.size, len(np.unique(planes["ids"][..., 0][hit])), args.features))
    print("%s: %dx%d, %d spheres, %d spp, depth %d: %.2f s, %.0f Mray/s -> %s" % (
        sc.name, p.width, p.height, len(sc.spheres), st.total_spp, p.max_depth, dt, st.segments / dt / 1e6, args.out))
    pt.close()


def parse_denoise(text, kappa_default=abi.PT_FILTER_KAPPA_DEFAULT):
    """--denoise's (or --denoise-patch's) value "R" or "R,KAPPA" -> (radius, kappa); ValueError says what is wrong with it."""
    parts = text.split(",")
    if len(parts) > 2:
        raise ValueError("R or R,KAPPA, not %r" % text)
    radius = int(parts[0])
    kappa = float(parts[1]) if len(parts) == 2 else kappa_default
    if not 0 <= radius <= abi.PT_FILTER_MAX_RADIUS:
        raise ValueError("the radius is 0 to %d" % abi.PT_FILTER_MAX_RADIUS)
    if not math.isfinite(kappa) or kappa < 0.0:
        raise ValueError("kappa is finite and not negative")
    return radius, kappa


def render_to_target(sc, args, geom, per):
    """The scene with the error estimate on: to --noise-target (at most --max-spp), or its fixed passes when only --error-out
    is asked for.  Returns (PathTracer, accum) like render_scene."""
    p = sc.params.copy()
    p.time_step = abi.PT_TIME_STEP_DECORRELATED
    pt = PathTracer(p.width, p.height, device=args.device)
    pt.set_geometry_path(geom)
    pt.set_spheres(sc.spheres)
    if args.next_event:
        pt.next_event(True)
    pt.set_params(p)
    pt.reserve_passes(per)
    pt.tune(min(per, 8))
    pt.error_estimate(True)
    max_passes = sc.n_passes if not args.max_spp else max(1, args.max_spp // p.samples_per_pixel)
    # (without a target: one that cannot be met, so the fixed number of passes is rendered)
    if args.adaptive:
        es, ad = pt.render_adaptive(args.noise_target, per, max_passes)
        uniform = es.pixels * es.passes_rendered * p.samples_per_pixel
        print("adaptive: %d rounds, %d of them partial, %d of %d tiles still active, %.1f %% of the uniform samples traced" % (
            ad.rounds, ad.partial_rounds, ad.tiles_active, ad.tiles, 100.0 * ad.samples / max(uniform, 1)))
    else:
        es = pt.render_until(args.noise_target if args.noise_target is not None else 1e-30, per, max_passes)
    print("%d spp rendered (%d passes of %d), rel_error %.5f, rms_error %.5g, reached %d" % (
        es.passes_rendered * p.samples_per_pixel, es.passes_rendered, p.samples_per_pixel, es.rel_error, es.rms_error, es.reached))
    return pt, pt.accum()


if __name__ == "__main__":
    main()
