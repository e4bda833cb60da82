"""PathTracer — thin Python handle on a pt_ctx (include/ptrace.h).

Mirrors how the reference drives its GPU boundary: set_geometry once (src/lib.rs:57), run the
uniform setters and render every frame (src/lib.rs:92-102), read the result out.  Device memory
and streams can come from PyTorch (`use_torch=True`): the accumulation buffer is then a torch
tensor bound with pt_bind_accum and kernels run on torch's current stream, which is what the
multi-GPU gather (dist.py) and bench.py's timing need.  PyTorch is plumbing here, not compute.
"""
import ctypes as C

import numpy as np

from . import abi
from ._lib import load


class PtError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libptrace error %d: %s" % (code, message))
        self.code = code


class _Arrays:
    """The array library of one call, chosen once: numpy on the host (`torch` None), or torch on `device`.  What the entry points
    that take or give arrays need of either: a contiguous float32 copy of an input where it must live (`f32`; `rows`: as
    (n, k)), fresh arrays (`zeros`, `empty`: numpy dtypes name the element type for both), the pointer the library takes
    (`ptr`), a reinterpreting view (`view`), and `cat`, `where` and `at_least` (an element-wise lower bound)."""

    def __init__(self, torch=None, device=None):
        self.torch, self.device = torch, device

    def _dtype(self, dtype):
        return getattr(self.torch, np.dtype(dtype).name) if self.torch else dtype

    def f32(self, v):
        if self.torch:
            return v.to(device=self.device, dtype=self.torch.float32).contiguous()
        return np.ascontiguousarray(v, dtype=np.float32)

    def rows(self, v, k=3):
        return self.f32(v).reshape(-1, k)

    def zeros(self, shape, dtype=np.float32):
        return self.torch.zeros(shape, dtype=self._dtype(dtype), device=self.device) if self.torch else np.zeros(shape, dtype)

    def empty(self, shape, dtype=np.float32):
        return self.torch.empty(shape, dtype=self._dtype(dtype), device=self.device) if self.torch else np.empty(shape, dtype)

    def ptr(self, a):
        return C.c_void_p(a.data_ptr()) if self.torch else a.ctypes.data_as(C.c_void_p)

    def view(self, a, dtype):
        return a.view(self._dtype(dtype))

    def cat(self, parts):
        return self.torch.cat(parts, dim=1) if self.torch else np.concatenate(parts, axis=1)

    def where(self, cond, a, b):
        return (self.torch or np).where(cond, a, b)

    def at_least(self, a, low):
        return self.torch.clamp(a, min=low) if self.torch else np.maximum(a, np.float32(low))


class PathTracer:
    def __init__(self, width, height, device=0, use_torch=False):
        self.lib = load()
        self.width, self.height = int(width), int(height)
        self.device = int(device)
        self._ctx = C.c_void_p()
        self.use_torch = bool(use_torch)
        stream_handle = None
        if self.use_torch:
            import torch

            self._torch = torch
            try:
                stream = torch.cuda.current_stream(self.device)
            except RuntimeError as e:  # e.g. "No HIP GPUs are available": a second HIP runtime in this process (_lib.py)
                raise PtError(abi.PT_ERR_NO_DEVICE, "PyTorch cannot see the GPU libptrace is using (%s): two HIP runtimes in one "
                              "process?  `import torch` before anything of ray_tracer_webgl_amd" % e) from e
            # torch's default stream is the NULL stream, and NULL means "the context's own stream" in this
            # ABI: name it as hipStreamLegacy (1).  Kernels must run on the stream torch orders its own work
            # on, or a gather / .cpu() right after render_passes reads the buffer before they have written it.
            # The context is CREATED on that stream (pt_create_on_stream): it never makes a stream — an HSA queue,
            # 80-150 ms when it is the process's first — that it would not use.
            stream_handle = C.c_void_p(stream.cuda_stream or abi.PT_STREAM_LEGACY)
            rc = self.lib.pt_create_on_stream(C.byref(self._ctx), self.device, self.width, self.height, stream_handle)
        else:
            rc = self.lib.pt_create(C.byref(self._ctx), self.device, self.width, self.height)
        if rc != abi.PT_OK:
            msg = self.lib.pt_last_error(None)
            self._ctx = C.c_void_p()
            raise PtError(rc, msg.decode() if msg else "pt_create failed")
        self.params = None
        self.local_rows = self.height
        self.accum_tensor = None
        self._keep = None

    # -- plumbing -------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != abi.PT_OK:
            msg = self.lib.pt_last_error(self._ctx)
            raise PtError(rc, msg.decode() if msg else "")
        return rc

    def close(self):
        if self._ctx:
            self.lib.pt_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _arrays(self, device=None):
        """the array library of a call: torch on `device` (a torch.device or its name), numpy for None"""
        return _Arrays(self._torch, device) if device is not None else _Arrays()

    def _device_of(self, v):
        """the device of a torch device tensor under use_torch; None for anything else: a host array"""
        return v.device if self.use_torch and self._torch.is_tensor(v) and v.is_cuda else None

    def _rays(self, what, xp, origins, directions):
        """the (n, 8) float32 PtRay records {origin, pad, direction, pad} of two (n, 3) inputs"""
        o, d = xp.rows(origins), xp.rows(directions)
        if o.shape != d.shape:
            raise ValueError("%s: %d origins, %d directions" % (what, o.shape[0], d.shape[0]))
        rays = xp.zeros((int(o.shape[0]), 8))
        rays[:, 0:3] = o
        rays[:, 4:7] = d
        return rays

    # -- scene / uniforms -----------------------------------------------------------------------
    def set_spheres(self, spheres):
        ptr, n, keep = abi.spheres_as_ctypes(spheres)
        self._check(self.lib.pt_set_spheres(self._ctx, ptr, n))
        self.n_spheres = n

    def set_params(self, params):
        self.params = params.copy()
        rows = abi.local_rows(self.height, params.band_rows, params.band_index, params.band_count)
        if self.use_torch and self.accum_tensor is not None and self.accum_tensor.shape[0] != max(rows, 1):
            # a different row partition: give the old tensor back before the context resizes
            self._check(self.lib.pt_bind_accum(self._ctx, None, 0))
            self.accum_tensor = None
        self._check(self.lib.pt_set_params(self._ctx, C.byref(self.params)))
        self.local_rows = rows
        if self.use_torch:
            self._bind_torch_accum()

    def _bind_torch_accum(self):
        torch = self._torch
        shape = (max(self.local_rows, 1), self.width, 4)
        if self.accum_tensor is None or tuple(self.accum_tensor.shape) != shape:
            self.accum_tensor = torch.zeros(shape, dtype=torch.float32, device="cuda:%d" % self.device)
            nbytes = self.accum_tensor.numel() * 4
            self._check(self.lib.pt_bind_accum(self._ctx, C.c_void_p(self.accum_tensor.data_ptr()), nbytes))

    def set_geometry_path(self, path):
        """abi.PT_GEOM_AUTO (default: measure the usable paths once per scene) / PT_GEOM_LDS /
        PT_GEOM_SCALAR / PT_GEOM_BVH / PT_GEOM_GRID."""
        self._check(self.lib.pt_set_option(self._ctx, abi.PT_OPT_GEOMETRY_PATH, int(path)))

    def set_count_work(self, on=True):
        """Walk kernels: launch the measuring twin, which fills stats().work (executed iterations
        and active lanes per phase).  Slower; never time it."""
        self._check(self.lib.pt_set_option(self._ctx, abi.PT_OPT_COUNT_WORK, int(on)))  # (2: dev tools, + the grid twins' gather histogram)

    def set_carry_lanes(self, n):
        """Walk kernels: move on to shading when fewer than n lanes (and less than half the wave)
        still walk; 0 = lockstep.  Scheduling only: images do not depend on it."""
        self._check(self.lib.pt_set_option(self._ctx, abi.PT_OPT_CARRY_LANES, int(n)))

    def set_refill_min(self, n):
        """Lanes of a busy wave that wait for a new item before the item decode runs (1 = at once).
        Stored and accepted; the look-ahead refill (every lane holds a decoded next item) does not consult it.
        Scheduling only: images do not depend on it."""
        self._check(self.lib.pt_set_option(self._ctx, abi.PT_OPT_REFILL_MIN, int(n)))

    def set_russian_roulette(self, min_depth):
        """Opt-in perf mode (0 = off, the default): after `min_depth` bounces a path survives each further
        bounce with probability min(max(throughput), 1) and is re-weighted.  Same expectation per pixel
        as the reference's estimator, different samples: bit-comparable with oracle.render(..., roulette=min_depth),
        not with the roulette-free oracle.  A context set to PT_GEOM_LDS renders through the scalar walk meanwhile."""
        self._check(self.lib.pt_set_option(self._ctx, abi.PT_OPT_RUSSIAN_ROULETTE, int(min_depth)))

    def next_event(self, on=True):
        """Next-event estimation (PT_OPT_NEXT_EVENT; off by default): at every DIFFUSE hit whose path goes on, the render launches
        sample one of the scene's emissive spheres through a shadow ray, and a path that then runs into a light it could have
        sampled adds nothing.  Same expectation per pixel as the plain estimator, different samples: bit-comparable with
        tests/nee_ref.py, not with the oracle (a scene without lights renders the oracle's bits).  Excludes Russian roulette,
        the debug overlay and the measuring twins; the feature, query and radiance calls stay the plain estimator."""
        self._check(self.lib.pt_set_option(self._ctx, abi.PT_OPT_NEXT_EVENT, 1 if on else 0))

    def set_debug_overlay(self, enable, selected_object=abi.NO_SELECTED_OBJECT_ID, cursor_point=(0.0, 0.0, 0.0)):
        """The shader's debug overlay (static/shader.frag:307-318; pt_set_debug_overlay): hits within 0.1 of `cursor_point`
        are blue, the silhouette band of the sphere whose uuid is `selected_object` is red, and such a path ends there.
        Off by default; enable=False restores the plain kernels and their bits.  Excludes Russian roulette."""
        cur = (C.c_float * 3)(*[float(x) for x in cursor_point])
        self._check(self.lib.pt_set_debug_overlay(self._ctx, 1 if enable else 0, int(selected_object), cur))

    def last_trace_build(self):
        """abi.BUILD_*: which build of the trace kernel the most recent launch was."""
        rc = self.lib.pt_last_trace_build(self._ctx)
        if rc < 0:
            raise PtError(rc, "pt_last_trace_build failed")
        return rc

    def set_grid_fit(self, unmeasured):
        """How tune() chooses the grid's margin class: False (default) it times the candidates, True it takes the smallest
        class that covers the camera without launching anything (PT_OPT_GRID_FIT).  Speed only."""
        self._check(self.lib.pt_set_option(self._ctx, abi.PT_OPT_GRID_FIT, 1 if unmeasured else 0))

    def tune(self, n_passes):
        """Fit the context to scene and uniforms: the grid is rebuilt for the margin class that renders this view fastest
        (measured: one timed launch of n_passes passes per candidate class; speed only), then PT_GEOM_AUTO is settled now
        (one cold + one untimed launch of n_passes passes per usable path); clears the accumulation."""
        self._check(self.lib.pt_tune(self._ctx, int(n_passes)))
        if self.accum_tensor is not None:
            self.accum_tensor.zero_()

    def refit_grid(self, only_if_stale=False):
        """Rebuild the grid for the margin class the current camera needs (pt_refit_grid): what a frame loop does when
        grid_fit() says 1.  No measuring launches; accumulation, textures and statistics stay."""
        self._check(self.lib.pt_refit_grid(self._ctx, 1 if only_if_stale else 0))

    def grid_fit(self):
        """0: the grid fits the camera of the last set_params (or there is none / another path is in use); 1: the camera
        stands outside the region whose rays walk the cells — every primary ray is tested against the whole list;
        2: a smaller margin class would do.  Host arithmetic, no synchronisation (PtStats.grid_fit_stale)."""
        rc = self.lib.pt_grid_fit(self._ctx)
        if rc < 0:
            raise PtError(rc, "pt_grid_fit failed")
        return rc

    def reserve_passes(self, n):
        self._check(self.lib.pt_reserve_passes(self._ctx, int(n)))

    # -- rendering ------------------------------------------------------------------------------
    def render(self):
        self._check(self.lib.pt_render(self._ctx))

    def render_passes(self, n):
        self._check(self.lib.pt_render_passes(self._ctx, int(n)))

    def reset(self):
        self._check(self.lib.pt_reset_accum(self._ctx))
        if self.accum_tensor is not None:
            self.accum_tensor.zero_()

    def synchronize(self):
        self._check(self.lib.pt_synchronize(self._ctx))

    def wait(self, timeout_s):
        """Dev tools' watchdog (include/ptrace_dev.h pt_debug_wait): True when the stream went idle within
        timeout_s, False on timeout.  Polls an event, never blocks in the driver."""
        fn = self.lib.pt_debug_wait
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_uint]
        rc = fn(self._ctx, int(timeout_s * 1000))
        if rc < 0:
            raise PtError(rc, "pt_debug_wait failed")
        return rc == 0

    # -- the reference's frame on device-resident textures ---------------------------------------
    def clear_textures(self):
        self._check(self.lib.pt_clear_textures(self._ctx))

    def render_frame(self, even_odd_count):
        """One animation tick (src/lib.rs:92-102) with the current uniforms: trace one pass, blend
        with texture[(even_odd_count + 1) % 2], draw to the canvas (and, when averaging, to the
        other texture).  Asynchronous; nothing crosses PCIe."""
        self._check(self.lib.pt_render_frame(self._ctx, int(even_odd_count) & 0xFFFFFFFF))

    def render_frames(self, even_odd_count, max_render_count, n_frames):
        """n ticks at the constant frame interval params.time_step, replayed from hipGraphs (groups of 64, 16 and 4 frames, then singles) with
        the per-frame state (u_time, render_count, even/odd) counted on the device."""
        self._check(self.lib.pt_render_frames(self._ctx, int(even_odd_count) & 0xFFFFFFFF, int(max_render_count), int(n_frames)))

    def read_canvas(self):
        out = np.empty((self.local_rows, self.width, 4), dtype=np.uint8)
        if out.size:
            self._check(self.lib.pt_read_canvas(self._ctx, out.ctypes.data_as(C.c_void_p)))
        return out

    def read_texture(self, index):
        out = np.empty((self.local_rows, self.width, 4), dtype=np.uint8)
        if out.size:
            self._check(self.lib.pt_read_texture(self._ctx, int(index), out.ctypes.data_as(C.c_void_p)))
        return out

    def write_texture(self, index, rgba8):
        a = np.ascontiguousarray(rgba8, dtype=np.uint8)
        if a.shape != (self.local_rows, self.width, 4):
            raise ValueError("texture is %s, this context holds %s" % (a.shape, (self.local_rows, self.width, 4)))
        self._check(self.lib.pt_write_texture(self._ctx, int(index), a.ctypes.data_as(C.c_void_p)))

    # -- read-out -------------------------------------------------------------------------------
    def resolve(self, gamma=True):
        out = np.empty((self.local_rows, self.width, 4), dtype=np.float32)
        if out.size:
            self._check(self.lib.pt_resolve(self._ctx, out.ctypes.data_as(C.c_void_p), 1 if gamma else 0))
        return out

    def resolve_rgba8(self, gamma=True):
        out = np.empty((self.local_rows, self.width, 4), dtype=np.uint8)
        if out.size:
            self._check(self.lib.pt_resolve_rgba8(self._ctx, out.ctypes.data_as(C.c_void_p), 1 if gamma else 0))
        return out

    def blend_rgba8(self, prev):
        prev = np.ascontiguousarray(prev, dtype=np.uint8)
        out = np.empty_like(prev)
        self._check(self.lib.pt_blend_rgba8(self._ctx, prev.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def accum(self):
        """Raw accumulation buffer (local_rows, width, 4) fp32: rgb sums, a = spp."""
        self.synchronize()
        if self.accum_tensor is not None:
            self._torch.cuda.current_stream(self.device).synchronize()
            return self.accum_tensor[: self.local_rows].cpu().numpy()
        out = np.empty((self.local_rows, self.width, 4), dtype=np.float32)
        if out.size:
            self._check(self.lib.pt_read_accum(self._ctx, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def load_accum(self, accum):
        """Resume from a checkpoint: `accum` is what accum() returned earlier (rgb sums, a = spp)
        for the same image size and row partition (image_io.load_accum reads one from disk)."""
        a = np.ascontiguousarray(accum, dtype=np.float32)
        if a.shape != (self.local_rows, self.width, 4):
            raise ValueError("accumulation checkpoint is %s, this context holds %s"
                             % (a.shape, (self.local_rows, self.width, 4)))
        self._check(self.lib.pt_load_accum(self._ctx, a.ctypes.data_as(C.c_void_p), a.nbytes))

    # -- the per-pixel error estimate (include/ptrace.h PT_OPT_ERROR_ESTIMATE) --------------------
    def error_estimate(self, on=True):
        """Keep a per-pixel error estimate beside the accumulation: mean and M2 of the pass sums (batch means), folded
        by the kernel that folds the slabs.  Off by default; the image bits are the same either way.  The estimate
        speaks for the passes folded since its last clear (reset, tune, resize, repartition, load_accum, bind), all of
        which must have the same samples_per_pixel, and assumes independent passes (time_step such as
        abi.PT_TIME_STEP_DECORRELATED)."""
        self._check(self.lib.pt_set_option(self._ctx, abi.PT_OPT_ERROR_ESTIMATE, 1 if on else 0))

    def error_state(self):
        """The raw state (local_rows, width, 2, 4) fp32: [..., 0, :] = {mean.rgb, n}, [..., 1, :] = {M2.rgb, k}."""
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        self._check(self.lib.pt_error_ptr(self._ctx, C.byref(ptr), C.byref(nbytes)))
        self.synchronize()
        out = np.empty((self.local_rows, self.width, 2, 4), dtype=np.float32)
        assert out.nbytes == nbytes.value
        if out.size:
            _memcpy(out.ctypes.data_as(C.c_void_p), ptr, out.nbytes, _D2H)
        return out

    def load_error_state(self, state):
        """Overwrite the raw state (tests and checkpoints): the inverse of error_state()."""
        a = np.ascontiguousarray(state, dtype=np.float32)
        if a.shape != (self.local_rows, self.width, 2, 4):
            raise ValueError("error state is %s, this context holds %s" % (a.shape, (self.local_rows, self.width, 2, 4)))
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        self._check(self.lib.pt_error_ptr(self._ctx, C.byref(ptr), C.byref(nbytes)))
        self.synchronize()
        if a.size:
            _memcpy(ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, _H2D)

    def error_image(self):
        """(local_rows, width, 4) fp32: the standard error of each pixel's mean as linear radiance, a = passes folded."""
        out = np.empty((self.local_rows, self.width, 4), dtype=np.float32)
        if out.size:
            self._check(self.lib.pt_resolve_error(self._ctx, out.ctypes.data_as(C.c_void_p)))
        return out

    def filtered_image(self, radius=2, kappa=abi.PT_FILTER_KAPPA_DEFAULT, gamma=True):
        """(local_rows, width, 4) fp32: the estimate's own mean of each pixel averaged with the neighbours within `radius`
        (at most abi.PT_FILTER_MAX_RADIUS) whose means differ from it by no more than `kappa` standard errors of the
        difference (include/ptrace.h pt_resolve_filtered); a = the accepted taps, 0 where the estimate has nothing to say.
        Reads the estimate's state only: it speaks for the passes the estimate knows of.  A band context filters inside its
        own row chunks."""
        out = np.empty((self.local_rows, self.width, 4), dtype=np.float32)
        if out.size:
            self._check(self.lib.pt_resolve_filtered(self._ctx, out.ctypes.data_as(C.c_void_p), int(radius), float(kappa), 1 if gamma else 0))
        return out

    def patch_filtered_image(self, radius=2, patch=abi.PT_FILTER_MAX_PATCH, kappa=abi.PT_FILTER_PATCH_KAPPA_DEFAULT, gamma=True):
        """filtered_image with the patch-wise test (include/ptrace.h pt_resolve_filtered_patch): a neighbour is averaged in when
        the (2 patch + 1)^2 neighbourhoods around the two pixels differ by no more than `kappa` standard errors, squared
        differences and variances summed over the patch; patch at most abi.PT_FILTER_MAX_PATCH, patch 0 gives filtered_image's
        bits.  a = the accepted taps.  Reads the estimate's state only; a band context filters inside its own row chunks."""
        out = np.empty((self.local_rows, self.width, 4), dtype=np.float32)
        if out.size:
            self._check(self.lib.pt_resolve_filtered_patch(self._ctx, out.ctypes.data_as(C.c_void_p), int(radius), int(patch),
                                                           float(kappa), 1 if gamma else 0))
        return out

    def error_tiles(self):
        """(tiles_y, tiles_x, 4) fp32 per 8x8 tile of the local rows: {sum se^2, sum mean^2, counted pixels, min passes}."""
        tx, ty = C.c_uint32(), C.c_uint32()
        self._check(self.lib.pt_error_tiles(self._ctx, None, C.byref(tx), C.byref(ty)))
        out = np.empty((ty.value, tx.value, 4), dtype=np.float32)
        if out.size:
            self._check(self.lib.pt_error_tiles(self._ctx, out.ctypes.data_as(C.c_void_p), C.byref(tx), C.byref(ty)))
        return out

    def error_stats(self):
        st = abi.PtErrorStats()
        self._check(self.lib.pt_error_stats(self._ctx, C.byref(st)))
        return st

    def render_until(self, target, passes_per_launch, max_passes):
        """Render until the frame's relative error (error_stats().rel_error) is at most `target`, passes_per_launch
        passes at a time, at most max_passes; returns the PtErrorStats of the last look (passes_rendered, reached).
        The context's first_pass advances by the passes rendered: a second call continues the same frame."""
        st = abi.PtErrorStats()
        self._check(self.lib.pt_render_until(self._ctx, float(target), int(passes_per_launch), int(max_passes), C.byref(st)))
        if self.params is not None:
            self.params.first_pass += st.passes_rendered
        return st

    def render_adaptive(self, target, passes_per_round, max_passes):
        """render_until with a choice of tiles between the launches (include/ptrace.h pt_render_adaptive): after every look
        only the 8x8 tiles that still miss their share of the target are traced and folded.  Returns (PtErrorStats,
        PtAdaptiveStats); the context's first_pass advances by the passes rendered, whatever share of the tiles ran."""
        st, ad = abi.PtErrorStats(), abi.PtAdaptiveStats()
        rc = self.lib.pt_render_adaptive(self._ctx, float(target), int(passes_per_round), int(max_passes), C.byref(st), C.byref(ad))
        if self.params is not None:
            self.params.first_pass += st.passes_rendered   # (rounds that ran before a failing one have advanced it too)
        self._check(rc)
        return st, ad

    def adaptive_tiles(self):
        """The tables of the most recent partial round: (base, order, n_active) — the cost order it partitioned and the table
        the trace launch read, uint32 arrays of one entry per tile; the first n_active entries of `order` are the active tiles."""
        n, na = C.c_uint32(), C.c_uint32()
        self._check(self.lib.pt_adaptive_tiles(self._ctx, None, None, C.byref(n), C.byref(na)))
        base, order = np.empty(n.value, np.uint32), np.empty(n.value, np.uint32)
        u32p = C.POINTER(C.c_uint32)
        self._check(self.lib.pt_adaptive_tiles(self._ctx, base.ctypes.data_as(u32p), order.ctypes.data_as(u32p), C.byref(n), C.byref(na)))
        return base, order, int(na.value)

    # -- first-hit feature planes (include/ptrace.h PT_OPT_FEATURES) -------------------------------
    def feature_planes(self, on=True):
        """Allocate (or release) the four first-hit feature planes: albedo + distance, normal, hit point and ids of the
        surface one pinhole ray through each pixel centre meets.  Off by default; the image bits are the same either way."""
        self._check(self.lib.pt_set_option(self._ctx, abi.PT_OPT_FEATURES, 1 if on else 0))

    def render_features(self):
        """One launch that fills the planes for the scene and uniforms in place (pt_render_features): asynchronous, and
        nothing of the accumulation, the estimate or the frame textures moves."""
        self._check(self.lib.pt_render_features(self._ctx))

    def features(self):
        """{"albedo", "normal", "point": float32, "ids": int32}, each (local_rows, width, 4), row 0 = lowest owned row:
        {albedo.rgb, t}, {n.xyz, 0}, {hit point.xyz, 0} and {list index, uuid, type, front_face} on a hit; {background.rgb, 0},
        zeros, zeros and {-1, -1, -1, 0} on a miss.  numpy copies — or, under use_torch, torch views of the device planes
        (no copy, ordered on torch's stream like the accumulation tensor: they answer while the planes exist, change with
        the next render_features and die with the planes).  The numpy read-out raises PtError(PT_ERR_NOT_READY) when the
        scene, the uniforms or the size changed since the last render_features."""
        names = (("albedo", abi.PT_FEAT_ALBEDO), ("normal", abi.PT_FEAT_NORMAL), ("point", abi.PT_FEAT_POINT), ("ids", abi.PT_FEAT_IDS))
        shape = (self.local_rows, self.width, 4)
        out = {}
        if not self.use_torch:
            for name, plane in names:
                a = np.empty(shape, dtype=np.int32 if plane == abi.PT_FEAT_IDS else np.float32)
                # (an empty band too: the call says whether the planes speak)
                self._check(self.lib.pt_read_features(self._ctx, plane, a.ctypes.data_as(C.c_void_p)))
                out[name] = a
            return out
        torch = self._torch
        for name, plane in names:
            ptr, nbytes = C.c_void_p(), C.c_size_t()
            self._check(self.lib.pt_features_ptr(self._ctx, plane, C.byref(ptr), C.byref(nbytes)))
            dtype = torch.int32 if plane == abi.PT_FEAT_IDS else torch.float32
            if nbytes.value == 0:
                out[name] = torch.empty(shape, dtype=dtype, device="cuda:%d" % self.device)
                continue
            view = _DeviceView(ptr.value, shape, "<i4" if plane == abi.PT_FEAT_IDS else "<f4")
            out[name] = torch.as_tensor(view, device="cuda:%d" % self.device)
        return out

    # -- ray queries (include/ptrace.h PT_OPT_RAY_QUERIES) ------------------------------------------
    def ray_queries(self, on=True):
        """Allocate (or release) the query planes of query_rays.  Off by default; the image bits are the same either way."""
        self._check(self.lib.pt_set_option(self._ctx, abi.PT_OPT_RAY_QUERIES, 1 if on else 0))

    def query_batch(self):
        """Rays one launch of query_rays takes (the local pixel count); 0 while it could not answer."""
        return int(self.lib.pt_query_batch(self._ctx))

    _HIT_FIELDS = (("albedo", 0, 3, False), ("t", 3, 4, False), ("normal", 4, 7, False), ("point", 8, 11, False),
                   ("index", 12, 13, True), ("uuid", 13, 14, True), ("type", 14, 15, True), ("front_face", 15, 16, True))

    def query_rays(self, origins, directions):
        """The closest hit of each of the caller's rays (pt_query_rays), through the trace kernels' own intersection: two
        (n, 3) float32 arrays in (directions are not normalised; t is in their units), a dict out — "albedo", "normal",
        "point": (n, 3) float32; "t": (n,) float32; "index", "uuid", "type", "front_face": (n,) int32.  A miss has index
        -1 and the background in "albedo"; an invalid ray (a non-finite component, a direction of three zeros) has index
        abi.PT_RAY_INVALID.  numpy arrays give numpy arrays; under use_torch, torch device tensors give torch device tensors
        (no host copy, ordered on torch's stream).  Synchronous; nothing else of the context moves."""
        xp = self._arrays(self._device_of(origins))
        rays = self._rays("query_rays", xp, origins, directions)
        n = int(rays.shape[0])
        hits = xp.zeros((n, 16), np.int32)
        if n:
            self._check(self.lib.pt_query_rays(self._ctx, xp.ptr(rays), n, xp.ptr(hits)))
        fl = xp.view(hits, np.float32)
        out = {}
        for name, a, b, integer in self._HIT_FIELDS:
            col = (hits if integer else fl)[:, a:b]
            out[name] = col if b - a > 1 else col[:, 0]
        return out

    def query_radiance(self, origins, directions, passes=1, next_event=False):
        """The path-traced radiance along each of the caller's rays (pt_query_radiance; needs ray_queries(True)): `passes`
        passes (at most those reserved) of the uniforms' samples_per_pixel samples per ray by the plain estimator — or, with
        next_event=True (pt_query_radiance_nee; needs next_event(True) as well), by the next-event estimator: the caller's ray
        is a path's first segment, the lamps are sampled from its first DIFFUSE hit on; the same expectation.  Two (n, 3)
        float32 arrays in (directions are not normalised), a dict out — "sum": (n, 3) float32, "samples": (n,) float32, "mean":
        (n, 3) float32 = sum / samples, 0 where samples is 0 (an invalid ray).  numpy arrays give numpy arrays; under
        use_torch, torch device tensors give torch device tensors.  Synchronous; nothing else of the context moves, first_pass
        included."""
        fn = self.lib.pt_query_radiance_nee if next_event else self.lib.pt_query_radiance
        xp = self._arrays(self._device_of(origins))
        rays = self._rays("query_radiance", xp, origins, directions)
        n = int(rays.shape[0])
        rec = xp.zeros((n, 4))
        if n:
            self._check(fn(self._ctx, xp.ptr(rays), n, int(passes), xp.ptr(rec)))
        samples = rec[:, 3]
        mean = xp.where(samples[:, None] > 0, rec[:, 0:3] / xp.at_least(samples, 1.0)[:, None], xp.zeros((n, 3)))
        return {"sum": rec[:, 0:3], "samples": samples, "mean": mean}

    # -- gather queries: irradiance at points and SH probes (include/ptrace.h pt_gather_irradiance, pt_bake_probes) --
    def _gather(self, fn, what, positions, normals, directions, passes, floats):
        """`fn` over n items: (n, floats) float32 records, numpy for numpy arrays and a torch device tensor for torch device
        tensors under use_torch"""
        if not (abi.PT_GATHER_MIN_DIRECTIONS <= int(directions) <= abi.PT_GATHER_MAX_DIRECTIONS and int(directions) % 64 == 0):
            raise ValueError("%s: %d directions (a multiple of 64 in [%d, %d])" % (what, directions, abi.PT_GATHER_MIN_DIRECTIONS, abi.PT_GATHER_MAX_DIRECTIONS))
        xp = self._arrays(self._device_of(positions))
        pos = xp.rows(positions)
        n = int(pos.shape[0])
        items = xp.zeros((n, 8))  # PtGatherPoint: {position, pad, normal, pad}
        items[:, 0:3] = pos
        if normals is not None:
            nrm = xp.rows(normals)
            if nrm.shape != pos.shape:
                raise ValueError("%s: %d positions, %d normals" % (what, n, nrm.shape[0]))
            items[:, 4:7] = nrm
        rec = xp.zeros((n, floats))
        if n:
            self._check(fn(self._ctx, xp.ptr(items), n, int(directions), int(passes), xp.ptr(rec)))
        return rec

    def gather_irradiance(self, points, normals, directions=256, passes=1, next_event=False):
        """The irradiance at each point of a surface with that normal (pt_gather_irradiance; needs ray_queries(True)):
        `directions` cosine-weighted rays per point (a multiple of 64 in [64, 4096]), made, walked by query_radiance's plain
        estimator and reduced on the device.  Two (n, 3) float32 arrays in (normals of any length), a dict out — "e": (n, 3)
        float32, "samples": (n,) float32, 0 for an invalid item (a non-finite component, a normal of three zeros).  numpy
        arrays give numpy arrays; under use_torch, torch device tensors give torch device tensors.  Synchronous; nothing else
        of the context moves.  next_event=True (pt_gather_irradiance_nee; needs next_event(True) as well): the rays are walked
        by query_radiance's next-event estimator; no light sample is drawn at the point itself."""
        rec = self._gather(self.lib.pt_gather_irradiance_nee if next_event else self.lib.pt_gather_irradiance, "gather_irradiance", points, normals, directions, passes, 4)
        return {"e": rec[:, 0:3], "samples": rec[:, 3]}

    def bake_probes(self, positions, directions=256, passes=1, next_event=False):
        """An SH probe of bands 0 to 2 at each position (pt_bake_probes; needs ray_queries(True)): `directions` rays over the
        sphere per probe.  An (n, 3) float32 array in, a dict out — "sh": (n, 9, 3) float32 in abi.PtProbeSH's order,
        "samples": (n,) float32, 0 for an invalid item.  abi.sh_irradiance(sh, normals) gives the irradiance the record holds
        for a normal.  Arrays and tensors as gather_irradiance takes them; next_event=True (pt_bake_probes_nee) likewise."""
        rec = self._gather(self.lib.pt_bake_probes_nee if next_event else self.lib.pt_bake_probes, "bake_probes", positions, None, directions, passes, 28)
        return {"sh": rec[:, 0:27].reshape(-1, 9, 3), "samples": rec[:, 27]}

    # -- probe lattices: bake a lattice of SH probes, shade the feature planes from it (include/ptrace.h pt_bake_lattice) --
    def bake_lattice(self, lattice, directions=256, passes=1, next_event=False, first=0, count=None):
        """The SH probes of nodes first .. first + count - 1 of an abi.PtProbeLattice (pt_bake_lattice; needs ray_queries(True),
        and next_event(True) for next_event=True): the points are made on the device and baked as bake_probes bakes them — the
        records of item k are bake_probes' for the k-th point of the slice, bit for bit; an item's seeds follow its index in
        the call, so a sliced bake draws other samples than a whole one.  count=None: every node from `first` on.  The
        bake_probes dict out — "sh": (count, 9, 3) float32, "samples": (count,) float32 — as numpy arrays, or as torch device
        tensors under use_torch (the records never leave the device: probe_lit_image takes them)."""
        if not (abi.PT_GATHER_MIN_DIRECTIONS <= int(directions) <= abi.PT_GATHER_MAX_DIRECTIONS and int(directions) % 64 == 0):
            raise ValueError("bake_lattice: %d directions (a multiple of 64 in [%d, %d])" % (directions, abi.PT_GATHER_MIN_DIRECTIONS, abi.PT_GATHER_MAX_DIRECTIONS))
        lat = lattice.copy()
        n = lat.nodes - int(first) if count is None else int(count)
        if n < 0:
            raise ValueError("bake_lattice: first %d beyond the lattice's %d nodes" % (first, lat.nodes))
        xp = self._arrays("cuda:%d" % self.device if self.use_torch else None)
        rec = xp.zeros((n, 28))
        # (count == 0 too: the call says whether the lattice and the slice are valid)
        self._check(self.lib.pt_bake_lattice(self._ctx, C.byref(lat), int(first), n, int(directions), int(passes), 1 if next_event else 0, xp.ptr(rec)))
        return {"sh": rec[:, 0:27].reshape(-1, 9, 3), "samples": rec[:, 27]}

    def probe_lit_image(self, lattice, probes, options=None):
        """(local_rows, width, 4) fp32: the feature planes in place shaded from a lattice's records (pt_shade_probes; needs
        feature_planes(True) and a render_features() of the view) — linear RGBA, alpha 0 where no probe was usable; what
        meter(src=...), glared_image(src=...) and toned_image(src=...) take next.  `probes`: the records of every node in node
        order — a bake_lattice dict, or (nodes, 28) float32 — as numpy arrays (a numpy image out) or, under use_torch, torch
        device tensors (a torch device tensor out, nothing crosses the bus).  `options`: abi.PtProbeShadeOptions (default:
        the half-space test on, no bias)."""
        lat = lattice.copy()
        on_device = self.use_torch and self._torch.is_tensor(probes["sh"] if isinstance(probes, dict) else probes)
        xp = self._arrays("cuda:%d" % self.device if on_device else None)
        if isinstance(probes, dict):
            probes = xp.cat([xp.f32(probes["sh"]).reshape(-1, 27), xp.f32(probes["samples"]).reshape(-1, 1)])
        rec = xp.f32(probes)
        out = xp.empty((self.local_rows, self.width, 4))
        if tuple(rec.shape) != (lat.nodes, 28):
            raise ValueError("probe_lit_image: records of shape %s for a lattice of %d nodes" % (tuple(rec.shape), lat.nodes))
        opt = C.byref(options) if options is not None else None
        self._check(self.lib.pt_shade_probes(self._ctx, C.byref(lat), xp.ptr(rec), opt, xp.ptr(out)))
        return out

    # -- exposure metering and the toned read-outs (include/ptrace.h PT_OPT_TONEMAP) -----------------
    def tone_mapping(self, on=True):
        """Put the exposure state in place (or release it: the exposure is forgotten).  Off by default; the image bits are the
        same either way.  The exposure survives set_spheres, set_params, resize and reset."""
        self._check(self.lib.pt_set_option(self._ctx, abi.PT_OPT_TONEMAP, 1 if on else 0))

    def _tone_src(self, src):
        """(pointer, object to keep alive) of a source image: None is the accumulation; a (local_rows, width, 4) float32 numpy
        array is read from the host; under use_torch a torch device tensor is read in place; a ctypes.c_void_p is taken as
        a device pointer to such texels (the caller keeps the memory alive)."""
        if src is None:
            return None, None
        if isinstance(src, C.c_void_p):
            return src, None
        shape = (self.local_rows, self.width, 4)
        if self.use_torch and self._torch.is_tensor(src) and src.is_cuda:
            t = src.to(self._torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError("source image is %s, this context holds %s" % (tuple(t.shape), shape))
            return C.c_void_p(t.data_ptr()), t  # (the context runs on torch's current stream: the tensor's writes come first)
        a = np.ascontiguousarray(src, dtype=np.float32)
        if a.shape != shape:
            raise ValueError("source image is %s, this context holds %s" % (a.shape, shape))
        return a.ctypes.data_as(C.c_void_p), a

    def meter(self, options=None, src=None):
        """Meter the frame on the device (pt_meter): the luminance histogram of the window's pixels, then the exposure record
        from it and the record before.  `options`: abi.PtMeterOptions (default: the header's).  `src`: None for the
        accumulation, or linear RGBA float32 texels (see _tone_src).  Asynchronous unless `src` is a host array."""
        opt = options if options is not None else abi.PtMeterOptions()
        ptr, keep = self._tone_src(src)
        self._check(self.lib.pt_meter(self._ctx, ptr, C.byref(opt)))
        del keep

    def exposure(self):
        """(abi.PtExposure, histogram (256,) uint32) of the last metering (pt_meter_read).  Synchronises."""
        rec = abi.PtExposure()
        hist = np.zeros(256, np.uint32)
        self._check(self.lib.pt_meter_read(self._ctx, C.byref(rec), hist.ctypes.data_as(C.POINTER(C.c_uint32))))
        return rec, hist

    def set_exposure(self, rec):
        """Load an exposure record (pt_meter_set): what a rank does with the record solved from the ranks' summed histograms."""
        r = rec.copy()
        self._check(self.lib.pt_meter_set(self._ctx, C.byref(r)))

    @staticmethod
    def solve_exposure(hist, below, options=None, prev=None):
        """Kernel 2 on the host (pt_exposure_solve; no device and no context): the record of a histogram (256 counts) and `below` under
        `options`, after the record `prev` (None: never valid)."""
        opt = options if options is not None else abi.PtMeterOptions()
        h = np.ascontiguousarray(hist, dtype=np.uint32)
        if h.shape != (256,):
            raise ValueError("solve_exposure: the histogram has 256 bins, not %s" % (h.shape,))
        out = abi.PtExposure()
        p = C.byref(prev) if prev is not None else None
        rc = load().pt_exposure_solve(h.ctypes.data_as(C.POINTER(C.c_uint32)), int(below), C.byref(opt), p, C.byref(out))
        if rc != abi.PT_OK:
            raise PtError(rc, "pt_exposure_solve: invalid options")
        return out

    def _toned(self, fn, dtype, options, src):
        opt = options if options is not None else abi.PtToneOptions()
        ptr, keep = self._tone_src(src)
        xp = self._arrays(keep.device if keep is not None and not isinstance(keep, np.ndarray) else None)
        out = xp.empty((self.local_rows, self.width, 4), dtype)
        if self.local_rows * self.width:
            self._check(fn(self._ctx, ptr, C.byref(opt), xp.ptr(out)))
        return out

    def toned_image(self, options=None, src=None):
        """(local_rows, width, 4) fp32: the frame exposed, through the curve, optionally square-rooted (pt_resolve_toned);
        a = 1.  `options`: abi.PtToneOptions — exposure 0 uses the device record of the last meter() or set_exposure().  A
        numpy or no `src` gives a numpy array; a torch device tensor gives a torch device tensor."""
        return self._toned(self.lib.pt_resolve_toned, np.float32, options, src)

    def toned_rgba8(self, options=None, src=None):
        """The same as bytes, alpha 255 (pt_resolve_toned_rgba8)."""
        return self._toned(self.lib.pt_resolve_toned_rgba8, np.uint8, options, src)

    # -- glare: the bloom pyramid ahead of the toned read-out (include/ptrace.h PT_OPT_GLARE) --------
    def glare(self, on=True):
        """Put the glare pyramid in place (or release it).  Off by default; scratch only: the image bits are the same either
        way, and resize and set_params refit it."""
        self._check(self.lib.pt_set_option(self._ctx, abi.PT_OPT_GLARE, 1 if on else 0))

    def glared_image(self, src=None, options=None):
        """(local_rows, width, 4) fp32: the LINEAR frame with its glare, a = 1 (pt_glare) — what meter(src=...) and
        toned_image(src=...) take next.  `options`: abi.PtGlareOptions (default: the header's).  `src`: None for the
        accumulation, or linear RGBA float32 texels (see _tone_src).  A numpy or no `src` gives a numpy array; a torch device
        tensor gives a torch device tensor."""
        opt = options if options is not None else abi.PtGlareOptions()
        return self._toned(self.lib.pt_glare, np.float32, opt, src)

    def glare_into(self, dst, src=None, options=None):
        """pt_glare into device memory of the caller's: `dst` is a ctypes.c_void_p to local_rows * width float4 texels, and may
        be a device `src`.  Synchronises."""
        opt = options if options is not None else abi.PtGlareOptions()
        ptr, keep = self._tone_src(src)
        if self.local_rows * self.width:
            self._check(self.lib.pt_glare(self._ctx, ptr, C.byref(opt), dst))
        del keep

    # -- temporal reprojection (include/ptrace.h PT_OPT_REPROJECT) ---------------------------------
    def reproject_option(self, on=True):
        """Allocate (or release) the history planes of temporal reprojection; needs feature_planes(True) first.  Off by
        default; the image bits of a context that never calls reproject() are the same either way."""
        self._check(self.lib.pt_set_option(self._ctx, abi.PT_OPT_REPROJECT, 1 if on else 0))

    def keep_history(self):
        """Remember the view in place (pt_keep_history): its ids and hit-point planes and the uniforms they were rendered
        with.  Needs a render_features() of that view.  Asynchronous."""
        self._check(self.lib.pt_keep_history(self._ctx))

    def load_history(self, prev, ids, point):
        """The same from host arrays (pt_load_history): `prev` the history view's PtParams, `ids` int32 and `point` float32,
        each (local_rows, width, 4)."""
        i = np.ascontiguousarray(ids, dtype=np.int32)
        p = np.ascontiguousarray(point, dtype=np.float32)
        shape = (self.local_rows, self.width, 4)
        if i.shape != shape or p.shape != shape:
            raise ValueError("history planes are %s and %s, this context holds %s" % (i.shape, p.shape, shape))
        q = prev.copy()
        self._check(self.lib.pt_load_history(self._ctx, C.byref(q), i.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p)))

    def reproject(self, options=None):
        """Carry the accumulation over from the history view into the view in place (pt_reproject): after set_params of the
        new view and render_features.  One-shot: it uses the history up.  `options`: abi.PtReprojectOptions (default: the
        header's caps and tolerance).  Asynchronous; the error estimate is cleared."""
        opt = options if options is not None else abi.PtReprojectOptions()
        self._check(self.lib.pt_reproject(self._ctx, C.byref(opt)))

    def reproject_estimate(self, options=None):
        """reproject() that carries the error estimate's state too (pt_reproject_estimate): the accumulation gets the bits
        reproject() would leave, the state is gathered from the same places instead of being cleared, so the filtered
        read-outs and error_stats() know of the history while the camera moves.  Needs error_estimate(True); the next fold
        must use the samples_per_pixel of the carried passes.  Good enough to steer a filter, no stopping criterion."""
        opt = options if options is not None else abi.PtReprojectOptions()
        self._check(self.lib.pt_reproject_estimate(self._ctx, C.byref(opt)))

    def reproject_stats(self):
        """abi.PtReprojectStats of the last reproject() or reproject_estimate(): pixels, pixels_hit, pixels_kept, samples_kept.  Synchronises."""
        st = abi.PtReprojectStats()
        self._check(self.lib.pt_reproject_stats(self._ctx, C.byref(st)))
        return st

    def sample_counts(self):
        """(local_rows, width) fp32: the samples each pixel holds (accum's fourth channel)."""
        return self.accum()[..., 3]

    def stats(self):
        st = abi.PtStats()
        self._check(self.lib.pt_get_stats(self._ctx, C.byref(st)))
        return st

    def probe(self, kind, inp, out_per_item, n):
        inp = np.ascontiguousarray(inp, dtype=np.float32)
        out = np.zeros(int(n) * out_per_item, dtype=np.float32)
        self._check(
            self.lib.pt_probe(self._ctx, int(kind), inp.ctypes.data_as(C.c_void_p), inp.size,
                              out.ctypes.data_as(C.c_void_p), out.size, int(n))
        )
        return out


_D2H, _H2D = 2, 1  # hipMemcpyDeviceToHost, hipMemcpyHostToDevice


class _DeviceView:
    """A device buffer the library owns, as PyTorch's array interface reads it (PathTracer.features under use_torch)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2,
                                         "strides": None}


def _memcpy(dst, src, nbytes, kind):
    """hipMemcpy of the HIP runtime this process already holds (the one serving libptrace.so, _lib.py): the raw error
    state is reached through its device pointer, like pt_accum_ptr's buffer."""
    hip = getattr(_memcpy, "hip", None)
    if hip is None:
        mapped = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln]
        hip = _memcpy.hip = C.CDLL(mapped[0] if mapped else "libamdhip64.so")
        hip.hipMemcpy.restype, hip.hipMemcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rc = hip.hipMemcpy(dst, src, nbytes, kind)
    if rc != 0:
        raise PtError(abi.PT_ERR_HIP, "hipMemcpy failed with %d" % rc)


def render_scene(scene, device=0, use_torch=False, passes_per_launch=None, band=None, geometry_path=None, tune=None, overlay=None, next_event=False):
    """Render a scenes.Scene completely; returns (PathTracer, accum ndarray).  `tune` = n: pt_tune(n) after scene and
    uniforms are up, as bench.py does before it times anything — the grid is refitted to the camera and PT_GEOM_AUTO
    settled with n-pass launches (the as-benchmarked path: tests that pin what the bench line times pass it).
    `overlay` = (selected_object, cursor_point): with the debug overlay on (set_debug_overlay).  `next_event`: with
    next-event estimation on (PathTracer.next_event)."""
    p = scene.params.copy()
    if band is not None:
        p.band_rows, p.band_index, p.band_count = band
    pt = PathTracer(p.width, p.height, device=device, use_torch=use_torch)
    if geometry_path is not None:
        pt.set_geometry_path(geometry_path)
    pt.set_spheres(scene.spheres)
    if overlay is not None:
        pt.set_debug_overlay(True, overlay[0], overlay[1])
    if next_event:
        pt.next_event(True)
    pt.set_params(p)
    per = passes_per_launch or scene.n_passes
    pt.reserve_passes(max(per, int(tune or 0)))
    if tune:
        pt.tune(int(tune))
    done = 0
    while done < scene.n_passes:
        k = min(per, scene.n_passes - done)
        q = p.copy()
        q.first_pass = scene.params.first_pass + done  # u_time = time + float(first_pass + p) * time_step
        pt.set_params(q)
        pt.render_passes(k)
        done += k
    return pt, pt.accum()
