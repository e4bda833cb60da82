"""A host-side model of ONE long-lived pt_ctx and the table of operations that drive it and the context side by side
(tests/test_context_model.py on the CPU, tests/test_gpu_context_sequences.py on the device).  TEST INFRASTRUCTURE ONLY.

The rule that makes a context predictable (include/ptrace.h): everything except scene, uniforms, size, roulette depth and the
debug overlay is scheduling only.  So the model is the oracle, an accumulation array, two textures and a canvas, and — while
the error estimate is on — the estimate's state as tests/error_ref.py keeps it.  What every call does to them is taken from the
header; the model shares no code with the library.

    Model            the state: spheres, PtParams (first_pass and the band fields included), size, roulette depth, overlay
                     triple, accumulation (local_rows x width x 4 float32, .a = spp), the segment tally since the last clear,
                     the two RGBA8 textures and the canvas, the estimate's state; and the few flags that decide whether a call
                     is REFUSED (count-work, reservation, estimate on, the estimate's samples per pass, the checkpoint's shape)
    OPS              name -> Op: `group` (CHANGE: configuration that must change the bits as the model says; KEEP:
                     configuration that must not change any bit; WORK), `variants`, and per step three functions:
                     plan(model, variant) -> the call's arguments, model(model, args) -> the predicted return code (the model
                     state follows the call), ctx(driver, args) -> the return code of the call made through PathTracer / lib
    Step             (operation name, variant); ("check", 0) compares context and model
    SEQUENCES        test name -> list of sequences, CONSTRUCTED (build_sequences): for the leading operation X of a test,
                     [X, Y, work, check] for every configuration operation Y, work rotating so that every configuration
                     operation stands directly before and directly after render_frames, render_adaptive, pt_tune and a
                     captured-and-replayed render_passes.  A dry model (no rendering) chooses the variants so that the work
                     of every triple is a call the header does not refuse; the documented refusals are a sequence of their own.

Two calls are modelled by what they did, not by what they will do: whether pt_tune launched anything (and therefore cleared) is
scheduling — the driver reports it from PtStats, the model's own guess (tune_launches) stands in the runs without a device.
pt_render_until / pt_render_adaptive run with the smallest positive target (0 is refused by the header: "a finite positive
target").  A frame with signal never reaches it, so they are `max_passes` plain passes with first_pass advanced; the model
still follows the header's loop to the letter, because two things do happen at these sizes: a frame WITHOUT signal (black
background, no light) has rel_error 0 by definition and is "reached" at its second pass, and a tile whose pixels see only
an absorbing or emitting sphere has a standard error of exactly 0 and falls idle — a partial round, folded into the active
tiles only (adaptive_ref), whose segments are the oracle's over those tiles' windows.
"""
import copy
import ctypes as C

import numpy as np

import adaptive_ref as A
import error_ref as E
import overlay_ref as R
from oracle import oracle
from ray_tracer_webgl_amd import abi, scenes
from test_gpu_fuzz import random_scene

OK, INVALID, CAPACITY = abi.PT_OK, abi.PT_ERR_INVALID, abi.PT_ERR_CAPACITY
SIZES = ((40, 24), (33, 19), (64, 36))   # 33 x 19: partial tiles on both edges
BANDS = ((8, 0, 1), (4, 1, 3), (3, 0, 2))   # (rows, index, count); count 1 = no partition
TARGET = float(np.finfo(np.float32).tiny)   # the smallest target the header accepts
CHANGE, KEEP, WORK = "change", "keep", "work"
STAT_FIELDS = ("n_spheres", "bvh_nodes", "bvh_slots", "grid_cells", "grid_kernel_build")


# ------------------------------------------------------------------------------------------------ scenes and uniforms
def _flat_field():
    """a ground and 129 small spheres standing on it: one layer of cells along y"""
    rng = np.random.default_rng(130)
    items = [scenes._sphere((0.0, -1000.0, 0.0), 1000.0, abi.PT_DIFFUSE, (0.5, 0.5, 0.5))]
    for k in range(129):
        x, z = (k % 13 - 6) * 0.55 + rng.uniform(-0.1, 0.1), (k // 13 - 5) * 0.55 + rng.uniform(-0.1, 0.1) - 1.0
        kind = (abi.PT_DIFFUSE, abi.PT_METAL, abi.PT_GLASS)[k % 3]
        items.append(scenes._sphere((x, 0.2, z), 0.2, kind, tuple(rng.uniform(0.2, 0.9, 3)), 0.1 * (k % 4), 1.5))
    return scenes._pack(items)


def _irregular():
    sp = random_scene(np.random.default_rng(31001), 40, 40, 24, 1, 4, 1).spheres.copy()
    sp["center"][17] = (2e15, 0.0, 0.0)   # no structure for this scene
    return sp


_scene_cache = {}
SCENES = ("three", "default", "random40", "flat130", "irregular")
HAS_GRID = {"three": False, "default": False, "random40": True, "flat130": True, "irregular": False}


def scene(name):
    if name not in _scene_cache:
        make = {"three": lambda: random_scene(np.random.default_rng(31003), 3, 40, 24, 1, 4, 1).spheres,
                "default": lambda: scenes.default_scene(40, 24, 1, 4).spheres,
                "random40": lambda: random_scene(np.random.default_rng(31001), 40, 40, 24, 1, 4, 1).spheres,
                "flat130": _flat_field, "irregular": _irregular}[name]
        _scene_cache[name] = make()
    return _scene_cache[name]


def camera(p, w, h, which):
    """the camera members of p for a w x h image: 0 the State's own, 1 a look-at camera with a lens"""
    lib = scenes._lib()
    if which == 0:
        scenes._state_camera(lib, p, w, h)
    else:
        scenes._look_at(lib, p, w, h, (2.5, 1.5, 3.0), (0.0, 0.2, -0.5), 50.0, 0.05, 3.5)
    p.width, p.height = w, h


def base_params(w, h):
    p = scenes._base_params(2, 4)
    camera(p, w, h, 0)
    p.time, p.time_step, p.first_pass = 100.0, 16.5, 0   # whole and half milliseconds: exact in fp32 (pt_render_frames)
    p.render_count, p.should_average, p.last_frame_weight = 1, 1, 1.0
    return p


def rows_of(p):
    return abi.local_rows(p.height, p.band_rows, p.band_index, p.band_count)


def band_of(p):
    """the partition as pt_set_params compares it: band_count <= 1 is "all rows" whatever the other two hold"""
    return (0, 0, 1) if p.band_count <= 1 or p.band_rows == 0 else (p.band_rows, p.band_index, p.band_count)


# ------------------------------------------------------------------------------------------------ renderers
class OracleRenderer:
    """the pass sums of passes first_pass ... first_pass + n - 1, each alone, and their segments"""
    dry = False

    def passes(self, spheres, p, n, roulette, overlay, window=None):
        out, seg = [], 0
        for k in range(n):
            q = p.copy()
            q.first_pass = p.first_pass + k
            if overlay is not None:
                acc, tally, _ = R.render(spheres, q, 1, overlay, window=window)
                s = tally["segments"]
            else:
                acc, s = oracle.render(spheres, q, 1, window=window, roulette=roulette)
            out.append(acc)
            seg += s
        return out, seg

    def blend(self, acc, p, prev):
        return oracle.blend_rgba8(acc, p.samples_per_pixel, p, prev)


class DryRenderer:
    """no rendering: black passes that carry their sample count — enough to follow every flag a refusal depends on"""
    dry = True

    def passes(self, spheres, p, n, roulette, overlay, window=None):
        s = np.zeros((rows_of(p), p.width, 4), np.float32)
        s[..., 3] = p.samples_per_pixel
        return [s] * n, 0

    def blend(self, acc, p, prev):
        return prev.copy()


# ------------------------------------------------------------------------------------------------ the model
class Model:
    def __init__(self, renderer, size=SIZES[0]):
        self.r = renderer
        self.w, self.h = size
        self.scene = None
        self.params = None
        self.cam = 0
        self.roulette = 0
        self.overlay = None
        self.segments = 0
        self.err_on, self.err, self.err_spp = False, None, 0
        # scheduling state: never in the bits, but refusals and the fresh context of a sequence's end depend on it
        self.policy, self.carry, self.refill, self.count_work, self.grid_fit = abi.PT_GEOM_AUTO, 12, 4, 0, 0
        self.reserved, self.side_stream, self.bound_pixels, self.captured, self.tuned = 1, False, 0, False, False
        self.checkpoint = None
        self.uneven = False   # pt_render_adaptive has run since the accumulation was last cleared or replaced
        self._shape(self.h)

    def _shape(self, rows):
        self.uneven = False
        self.accum = np.zeros((rows, self.w, 4), np.float32)
        self.tex = [np.zeros((rows, self.w, 4), np.uint8), np.zeros((rows, self.w, 4), np.uint8)]
        self.canvas = np.zeros((rows, self.w, 4), np.uint8)
        if self.err_on:
            self.err, self.err_spp = E.empty_state(rows, self.w), 0

    @property
    def rows(self):
        return self.accum.shape[0]

    @property
    def total_spp(self):
        return int(self.accum[0, 0, 3]) if self.accum.size else 0

    def clone(self):
        r, self.r = self.r, None
        m = copy.deepcopy(self)
        self.r = m.r = r
        return m

    # ---- clears -------------------------------------------------------------------------------------------------------
    def _clear_error(self):
        if self.err_on:
            self.err, self.err_spp = E.empty_state(self.rows, self.w), 0

    def reset(self):
        """pt_reset_accum: accumulation, sample count, statistics and the estimate; the textures stay"""
        self.accum[...] = 0
        self.segments, self.captured, self.uneven = 0, False, False
        self._clear_error()
        return OK

    def clear_textures(self):
        for a in (self.tex[0], self.tex[1], self.canvas):
            a[...] = 0
        return OK

    # ---- configuration that changes the bits ------------------------------------------------------------------------
    def set_spheres(self, name):
        self.scene, self.tuned = name, False
        return OK

    def set_params(self, p):
        """pt_set_params.  A changed row partition clears accumulation, sample count, estimate, textures and canvas and
        leaves the statistics counting; refused (PT_ERR_CAPACITY, nothing changed) when a bound buffer cannot hold the rows"""
        rows = rows_of(p)
        repartition = self.params is not None and (rows != self.rows or band_of(p) != band_of(self.params))
        if repartition and self.bound_pixels and rows * self.w > self.bound_pixels:
            return CAPACITY
        self.params = p.copy()
        if repartition:
            self._shape(rows)
            self.captured = False
        return OK

    def resize(self, w, h, p):
        """pt_resize + the pt_set_params it asks for: everything cleared, statistics included, a bound buffer given back"""
        self.w, self.h = w, h
        self.bound_pixels = 0
        self._shape(h)
        self.segments, self.captured = 0, False
        self.params = None
        return self.set_params(p)

    def set_roulette(self, k):
        if k > 0 and self.overlay is not None:
            return INVALID
        self.roulette = k
        return OK

    def set_overlay(self, ov):
        if ov is not None and self.roulette > 0:
            return INVALID
        self.overlay = ov
        return OK

    def load_accum(self, a):
        if a.shape != self.accum.shape or a[0, 0, 3] != a[-1, -1, 3]:   # (not an accumulation of whole passes: after a partial round)
            return INVALID
        self.accum = a.copy()
        self.captured, self.uneven = False, False
        self._clear_error()
        return OK

    # ---- configuration that changes no bit ----------------------------------------------------------------------------
    def set_estimate(self, on):
        if not on:
            self.err_on, self.err, self.err_spp = False, None, 0
        elif not self.err_on:
            self.err_on = True
            self._clear_error()
        return OK

    def reserve(self, n):
        self.reserved = max(self.reserved, n)   # the reservation only grows
        return OK

    def tune_launches(self):
        """the model's guess at whether pt_tune launches anything (the driver reports what it did)"""
        grid = HAS_GRID[self.scene] and not self.captured and self.grid_fit == 0
        return self.policy == abi.PT_GEOM_AUTO or (self.policy == abi.PT_GEOM_GRID and grid)

    def tune(self, n, launched):
        if launched and self.count_work and (self.roulette or self.overlay is not None):
            return INVALID   # its launches are refused like any
        if launched:
            self.reset()
        self.tuned = True
        return OK

    def bind(self, on):
        """pt_bind_accum: the caller's buffer (zeros here) or, with NULL, the own buffer, cleared; the estimate is cleared"""
        self.bound_pixels = self.rows * self.w if on else 0
        self.accum[...] = 0
        self.uneven = False
        self._clear_error()
        return OK

    # ---- work -----------------------------------------------------------------------------------------------------------
    def _launch_rc(self):
        return INVALID if self.count_work and (self.roulette or self.overlay is not None) else OK

    def passes_rc(self, n):
        if n > self.reserved:
            return CAPACITY
        if self.err_on and self.err_spp not in (0, self.params.samples_per_pixel):
            return INVALID
        return self._launch_rc()

    def render_passes(self, n, advance=False, active=None):
        """n passes; `active` (flags per 8x8 tile of the local rows, not all set): a partial round of pt_render_adaptive —
        folded into the pixels of the active tiles only, whose segments alone are counted"""
        rc = self.passes_rc(n)
        if rc != OK or self.rows == 0:
            return rc
        sums, seg = self.r.passes(scene(self.scene), self.params, n, self.roulette, self.overlay)
        if active is not None:
            self.err, self.accum = A.masked_fold(self.err, self.accum, sums, active)
            self.err_spp = self.params.samples_per_pixel
            seg = sum(self.r.passes(scene(self.scene), self.params, n, self.roulette, self.overlay, self._window(t))[1]
                      for t in np.flatnonzero(active))
        elif self.err_on:
            self.err, self.accum = E.fold(self.err, self.accum, sums)
            self.err_spp = self.params.samples_per_pixel
        else:
            for s in sums:
                self.accum = self.accum + s
        self.segments += seg
        if advance:
            self.params.first_pass += n
        return OK

    def _window(self, tile):
        """(x0, x1, y0, y1) in image coordinates around tile `tile` of the local rows: the owned rows inside are the tile's"""
        p = self.params
        tx = (self.w + 7) // 8

        def image_row(l):
            rows, index, count = band_of(p)
            return l if count <= 1 else ((l // rows) * count + index) * rows + l % rows

        x0, l0 = 8 * (tile % tx), 8 * (tile // tx)
        return x0, min(x0 + 8, self.w), image_row(l0), image_row(min(l0 + 8, self.rows) - 1) + 1

    def captured_passes(self, n):
        """n passes directly (the warm-up of the capture helper), then the same n captured and replayed once"""
        if self.count_work:
            return INVALID   # (the measuring twins allocate: not inside a capture.  The sequences never ask for it.)
        rc = self.render_passes(n)
        if rc == OK:
            rc = self.render_passes(n)
            self.captured = True
        return rc

    def render_to_target(self, k, max_passes, adaptive):
        if not self.err_on:
            return INVALID
        if k > self.reserved:
            return CAPACITY
        if adaptive and self.count_work:
            return INVALID
        if adaptive and self.err_spp not in (0, self.params.samples_per_pixel):
            return INVALID
        def reached():
            s = E.stats(self.err)
            return s["rel_error"] <= TARGET and s["pixels_short"] == 0

        done = 0
        active = None
        self.uneven = self.uneven or adaptive
        if adaptive and not self.r.dry:   # the look at the state the call finds
            active = A.select(self.err, TARGET)
            if reached() or not active.any():
                return OK
        while done < max_passes:
            n = min(k, max_passes - done)
            rc = self.render_passes(n, advance=True, active=None if active is None or active.all() else active)
            if rc != OK:
                return rc
            done += n
            if self.r.dry:
                continue
            if reached():   # (a frame without signal: rel_error is 0 by definition)
                break
            if adaptive:
                active = A.select(self.err, TARGET)
                if not active.any():
                    break
        return OK

    def frames(self, e0, max_rc, n):
        if self.count_work:
            return INVALID
        rc = self._launch_rc()
        if rc != OK or self.rows == 0:
            return rc
        p = self.params
        for k in range(n):
            q = p.copy()
            q.first_pass = p.first_pass + k
            q.render_count = min(p.render_count + k, max_rc)
            (acc,), seg = self.r.passes(scene(self.scene), q, 1, self.roulette, self.overlay)
            self.segments += seg
            self.canvas = self.r.blend(acc, q, self.tex[(e0 + k + 1) % 2])
            if q.should_average:
                self.tex[(e0 + k) % 2] = self.canvas.copy()
        return OK

    def write_texture(self, index, a):
        self.tex[index] = a.copy()
        return OK


# ------------------------------------------------------------------------------------------------ the driver (device side)
class Driver:
    """One PathTracer and what the calls need beside it: two torch streams, the bound tensor, the last checkpoint."""

    def __init__(self, size):
        import torch
        from ray_tracer_webgl_amd.tracer import PathTracer, PtError

        self.torch, self.PtError = torch, PtError
        self.t = PathTracer(*size)
        self.lib, self.ctx = self.t.lib, self.t._ctx
        self.side, self.cap = torch.cuda.Stream(), torch.cuda.Stream()
        self.on_side = False
        self.tensor = None

    def close(self):
        self.t.close()

    def call(self, fn, *a):
        try:
            fn(*a)
            return OK
        except self.PtError as e:
            return e.code

    def stream_handle(self):
        return C.c_void_p(self.side.cuda_stream) if self.on_side else None

    def set_params(self, p):
        return self.call(self.t.set_params, p)

    def resize(self, w, h, p):
        rc = self.lib.pt_resize(self.ctx, w, h)
        if rc != OK:
            return rc
        self.t.width, self.t.height, self.t.local_rows, self.tensor = w, h, h, None
        return self.set_params(p)

    def load_accum(self, a):
        a = np.ascontiguousarray(a, np.float32)
        return self.lib.pt_load_accum(self.ctx, a.ctypes.data_as(C.c_void_p), a.nbytes)

    def set_stream(self, side):
        self.on_side = side
        return self.lib.pt_set_stream(self.ctx, self.stream_handle())

    def bind(self, on):
        if not on:
            rc = self.lib.pt_bind_accum(self.ctx, None, 0)
            self.tensor = None
            return rc
        self.t.synchronize()
        tensor = self.torch.zeros((max(self.t.local_rows, 1), self.t.width, 4), dtype=self.torch.float32, device="cuda")
        self.torch.cuda.synchronize()
        rc = self.lib.pt_bind_accum(self.ctx, C.c_void_p(tensor.data_ptr()), tensor.numel() * 4)
        self.tensor = tensor   # (the one before stays alive until the context has let go of it)
        return rc

    def tune(self, n):
        """(return code, did it clear?) — whether pt_tune launched is read off the statistics it clears when it did"""
        before = self.t.stats()
        rc = self.lib.pt_tune(self.ctx, n)
        after = self.t.stats()
        had = before.render_launches or before.segments or before.total_spp
        return rc, bool(had and not (after.render_launches or after.segments or after.total_spp)) if had else None

    def captured_passes(self, n):
        """the capture helper of test_render_is_hip_graph_capturable: a warm-up outside the capture, the same launch captured
        on a torch side stream, one replay"""
        torch = self.torch
        rc = self.lib.pt_render_passes(self.ctx, n)
        if rc != OK:
            return rc
        self.t.stats()   # (synchronises and lets PT_GEOM_AUTO settle: nothing is left to ask of the device inside the capture)
        assert self.lib.pt_set_stream(self.ctx, C.c_void_p(self.cap.cuda_stream)) == OK
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=self.cap):
            rc = self.lib.pt_render_passes(self.ctx, n)
        assert rc == OK, "a launch the warm-up accepted was refused inside the capture: %d %s" % (rc, self.lib.pt_last_error(self.ctx))
        g.replay()
        torch.cuda.synchronize()
        assert self.lib.pt_set_stream(self.ctx, self.stream_handle()) == OK
        return rc

    def frames_on_legacy(self, e0, max_rc, n):
        assert self.lib.pt_set_stream(self.ctx, C.c_void_p(abi.PT_STREAM_LEGACY)) == OK
        rc = self.lib.pt_render_frames(self.ctx, e0, max_rc, n)
        assert self.lib.pt_set_stream(self.ctx, self.stream_handle()) == OK
        return rc


# ------------------------------------------------------------------------------------------------ the operations
class Op:
    def __init__(self, group, variants, plan, model, ctx):
        self.group, self.variants, self.plan, self.model, self.ctx = group, variants, plan, model, ctx


def _new_params(m, v):
    """set_params variant v on the model's uniforms"""
    p = m.params.copy()
    if v == 0:
        m_cam = 1 - m.cam
        camera(p, m.w, m.h, m_cam)
        return p, m_cam
    if v == 1:
        p.time, p.time_step = (7.5, 0.5) if p.time == 100.0 else (100.0, 16.5)
    elif v == 2:
        p.first_pass = p.first_pass + 3
    elif v == 3:
        p.samples_per_pixel = p.samples_per_pixel % 3 + 1
    elif v == 4:
        p.max_depth = {1: 4, 4: 8, 8: 1}[p.max_depth]
    elif v == 5:
        p.background_mode = abi.PT_BG_BLACK if p.background_mode == abi.PT_BG_SKY else abi.PT_BG_SKY
    else:
        p.should_average, p.render_count, p.last_frame_weight = {(1, 1): (1, 3, 0.5), (1, 3): (0, 2, 1.0), (0, 2): (1, 1, 1.0)}[
            (p.should_average, p.render_count)]
    return p, m.cam


def _m_set_params(m, a):
    rc = m.set_params(a[0])
    if rc == OK:
        m.cam = a[1]
    return rc


def _band_params(m, v):
    p = m.params.copy()
    p.band_rows, p.band_index, p.band_count = BANDS[v]
    return p


def _resize_args(m, v):
    w, h = SIZES[v]
    p = m.params.copy()
    camera(p, w, h, m.cam)
    p.band_rows, p.band_index, p.band_count = BANDS[0]
    return w, h, p


OVERLAYS = (None, (1, (0.0, 0.0, -0.5)), (abi.NO_SELECTED_OBJECT_ID, (0.3, 0.1, -0.6)))


def _d_overlay(d, ov):
    return d.call(d.t.set_debug_overlay, False) if ov is None else d.call(d.t.set_debug_overlay, True, ov[0], ov[1])


def _m_tune(m, n, observed=None):
    return m.tune(n, m.tune_launches() if observed is None else observed)


def _texture_args(m, v):
    a = np.random.default_rng(500 + v).integers(0, 256, (m.rows, m.w, 4), dtype=np.uint8)
    a[..., 3] = 255
    return v, a


def _option(key):
    return lambda d, a: d.lib.pt_set_option(d.ctx, key, int(a))


def _const(variants):
    return lambda m, v: variants[v]


def _set(field):
    def f(m, a):
        setattr(m, field, a)
        return OK
    return f


OPT_GEOMETRY_PATH, OPT_COUNT_WORK, OPT_CARRY_LANES, OPT_REFILL_MIN, OPT_ROULETTE, OPT_GRID_FIT = 1, 2, 3, 4, 5, 6
PATHS = (abi.PT_GEOM_AUTO, 1, 2, 3, 4, 5)   # PT_GEOM_LDS, _SCALAR, _BVH, _GRID, _SMALL

OPS = {
    # ---- configuration that must change the bits as the model says
    "set_spheres": Op(CHANGE, len(SCENES), _const(SCENES), Model.set_spheres, lambda d, a: d.call(d.t.set_spheres, scene(a))),
    "set_params": Op(CHANGE, 7, _new_params, _m_set_params, lambda d, a: d.set_params(a[0])),
    "set_band": Op(CHANGE, len(BANDS), _band_params, Model.set_params, lambda d, a: d.set_params(a)),
    "resize": Op(CHANGE, len(SIZES), _resize_args, lambda m, a: m.resize(*a), lambda d, a: d.resize(*a)),
    "set_russian_roulette": Op(CHANGE, 3, _const((0, 1, 3)), Model.set_roulette, _option(OPT_ROULETTE)),
    "set_debug_overlay": Op(CHANGE, len(OVERLAYS), _const(OVERLAYS), Model.set_overlay, _d_overlay),
    "reset": Op(CHANGE, 1, _const((None,)), lambda m, a: m.reset(), lambda d, a: d.call(d.t.reset)),
    # variant 0: the last checkpoint (refused with PT_ERR_INVALID when the size has changed since); 1: one of a wrong size
    "load_accum": Op(CHANGE, 2, lambda m, v: m.checkpoint if v == 0 else np.zeros((m.rows + 1, m.w, 4), np.float32),
                     Model.load_accum, lambda d, a: d.load_accum(a)),
    # ---- configuration that must not change any bit
    "set_geometry_path": Op(KEEP, len(PATHS), _const(PATHS), _set("policy"), _option(OPT_GEOMETRY_PATH)),
    "set_carry_lanes": Op(KEEP, 3, _const((0, 12, 40)), _set("carry"), _option(OPT_CARRY_LANES)),
    "set_refill_min": Op(KEEP, 3, _const((1, 4, 64)), _set("refill"), _option(OPT_REFILL_MIN)),
    "set_count_work": Op(KEEP, 2, _const((0, 1)), _set("count_work"), _option(OPT_COUNT_WORK)),
    "set_grid_fit": Op(KEEP, 2, _const((0, 1)), _set("grid_fit"), _option(OPT_GRID_FIT)),
    "tune": Op(KEEP, 2, lambda m, v: min(v + 1, m.reserved), _m_tune, lambda d, a: d.tune(a)),
    "refit_grid": Op(KEEP, 2, _const((0, 1)), lambda m, a: (setattr(m, "tuned", True), OK)[1],
                     lambda d, a: d.lib.pt_refit_grid(d.ctx, a)),
    "reserve_passes": Op(KEEP, 3, _const((3, 1, 4)), Model.reserve, lambda d, a: d.lib.pt_reserve_passes(d.ctx, a)),
    "error_estimate": Op(KEEP, 2, _const((True, False)), Model.set_estimate, lambda d, a: d.call(d.t.error_estimate, a)),
    "set_stream": Op(KEEP, 2, _const((True, False)), _set("side_stream"), lambda d, a: d.set_stream(a)),
    "bind_accum": Op(KEEP, 2, _const((True, False)), Model.bind, lambda d, a: d.bind(a)),
    # ---- work
    "render": Op(WORK, 1, _const((1,)), Model.render_passes, lambda d, a: d.lib.pt_render(d.ctx)),
    # variant 3: one pass more than was ever reserved — refused with PT_ERR_CAPACITY
    "render_passes": Op(WORK, 4, lambda m, v: v + 1 if v < 3 else m.reserved + 1, Model.render_passes,
                        lambda d, a: d.lib.pt_render_passes(d.ctx, a)),
    "render_until": Op(WORK, 2, _const(((1, 2), (2, 3))), lambda m, a: m.render_to_target(a[0], a[1], False),
                       lambda d, a: d.call(d.t.render_until, TARGET, a[0], a[1])),
    "render_adaptive": Op(WORK, 2, _const(((1, 2), (2, 3))), lambda m, a: m.render_to_target(a[0], a[1], True),
                          lambda d, a: d.call(d.t.render_adaptive, TARGET, a[0], a[1])),
    "render_frame": Op(WORK, 2, _const((0, 1)), lambda m, a: m.frames(a, 0x7fffffff, 1), lambda d, a: d.lib.pt_render_frame(d.ctx, a)),
    "render_frames": Op(WORK, 3, _const(((1, 4, 1), (0, 4, 5), (1, 100000, 20))), lambda m, a: m.frames(*a),
                        lambda d, a: d.lib.pt_render_frames(d.ctx, *a)),
    "clear_textures": Op(WORK, 1, _const((None,)), lambda m, a: m.clear_textures(), lambda d, a: d.lib.pt_clear_textures(d.ctx)),
    "write_texture": Op(WORK, 2, _texture_args, lambda m, a: m.write_texture(*a), lambda d, a: d.call(d.t.write_texture, *a)),
    "captured_passes": Op(WORK, 2, _const((1, 2)), Model.captured_passes, lambda d, a: d.captured_passes(a)),
    # pt_render_frames on PT_STREAM_LEGACY: refused with PT_ERR_INVALID (the stream is put back afterwards)
    "frames_on_legacy": Op(WORK, 1, _const(((0, 4, 5),)), lambda m, a: INVALID, lambda d, a: d.frames_on_legacy(*a)),
}
CONFIG = [k for k, o in OPS.items() if o.group in (CHANGE, KEEP)]
WORKS = ["render_frames", "render_adaptive", "captured_passes", "render_passes", "render_until", "render_frame", "render",
         "write_texture", "clear_textures"]
NEIGHBOURS = ("render_frames", "render_adaptive", "captured_passes", "tune")   # every configuration operation stands next to these
CHECK = ("check", 0)


def apply_model(m, step, observed=None):
    """one step on the model: (arguments, predicted return code)"""
    name, v = step
    op = OPS[name]
    args = op.plan(m, v)
    rc = _m_tune(m, args, observed) if name == "tune" else op.model(m, args)
    return args, rc


def checkpoint(m):
    """what every check step does besides comparing: the accumulation as a checkpoint for a later load_accum — unless
    pt_render_adaptive has run since the last clear: after a partial round the pixels hold different numbers of passes, and
    such a buffer is no checkpoint (pt_load_accum refuses it)"""
    if not m.uneven:
        m.checkpoint = m.accum.copy()


PROLOGUE = [("set_spheres", 1), ("set_band", 0), ("reserve_passes", 0), ("error_estimate", 0), CHECK]


def start(renderer, size=SIZES[0]):
    """a model as every sequence finds it: created at `size`, the first uniforms in place (a context takes them with its
    first pt_set_params; the PROLOGUE's set_band re-sends them)"""
    m = Model(renderer, size)
    m.params = base_params(*size)
    return m


def run_model(seq, renderer):
    """a sequence on the model alone: the return code of every step"""
    m = start(renderer)
    out = []
    for step in seq:
        if step == CHECK:
            checkpoint(m)
            out.append(OK)
        else:
            out.append(apply_model(m, step)[1])
    return m, out


# ------------------------------------------------------------------------------------------------ the sequences
FIXERS = [[("reset", 0)], [("set_count_work", 0)], [("error_estimate", 0)], [("set_debug_overlay", 0)], [("set_russian_roulette", 0)],
          [("reserve_passes", 0)], [("bind_accum", 1)], [("reset", 0), ("render", 0), CHECK]]   # (the last: a fresh checkpoint)


def _try(m, steps):
    """the steps on a clone of the dry model: the clone when every call is accepted, else None"""
    c = m.clone()
    for s in steps:
        if s == CHECK:
            checkpoint(c)
        elif s[0] == "load_accum" and (s[1] != 0 or c.checkpoint is None):
            return None
        elif apply_model(c, s)[1] != OK:
            return None
    return c


def _rot(name, turn):
    n = OPS[name].variants
    if name == "render_passes":
        n = 3   # (the fourth is the refusal)
    if name == "load_accum":
        n = 1
    return [(name, (turn + k) % n) for k in range(n)]


def build_sequences():
    """test name -> sequences.  For the leading operation X (test `X`), two sequences cover [X, Y, work, check] for every
    configuration operation Y; triple (X, Y) uses WORKS[(index of X + index of Y) % 9], so that over the tests every Y
    meets every kind of work, and inside a test X follows every kind of work.  Variants rotate per operation; a dry
    model picks the first combination whose three calls are accepted, inserting a fixer (FIXERS) in front of X where none is."""
    turn = dict.fromkeys(OPS, 0)
    out = {}
    for ix, x in enumerate(CONFIG):
        seqs = []
        for chunk in (range(0, 10), range(10, len(CONFIG))):
            m = start(DryRenderer())
            seq = list(PROLOGUE)
            m = _try(m, seq)
            assert m is not None
            for iy in chunk:
                y, w = CONFIG[iy], WORKS[(ix + iy) % len(WORKS)]
                found = None
                for fix in [[]] + FIXERS + [f + g for f in FIXERS for g in FIXERS if f != g]:
                    for sx in _rot(x, turn[x]):
                        for sy in _rot(y, turn[y] + (1 if x == y else 0)):
                            for sw in _rot(w, turn[w]):
                                steps = fix + [sx, sy, sw, CHECK]
                                c = _try(m, steps)
                                if c is not None:
                                    found = (steps, c)
                                    break
                            if found:
                                break
                        if found:
                            break
                    if found:
                        break
                assert found, (x, y, w)
                steps, m = found
                for s in steps:
                    if s != CHECK:
                        turn[s[0]] += 1
                seq += steps
            seqs.append(seq)
        out[x] = seqs
    out["refusals"] = [REFUSALS]
    return out


# The documented refusals, each with the code the header names; a refused call leaves the context as it was, which the check
# after it shows.  ("roulette switched off after the overlay was refused" is steps 2-4.)
REFUSALS = PROLOGUE + [
    ("set_russian_roulette", 2), ("set_debug_overlay", 1), ("set_russian_roulette", 0), ("render_passes", 1), CHECK,
    ("set_debug_overlay", 1), ("set_russian_roulette", 1), ("set_debug_overlay", 0), ("render_frames", 1), CHECK,
    ("set_count_work", 1), ("set_debug_overlay", 2), ("render_passes", 0), ("render_frames", 0), ("set_debug_overlay", 0), CHECK,
    ("set_russian_roulette", 1), ("render", 0), ("render_until", 0), ("set_russian_roulette", 0), ("render", 0), CHECK,
    ("render_adaptive", 0), ("set_count_work", 0), ("render_passes", 3), ("render_adaptive", 0), CHECK,
    ("resize", 1), ("load_accum", 0), ("load_accum", 1), ("render", 0), CHECK,
    ("frames_on_legacy", 0), ("error_estimate", 1), ("render_until", 0), ("render_frames", 1), CHECK,
]

def _refused_codes():
    codes = [None] * len(REFUSALS)
    expect = [INVALID,   # the overlay while roulette is on
              INVALID,   # roulette while the overlay is on
              INVALID, INVALID,   # a launch / a frame with the overlay and count-work on
              INVALID, INVALID,   # a launch / render_until with roulette and count-work on
              INVALID,   # render_adaptive with count-work on
              CAPACITY,  # render_passes beyond the reservation
              INVALID, INVALID,   # load_accum of a checkpoint taken at another size, and of a wrong size outright
              INVALID,   # frames on PT_STREAM_LEGACY
              INVALID]   # render_until without the estimate
    at = [len(PROLOGUE) + k for k in (1, 6, 12, 13, 17, 18, 22, 24, 28, 29, 32, 34)]
    for i, code in zip(at, expect):
        codes[i] = code
    return codes


REFUSED = _refused_codes()   # per step of REFUSALS: the code the call must return, None where it must be accepted
SEQUENCES = build_sequences()
