"""Temporal reprojection (PT_OPT_REPROJECT, pt_keep_history / pt_load_history / pt_reproject / pt_reproject_stats;
include/ptrace.h has the contract) on the device, bit for bit against tests/reproject_ref.py.

The planes a comparison starts from are read back with pt_read_features (their own correctness is test_gpu_features.py's
business), accumulations go in through pt_load_accum (equal whole counts at both ends, anything between) or a bound buffer,
hand-made current planes are written through pt_features_ptr after a pt_render_features, hand-made history goes in through
pt_load_history.  Tolerance: none (NaN compares equal to NaN).

  (a) sizes          1x1, 3x2, 31x7, 33x9 and 37x21: partial 32x8 workgroups, one to several of them
  (b) operands       a 131x13 hand-made frame with every operand class of the contract, at four settings
  (c) bands          74x26 in bands of 4 rows over 3 ranks
  (d) a flight       two moves at 200x120 through pt_keep_history, compared with the restatement after each move
  (e) a bound buffer keeps its address; (f) nothing else of the context moves; (g) every PT_ERR_* path and every way the
  history ends; (h) FrameLoop with and without `reproject`
"""
import ctypes as C

import numpy as np
import pytest

import error_ref as ER
import reproject_ref as RR
from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd.tracer import PathTracer, _H2D, _memcpy

pytestmark = pytest.mark.gpu

CAPS, TOL = (32.0, 8.0), 2.0


def options(caps=CAPS, tol=TOL):
    return abi.PtReprojectOptions(caps[0], caps[1], tol)


def context(sph, p, estimate=False, use_torch=False):
    t = PathTracer(p.width, p.height, use_torch=use_torch)
    t.set_spheres(sph)
    t.feature_planes(True)
    t.reproject_option(True)
    if estimate:
        t.error_estimate(True)
    t.set_params(p)
    return t


def write_current_planes(t, ids, pnt):
    """hand-made current planes: over the planes a pt_render_features has just declared valid"""
    t.render_features()
    t.synchronize()
    for plane, a in ((abi.PT_FEAT_IDS, np.ascontiguousarray(ids, np.int32)), (abi.PT_FEAT_POINT, np.ascontiguousarray(pnt, np.float32))):
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        t._check(t.lib.pt_features_ptr(t._ctx, plane, C.byref(ptr), C.byref(nbytes)))
        assert nbytes.value == a.nbytes
        if a.nbytes:
            _memcpy(ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, _H2D)


def checkpoint(acc):
    """an accumulation pt_load_accum accepts: equal whole counts at both ends, anything between"""
    acc = np.array(acc, np.float32)
    acc[0, 0] = (1.5, 0.25, 3.0, 3.0)
    acc[-1, -1] = (0.5, 2.25, 1.0, 3.0)
    return acc


def assert_reprojected(t, ref, what):
    out, tallies = ref
    got = t.accum()
    assert RR.same_floats(got, out), "%s: %s" % (what, RR.first_difference(got, out))
    st = t.reproject_stats()
    assert {k: int(getattr(st, k)) for k in tallies} == tallies, what
    assert t.stats().total_spp == int(out[0, 0, 3])   # pixel (0, 0)'s count, as after a partial adaptive round


# ---------------------------------------------------------------------------------------------------- (a) sizes
@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (31, 7), (33, 9), (37, 21)])
def test_partial_workgroups(w, h):
    sph, p0 = ER.estimate_scene(w, h)
    p1 = RR.flight_params(p0, 2)
    t = context(sph, p0)
    try:
        t.render_features()
        hist = t.features()
        t.keep_history()
        t.reserve_passes(2)
        t.render_passes(2)
        acc = t.accum()
        t.set_params(p1)
        t.render_features()
        cur = t.features()
        t.reproject(options())
        ref = RR.reproject(cur["ids"], cur["point"], hist["ids"], hist["point"], acc, p0, p1, CAPS[0], CAPS[1], TOL)
        assert_reprojected(t, ref, "%dx%d" % (w, h))
        if w * h >= 200:
            assert ref[1]["pixels_kept"] > 0
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------- (b) operands
@pytest.fixture(scope="module")
def hand():
    sph, p = ER.estimate_scene(131, 13)
    f = RR.hand_frame(p)
    f["acc"] = checkpoint(f["acc"])
    return sph, p, f


def test_every_operand_class(hand):
    sph, p, f = hand
    t = context(sph, p)
    try:
        for caps, tol in ((CAPS, TOL), ((16777215.0, 0.0), 1000.0), ((0.0, 3.0), 0.0), ((1.0, 1.0), 0.5)):
            write_current_planes(t, f["cur_ids"], f["cur_pnt"])
            t.load_history(p, f["hist_ids"], f["hist_pnt"])
            t.load_accum(f["acc"])
            t.reproject(options(caps, tol))
            ref = RR.reproject(f["cur_ids"], f["cur_pnt"], f["hist_ids"], f["hist_pnt"], f["acc"], p, p, caps[0], caps[1], tol)
            assert_reprojected(t, ref, "hand-made frame, caps %s tolerance %s" % (caps, tol))
        out = t.accum()
        assert np.all(out[..., 3] == np.floor(out[..., 3]))
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------- (c) bands
def test_bands_of_four_rows_over_three_ranks():
    sph, p = ER.estimate_scene(74, 26)
    f = RR.hand_frame(p, seed=11)
    for r in range(3):
        q = p.copy()
        q.band_rows, q.band_index, q.band_count = 4, r, 3
        ys = abi.owned_rows(26, 4, r, 3)
        g = {k: v[ys] for k, v in f.items()}
        g["acc"] = checkpoint(g["acc"])
        t = context(sph, q)
        try:
            assert t.local_rows == len(ys)
            write_current_planes(t, g["cur_ids"], g["cur_pnt"])
            t.load_history(q, g["hist_ids"], g["hist_pnt"])
            t.load_accum(g["acc"])
            t.reproject(options())
            ref = RR.reproject(g["cur_ids"], g["cur_pnt"], g["hist_ids"], g["hist_pnt"], g["acc"], q, q, CAPS[0], CAPS[1], TOL)
            assert_reprojected(t, ref, "band %d of 3" % r)
            assert ref[1]["pixels_kept"] > 100
        finally:
            t.close()


# ---------------------------------------------------------------------------------------------------- (d) a flight
def test_a_two_move_flight_through_keep_history():
    sph, p0 = ER.estimate_scene(200, 120)
    t = context(sph, p0)
    try:
        t.render_features()
        planes = t.features()
        t.render_passes(1)
        prev = p0
        for k in (1, 2):
            p = RR.flight_params(p0, k)
            acc = t.accum()
            t.keep_history()             # the tick of include/ptrace.h
            t.set_params(p)
            t.render_features()
            t.reproject(options())
            cur = t.features()
            ref = RR.reproject(cur["ids"], cur["point"], planes["ids"], planes["point"], acc, prev, p, CAPS[0], CAPS[1], TOL)
            assert_reprojected(t, ref, "move %d" % k)
            assert 0.55 < ref[1]["pixels_kept"] / ref[1]["pixels"] < 0.70
            t.render_passes(1)
            counts = t.sample_counts()
            assert np.array_equal(counts, ref[0][..., 3] + 4)   # every pixel: what it kept + the fresh pass
            planes, prev = cur, p
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------- (e) a bound buffer
def test_a_caller_bound_accumulation_keeps_its_address(hand):
    import torch

    sph, p, f = hand
    t = context(sph, p, use_torch=True)
    try:
        addr = t.accum_tensor.data_ptr()
        write_current_planes(t, f["cur_ids"], f["cur_pnt"])
        t.load_history(p, f["hist_ids"], f["hist_pnt"])
        t.accum_tensor.copy_(torch.from_numpy(f["acc"]))
        torch.cuda.synchronize()
        t.reproject(options())
        ref = RR.reproject(f["cur_ids"], f["cur_pnt"], f["hist_ids"], f["hist_pnt"], f["acc"], p, p, CAPS[0], CAPS[1], TOL)
        assert_reprojected(t, ref, "bound buffer")
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        t._check(t.lib.pt_accum_ptr(t._ctx, C.byref(ptr), C.byref(nbytes)))
        assert ptr.value == addr == t.accum_tensor.data_ptr() and nbytes.value == f["acc"].nbytes
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------- (f) nothing else moves
def test_nothing_else_of_the_context_moves(ora):
    sph, p0 = ER.estimate_scene(37, 21)
    p1 = RR.flight_params(p0, 1)
    t = context(sph, p0, estimate=True)
    try:
        t.reserve_passes(2)
        t.render_until(1e-9, 2, 4)        # four passes: first_pass stands at 4, the estimate knows them
        assert t.error_state().any()
        t.render_frame(0)
        tex, canvas = [t.read_texture(0), t.read_texture(1)], t.read_canvas()
        t.render_features()
        t.keep_history()
        q = p1.copy()
        q.first_pass = 4
        t.set_params(q)
        t.render_features()
        before = t.stats()
        t.reproject(options())
        after = t.stats()
        assert t.reproject_stats().pixels_kept > 0
        assert not t.error_state().any()                       # cleared, as pt_load_accum clears it
        for k in ("segments", "samples", "render_launches", "far_rays"):
            assert getattr(after, k) == getattr(before, k), k
        assert np.array_equal(t.read_texture(0), tex[0]) and np.array_equal(t.read_texture(1), tex[1])
        assert np.array_equal(t.read_canvas(), canvas)
        # first_pass: after a reprojection that keeps nothing, the next pass IS pass 4 of the new view
        t.keep_history()
        t.set_params(q)
        t.render_features()
        t.reproject(options((0.0, 0.0)))
        assert not t.accum().any() and t.reproject_stats().pixels_kept == 0
        t.render_passes(1)
        ref, _ = ora.render(sph, q, 1)
        assert t.accum().tobytes() == ref.tobytes()
    finally:
        t.close()


def test_a_context_that_never_reprojects_keeps_its_bits(ora):
    sph, p = ER.estimate_scene(37, 21)
    t = context(sph, p)
    try:
        t.render_features()
        t.keep_history()
        t.render_passes(1)
        assert t.accum().tobytes() == ora.render(sph, p, 1)[0].tobytes()
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------- (g) errors, validity
def rc_reproject(t, opt=None):
    o = opt if opt is not None else options()
    return t.lib.pt_reproject(t._ctx, C.byref(o))


def test_error_codes():
    sph, p = ER.estimate_scene(33, 9)
    t = PathTracer(33, 9)
    lib = t.lib
    try:
        t.set_spheres(sph)
        t.set_params(p)
        assert lib.pt_set_option(t._ctx, abi.PT_OPT_REPROJECT, 1) == abi.PT_ERR_INVALID     # needs the feature planes
        assert lib.pt_set_option(t._ctx, abi.PT_OPT_REPROJECT, 2) == abi.PT_ERR_INVALID
        st = abi.PtReprojectStats()
        planes = np.zeros((9, 33, 4), np.float32)
        vp = planes.ctypes.data_as(C.c_void_p)
        for rc in (lib.pt_keep_history(t._ctx), rc_reproject(t), lib.pt_reproject_stats(t._ctx, C.byref(st)),
                   lib.pt_load_history(t._ctx, C.byref(p), vp, vp)):
            assert rc == abi.PT_ERR_NOT_READY                                                # the option is off
        t.feature_planes(True)
        t.reproject_option(True)
        t.reproject_option(True)                                                             # (again: a no-op)
        assert lib.pt_keep_history(t._ctx) == abi.PT_ERR_NOT_READY                           # no planes rendered yet
        assert lib.pt_reproject_stats(t._ctx, C.byref(st)) == abi.PT_ERR_NOT_READY           # no pt_reproject yet
        t.render_features()
        assert rc_reproject(t) == abi.PT_ERR_NOT_READY                                       # no history
        t.keep_history()
        assert lib.pt_reproject(t._ctx, None) == abi.PT_ERR_INVALID
        assert lib.pt_reproject_stats(t._ctx, None) == abi.PT_ERR_INVALID
        for caps, tol in (((-1.0, 8.0), 2.0), ((32.0, 2.5), 2.0), ((16777216.0, 8.0), 2.0), ((float("nan"), 8.0), 2.0),
                          ((32.0, float("inf")), 2.0), (CAPS, -0.5), (CAPS, float("nan")), (CAPS, float("inf"))):
            assert rc_reproject(t, options(caps, tol)) == abi.PT_ERR_INVALID, (caps, tol)
        assert rc_reproject(t) == abi.PT_OK                                                  # ... and none of them used the history up
        assert rc_reproject(t) == abi.PT_ERR_NOT_READY                                       # one-shot
        assert lib.pt_reproject_stats(t._ctx, C.byref(st)) == abi.PT_OK and st.pixels == 33 * 9
        # pt_load_history: NULL arguments, another size, another partition
        for args in ((None, vp, vp), (C.byref(p), None, vp), (C.byref(p), vp, None)):
            assert lib.pt_load_history(t._ctx, *args) == abi.PT_ERR_INVALID
        q = p.copy()
        q.width = 34
        assert lib.pt_load_history(t._ctx, C.byref(q), vp, vp) == abi.PT_ERR_INVALID
        q = p.copy()
        q.band_rows, q.band_index, q.band_count = 4, 0, 2
        assert lib.pt_load_history(t._ctx, C.byref(q), vp, vp) == abi.PT_ERR_INVALID
        # a history whose camera is degenerate is refused when it is used
        q = p.copy()
        q.horizontal = abi.f3(0.0, 0.0, 0.0)
        assert lib.pt_load_history(t._ctx, C.byref(q), vp, vp) == abi.PT_OK
        assert rc_reproject(t) == abi.PT_ERR_INVALID and b"degenerate" in lib.pt_last_error(t._ctx)
        # current planes must be rendered after the pt_set_params of the new view
        t.keep_history()
        t.set_params(p)
        assert rc_reproject(t) == abi.PT_ERR_NOT_READY
        t.render_features()
        assert rc_reproject(t) == abi.PT_OK
    finally:
        t.close()


def test_every_way_the_history_ends():
    sph, p = ER.estimate_scene(33, 9)
    t = context(sph, p)
    try:
        def history():
            t.set_params(p)
            t.render_features()
            t.keep_history()

        def ready():
            """would pt_reproject run?  (asked with fresh current planes, so only the history can be missing)"""
            t.render_features()
            return rc_reproject(t)

        history()
        t.set_params(RR.flight_params(p, 1))             # an ordinary pt_set_params does NOT end it
        assert ready() == abi.PT_OK
        assert ready() == abi.PT_ERR_NOT_READY           # pt_reproject itself did
        history()
        t.set_spheres(sph)
        assert ready() == abi.PT_ERR_NOT_READY
        history()
        q = p.copy()
        q.band_rows, q.band_index, q.band_count = 4, 1, 2   # (another set of rows)
        t.set_params(q)
        assert ready() == abi.PT_ERR_NOT_READY
        history()
        t._check(t.lib.pt_resize(t._ctx, 31, 7))
        t.width, t.height = 31, 7
        sph2, p2 = ER.estimate_scene(31, 7)
        t.set_params(p2)
        assert ready() == abi.PT_ERR_NOT_READY
        t.keep_history()                                  # (the planes were reallocated for the new size)
        assert ready() == abi.PT_OK
        t.keep_history()
        t.reproject_option(False)
        t.reproject_option(True)
        assert ready() == abi.PT_ERR_NOT_READY
        t.keep_history()
        t.feature_planes(False)                           # turns reprojection off too
        assert rc_reproject(t) == abi.PT_ERR_NOT_READY and t.lib.pt_keep_history(t._ctx) == abi.PT_ERR_NOT_READY
        assert t.lib.pt_set_option(t._ctx, abi.PT_OPT_REPROJECT, 1) == abi.PT_ERR_INVALID
    finally:
        t.close()


def test_a_band_without_rows_and_a_stream_capture():
    import torch

    sph, p = ER.estimate_scene(33, 9)
    q = p.copy()
    q.band_rows, q.band_index, q.band_count = 16, 1, 2   # rows 16 .. 31 of a 9-row image: none
    t = context(sph, q)
    try:
        assert t.local_rows == 0
        t.render_features()
        t.keep_history()
        t.set_params(q)
        t.render_features()
        assert rc_reproject(t) == abi.PT_OK
        st = t.reproject_stats()
        assert (st.pixels, st.pixels_hit, st.pixels_kept, st.samples_kept) == (0, 0, 0, 0)
    finally:
        t.close()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = context(sph, p, use_torch=True)   # binds the side stream as its launch stream
        t.render_features()
        t.keep_history()
        torch.cuda.current_stream().synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            rc = rc_reproject(t)
            t.render_passes(1)  # (something to capture)
    assert rc == abi.PT_ERR_INVALID
    torch.cuda.synchronize()
    assert rc_reproject(t) == abi.PT_OK       # ... and the refused call did not use the history up
    t.close()


# ---------------------------------------------------------------------------------------------------- (h) the frame loop
def fly(loop_or_none, tracer, state, opt, ticks):
    """`ticks` frames of a flight: the camera turns before every third tick.  With a FrameLoop, through it; else the manual
    sequence on `tracer` / `state` — with `opt` the tick of include/ptrace.h, without it the parent's reset."""
    canvases = []
    prev_now, rendered = 0.0, 0
    for k in range(ticks):
        now = 100.0 + 16.5 * k
        st = loop_or_none.state if loop_or_none is not None else state
        if k % 3 == 0:
            st.set_camera_angles(-90.0 + 0.5 * (k // 3), 0.25 * (k // 3))
        if loop_or_none is not None:
            assert loop_or_none.frame(now)
            canvases.append(loop_or_none.canvas)
            continue
        st.update_position(now - prev_now)
        assert st.should_render(False)
        st.update_render_globals()
        prev_now = now
        v, p = st.view(), st.to_params(now)
        moved = v.render_count <= 1
        carry = moved and opt is not None and rendered > 0
        if moved and not carry:
            tracer.reset()
        tracer.set_params(p)
        if moved and opt is not None:
            tracer.render_features()
            if carry:
                tracer.reproject(opt)
            tracer.keep_history()
        tracer.render()
        canvases.append(tracer.resolve_rgba8(True))
        rendered += 1
    return canvases


@pytest.mark.parametrize("with_options", [True, False])
def test_frame_loop_reproduces_the_manual_sequence(with_options):
    from ray_tracer_webgl_amd.app import FrameLoop
    from ray_tracer_webgl_amd.state import State

    w, h, ticks = 160, 88, 7
    opt = options() if with_options else None
    loop = FrameLoop(w, h, mode="linear", reproject=opt) if with_options else FrameLoop(w, h, mode="linear")
    loop.state.set_flags(is_paused=False)
    got = fly(loop, None, None, None, ticks)
    state = State(w, h)
    state.set_flags(is_paused=False)
    t = PathTracer(w, h)
    try:
        t.set_spheres(state.spheres())
        if with_options:
            t.feature_planes(True)
            t.reproject_option(True)
        t.clear_textures()
        ref = fly(None, t, state, opt, ticks)
        for k in range(ticks):
            assert got[k].tobytes() == ref[k].tobytes(), "tick %d" % k
        assert loop.tracer.accum().tobytes() == t.accum().tobytes()
        counts, spp = t.sample_counts(), state.to_params(0.0).samples_per_pixel
        if with_options:   # the accumulation was carried across both turns: most pixels hold more than the last view's one tick
            assert (counts > spp).mean() > 0.5 and counts.max() <= ticks * spp
            assert loop.tracer.reproject_stats().pixels_kept > 0.5 * w * h
        else:              # the parent's behaviour: the last turn (tick 6) cleared everything
            assert np.all(counts == spp)
    finally:
        t.close()
        state.close()
        loop.close()
