"""Temporal reprojection with the error estimate (pt_reproject_estimate; include/ptrace.h has the contract) on
the device: the state bit for bit against tests/reproject_estimate_ref.py, the accumulation bit for bit against what
pt_reproject leaves for the same inputs (and against tests/reproject_ref.py), the tallies equal.  Tolerance: none (NaN compares
equal to NaN).

Hand-made inputs go in as in test_gpu_reproject.py (current planes over pt_features_ptr after a pt_render_features, history
through pt_load_history); one rendered pass first makes the context remember a samples_per_pixel (only a fold does), then the
accumulation is overwritten through pt_accum_ptr and the state through pt_error_ptr.

  (a) operands       hand-made frames and states with every operand class at 37x21 and 131x13, three settings each
  (b) 5x3            less than one workgroup
  (c) bands          both ranks of 74x26 in bands of 4 rows (the last chunk is partial)
  (d) a flight       three ticks at 96x54, device-rendered passes folded onto the carried state, compared after every tick:
                     1 spp x 4 passes, and 4 spp x 2 passes with cap_other = 4 (that class carries nothing); the patch-wise
                     filtered read-out and pt_error_stats of the carried state against their restatements
  (e) FrameLoop(carry_estimate=True) reproduces the manual sequence; False is the parent's canvas byte for byte
  (f) nothing else of the context moves (statistics, textures, canvas; first_pass and the tile order through the next pass,
      which is the oracle's fold bit for bit); the next fold with another samples_per_pixel is refused; nothing folded: a clear
  (g) the refusals: estimate off, no history, no planes, inside a stream capture; a band without rows
"""
import ctypes as C

import numpy as np
import pytest

import error_ref as ER
import patch_filter_ref as PF
import reproject_estimate_ref as REF
import reproject_ref as RR
from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd.tracer import PathTracer, PtError, _H2D, _memcpy

pytestmark = pytest.mark.gpu

CAPS, TOL = (32.0, 8.0), 2.0


def options(caps=CAPS, tol=TOL):
    return abi.PtReprojectOptions(caps[0], caps[1], tol)


def context(sph, p, estimate=True, use_torch=False):
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


def write_accum(t, acc):
    """overwrite the accumulation in place (pt_load_accum would clear the estimate and forget its samples_per_pixel)"""
    a = np.ascontiguousarray(acc, np.float32)
    ptr, nbytes = C.c_void_p(), C.c_size_t()
    t._check(t.lib.pt_accum_ptr(t._ctx, C.byref(ptr), C.byref(nbytes)))
    t.synchronize()
    assert nbytes.value == a.nbytes
    if a.nbytes:
        _memcpy(ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, _H2D)


def load_hand(t, p, f, st):
    write_current_planes(t, f["cur_ids"], f["cur_pnt"])
    t.load_history(p, f["hist_ids"], f["hist_pnt"])
    write_accum(t, f["acc"])
    t.load_error_state(st)


def tallies_of(t):
    s = t.reproject_stats()
    return {k: int(getattr(s, k)) for k in ("pixels", "pixels_hit", "pixels_kept", "samples_kept")}


def check_hand(sph, p, f, st, S, settings, what):
    """pt_reproject_estimate and pt_reproject on the same hand-made inputs, in one context that has folded one pass of S spp"""
    q = p.copy()
    q.samples_per_pixel = S
    t = context(sph, q)
    try:
        t.render_passes(1)    # the context now remembers S
        for caps, tol in settings:
            load_hand(t, q, f, st)
            t.reproject_estimate(options(caps, tol))
            got_acc, got_st, got_tallies = t.accum(), t.error_state(), tallies_of(t)
            out, new, tallies = REF.reproject_estimate(f["cur_ids"], f["cur_pnt"], f["hist_ids"], f["hist_pnt"], f["acc"], st, S, q, q,
                                                       caps[0], caps[1], tol)
            tag = "%s, caps %s tolerance %s" % (what, caps, tol)
            assert RR.same_floats(got_st, new), "%s: state: %s" % (tag, RR.first_difference(got_st, new))
            assert RR.same_floats(got_acc, out), "%s: accumulation: %s" % (tag, RR.first_difference(got_acc, out))
            assert got_tallies == tallies, tag
            load_hand(t, q, f, st)
            t.reproject(options(caps, tol))
            plain = t.accum()
            assert RR.same_floats(got_acc, plain), "%s: against pt_reproject: %s" % (tag, RR.first_difference(got_acc, plain))
            assert tallies_of(t) == got_tallies, tag
            assert not t.error_state().any()      # pt_reproject cleared it, and forgot S:
            t.render_passes(1)                    # ... so this fold is the first again
    finally:
        t.close()
    return new


SETTINGS = ((CAPS, TOL), ((16777215.0, 12.0), 1000.0), ((7.0, 100.0), 0.5))


# ---------------------------------------------------------------------------------------------------- (a) operands
@pytest.mark.parametrize("w,h,S", [(37, 21, 4), (131, 13, 1)])
def test_every_operand_class(w, h, S):
    sph, p = ER.estimate_scene(w, h)
    f = RR.hand_frame(p)
    st, cls = REF.hand_state(h, w, S=S)
    new = check_hand(sph, p, f, st, S, SETTINGS, "%dx%d" % (w, h))
    if w == 131:
        assert all((cls == i).any() for i in range(len(REF.STATE_CLASSES)))
        assert (new[..., 0, 3] >= 2).any() and not new.all()


# ---------------------------------------------------------------------------------------------------- (b) below one workgroup
def test_less_than_one_workgroup():
    sph, p = ER.estimate_scene(5, 3)
    f = RR.hand_frame(p, seed=2)
    st, _ = REF.hand_state(3, 5, seed=4)
    check_hand(sph, p, f, st, 4, ((CAPS, TOL), ((64.0, 64.0), 4.0)), "5x3")


# ---------------------------------------------------------------------------------------------------- (c) bands
@pytest.mark.parametrize("rank", [0, 1])
def test_both_ranks_of_a_band(rank):
    sph, p = ER.estimate_scene(74, 26)
    f = RR.hand_frame(p, seed=11)
    st, _ = REF.hand_state(26, 74, seed=12)
    q = p.copy()
    q.band_rows, q.band_index, q.band_count = 4, rank, 2
    ys = abi.owned_rows(26, 4, rank, 2)
    g = {k: v[ys] for k, v in f.items()}
    new = check_hand(sph, q, g, st[ys], 4, ((CAPS, TOL),), "band %d of 2" % rank)
    assert (new[..., 0, 3] >= 2).sum() > 100


# ---------------------------------------------------------------------------------------------------- (d) a flight
@pytest.mark.parametrize("spp,passes,caps", [(1, 4, CAPS), (4, 2, (32.0, 4.0))])
def test_three_ticks_of_the_flight(spp, passes, caps):
    W, H = 96, 54
    sph, p0 = ER.estimate_scene(W, H, spp=spp)
    t = context(sph, p0)
    try:
        t.reserve_passes(passes)
        t.render_features()
        planes = t.features()
        t.render_passes(passes)
        prev, first = p0, passes
        for k in (1, 2, 3):
            p = RR.flight_params(p0, k)
            p.first_pass = first
            acc, st = t.accum(), t.error_state()
            t.keep_history()             # the tick of include/ptrace.h, with pt_reproject_estimate in pt_reproject's place
            t.set_params(p)
            t.render_features()
            t.reproject_estimate(options(caps))
            cur = t.features()
            out, new, tallies = REF.reproject_estimate(cur["ids"], cur["point"], planes["ids"], planes["point"], acc, st, spp, prev, p,
                                                       caps[0], caps[1], TOL)
            got_st, got_acc = t.error_state(), t.accum()
            assert RR.same_floats(got_st, new), "tick %d: state: %s" % (k, RR.first_difference(got_st, new))
            assert RR.same_floats(got_acc, out), "tick %d: accumulation: %s" % (k, RR.first_difference(got_acc, out))
            assert tallies_of(t) == tallies
            known = new[..., 0, 3] >= 2
            assert 0.3 < known.mean() < 0.70
            other = (cur["ids"][..., 0] >= 0) & (cur["ids"][..., 2] != abi.PT_DIFFUSE)
            if caps[1] < 2 * spp:        # a class whose cap is below 2 passes carries no estimate, but keeps its samples
                assert other.any() and not new[other].any() and (out[other][:, 3] > 0).any()
            else:
                assert (new[other][:, 0, 3] >= 2).any()
            # the read-outs of the carried state: the patch-wise filter and the frame's statistics
            img = t.patch_filtered_image(2, 1, 1.5, gamma=False)
            ref_img = PF.filtered(new, 2, 1, 1.5)
            assert RR.same_floats(img, ref_img), "tick %d: filtered: %s" % (k, RR.first_difference(img, ref_img))
            assert ER.same_stats(t.error_stats(), ER.stats(new)) == ""
            # the tick's fresh passes fold onto the carried state
            t.render_passes(passes)
            first += passes
            got_st = t.error_state()
            assert np.all(got_st[..., 0, 3] == new[..., 0, 3] + passes)
            assert np.all(got_st[..., 1, 3] == new[..., 1, 3] + passes * spp)
            assert np.array_equal(t.sample_counts(), out[..., 3] + passes * spp)
            planes, prev = cur, p
    finally:
        t.close()


def test_the_fold_onto_the_carried_state_is_the_restated_fold(ora):
    """one tick at 37x21: the passes folded after pt_reproject_estimate give error_ref.fold of the oracle's passes onto the
    restated carried state, bit for bit"""
    sph, p0 = ER.estimate_scene(37, 21)
    t = context(sph, p0)
    try:
        t.reserve_passes(2)
        t.render_features()
        planes = t.features()
        t.render_passes(2)
        acc, st = t.accum(), t.error_state()
        p = RR.flight_params(p0, 1)
        p.first_pass = 2
        t.keep_history()
        t.set_params(p)
        t.render_features()
        t.reproject_estimate(options())
        cur = t.features()
        out, new, _ = REF.reproject_estimate(cur["ids"], cur["point"], planes["ids"], planes["point"], acc, st, 4, p0, p, CAPS[0], CAPS[1], TOL)
        t.render_passes(2)
        ref_st, ref_acc = ER.fold(new, out, ER.oracle_passes(ora, sph, p, 2))
        assert RR.same_floats(t.error_state(), ref_st) and RR.same_floats(t.accum(), ref_acc)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------- (e) the frame loop
def fly(loop_or_none, tracer, state, opt, ticks, carry_estimate):
    """test_gpu_reproject.py's flight: the camera turns before every third tick.  With a FrameLoop, through it; else the manual
    sequence on `tracer` / `state`."""
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
            if carry and carry_estimate:
                tracer.reproject_estimate(opt)
            elif carry:
                tracer.reproject(opt)
            tracer.keep_history()
        tracer.render()
        canvases.append(tracer.resolve_rgba8(True))
        rendered += 1
    return canvases


@pytest.mark.parametrize("carry_estimate", [True, False])
def test_frame_loop(carry_estimate):
    from ray_tracer_webgl_amd.app import FrameLoop
    from ray_tracer_webgl_amd.state import State

    w, h, ticks = 160, 88, 7
    opt = options()
    loop = FrameLoop(w, h, mode="linear", reproject=opt, carry_estimate=carry_estimate)
    loop.state.set_flags(is_paused=False)
    got = fly(loop, None, None, None, ticks, carry_estimate)
    state = State(w, h)
    state.set_flags(is_paused=False)
    t = PathTracer(w, h)
    try:
        t.set_spheres(state.spheres())
        t.feature_planes(True)
        t.reproject_option(True)
        if carry_estimate:
            t.error_estimate(True)
        t.clear_textures()
        # carry_estimate=False: the manual sequence is the PARENT's (plain pt_reproject, no estimate)
        ref = fly(None, t, state, opt, ticks, carry_estimate)
        for k in range(ticks):
            assert got[k].tobytes() == ref[k].tobytes(), "tick %d" % k
        assert loop.tracer.accum().tobytes() == t.accum().tobytes()
        if carry_estimate:
            a, b = loop.tracer.error_state(), t.error_state()
            assert a.tobytes() == b.tobytes()
            # seven ticks of one pass, carried across both turns: most hit pixels hold more passes than the last view's one
            assert (a[..., 0, 3] > 1).mean() > 0.4 and a[..., 0, 3].max() <= ticks
            img = loop.tracer.patch_filtered_image(2, 1, 1.5)
            assert (img[..., 3] > 1).mean() > 0.3      # ... so the filter has neighbourhoods to accept
        else:
            with pytest.raises(PtError):
                loop.tracer.error_state()              # the estimate was never turned on
    finally:
        t.close()
        state.close()
        loop.close()


def test_frame_loop_when_the_samples_per_pixel_change():
    """the estimate holds passes of one size: when the State's samples_per_pixel change the loop does not carry it (a turning
    camera: pt_reproject, which clears it) or starts the frame afresh (a standing one); no fold is ever refused"""
    from ray_tracer_webgl_amd.app import FrameLoop

    loop = FrameLoop(96, 54, mode="linear", reproject=options(), carry_estimate=True)
    try:
        loop.state.set_flags(is_paused=False)
        depth = loop.state.view().max_depth

        def known_passes_of(spp):
            st = loop.tracer.error_state()
            n, k = st[..., 0, 3], st[..., 1, 3]
            assert np.all(k == n * spp)
            return n

        now = 100.0
        for tick in range(7):
            if tick in (2, 5):
                loop.state.set_camera_angles(-90.0 + 0.5 * tick, 0.0)      # a turn
            if tick in (3, 5):
                loop.state.set_quality(2 if tick == 3 else 3, depth)       # alone at tick 3, together with a turn at tick 5
            assert loop.frame(now)
            now += 16.5
            spp = loop.state.to_params(0.0).samples_per_pixel
            n = known_passes_of(spp)
            if tick == 2:
                assert n.max() == 3 and (n == 3).mean() > 0.4               # carried across the turn
            if tick in (3, 5):
                assert np.all(n == 1)                                       # afresh / cleared: the tick's own pass alone
            if tick == 5:
                assert (loop.tracer.sample_counts() > spp).mean() > 0.4     # ... while the accumulation was carried
    finally:
        loop.close()


# ---------------------------------------------------------------------------------------------------- (f) nothing else moves
def test_nothing_else_of_the_context_moves_and_the_next_fold_keeps_its_spp(ora):
    sph, p0 = ER.estimate_scene(37, 21)
    p1 = RR.flight_params(p0, 1)
    t = context(sph, p0)
    try:
        t.reserve_passes(2)
        t.render_until(1e-9, 2, 4)        # four passes: first_pass stands at 4, the estimate knows them
        t.render_frame(0)
        tex, canvas = [t.read_texture(0), t.read_texture(1)], t.read_canvas()
        t.render_features()
        t.keep_history()
        q = p1.copy()
        q.first_pass = 4
        t.set_params(q)
        t.render_features()
        before = t.stats()
        t.reproject_estimate(options())
        after = t.stats()
        assert t.reproject_stats().pixels_kept > 0
        assert (t.error_state()[..., 0, 3] >= 2).any()           # carried, not cleared
        for k in ("segments", "samples", "render_launches", "far_rays"):
            assert getattr(after, k) == getattr(before, k), k
        assert np.array_equal(t.read_texture(0), tex[0]) and np.array_equal(t.read_texture(1), tex[1])
        assert np.array_equal(t.read_canvas(), canvas)
        # the next fold with another samples_per_pixel is refused, as after any fold; with the same one it is pass 4 of the view
        r = q.copy()
        r.samples_per_pixel = 2
        t.set_params(r)
        assert t.lib.pt_render_passes(t._ctx, 1) == abi.PT_ERR_INVALID
        t.set_params(q)
        st, acc = t.error_state(), t.accum()
        t.render_passes(1)
        ref_st, ref_acc = ER.fold(st, acc, ER.oracle_passes(ora, sph, q, 1))
        assert RR.same_floats(t.error_state(), ref_st) and RR.same_floats(t.accum(), ref_acc)
    finally:
        t.close()


def test_nothing_folded_since_the_last_clear_is_pt_reproject():
    sph, p = ER.estimate_scene(37, 21)
    f = RR.hand_frame(p)
    f["acc"][0, 0] = (1.5, 0.25, 3.0, 3.0)
    f["acc"][-1, -1] = (0.5, 2.25, 1.0, 3.0)     # (a checkpoint pt_load_accum accepts)
    t = context(sph, p)
    try:
        write_current_planes(t, f["cur_ids"], f["cur_pnt"])
        t.load_history(p, f["hist_ids"], f["hist_pnt"])
        t.load_accum(f["acc"])                    # clears the estimate: nothing folded
        t.reproject_estimate(options())
        out, tallies = RR.reproject(f["cur_ids"], f["cur_pnt"], f["hist_ids"], f["hist_pnt"], f["acc"], p, p, CAPS[0], CAPS[1], TOL)
        assert RR.same_floats(t.accum(), out) and tallies_of(t) == tallies
        assert not t.error_state().any()
        q = p.copy()
        q.samples_per_pixel = 2
        t.set_params(q)
        t.render_passes(1)                        # ... and any samples_per_pixel may come next
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------- (g) refusals
def rc_estimate(t, opt=None):
    o = opt if opt is not None else options()
    return t.lib.pt_reproject_estimate(t._ctx, C.byref(o))


def test_refusals_in_order():
    sph, p = ER.estimate_scene(33, 9)
    t = PathTracer(33, 9)
    try:
        t.set_spheres(sph)
        t.set_params(p)
        assert rc_estimate(t) == abi.PT_ERR_NOT_READY and b"reprojection is off" in t.lib.pt_last_error(t._ctx)
        t.feature_planes(True)
        t.reproject_option(True)
        # the estimate off: refused before the history and the planes are looked at, and with them in place too
        assert rc_estimate(t) == abi.PT_ERR_NOT_READY and b"error estimate is off" in t.lib.pt_last_error(t._ctx)
        t.render_features()
        t.keep_history()
        assert rc_estimate(t) == abi.PT_ERR_NOT_READY and b"error estimate is off" in t.lib.pt_last_error(t._ctx)
        assert t.lib.pt_reproject(t._ctx, C.byref(options())) == abi.PT_OK      # ... which pt_reproject does not need
        t.error_estimate(True)
        t.reserve_passes(2)
        t.render_passes(2)                                                       # (two: a state of one pass carries nothing)
        assert t.lib.pt_reproject_estimate(t._ctx, None) == abi.PT_ERR_INVALID
        for caps, tol in (((-1.0, 8.0), 2.0), ((32.0, 2.5), 2.0), ((16777216.0, 8.0), 2.0), (CAPS, -0.5), (CAPS, float("nan"))):
            assert rc_estimate(t, options(caps, tol)) == abi.PT_ERR_INVALID, (caps, tol)
        assert rc_estimate(t) == abi.PT_ERR_NOT_READY and b"no history" in t.lib.pt_last_error(t._ctx)   # (used up above)
        t.keep_history()
        t.set_params(p)                                                          # the planes no longer speak
        assert rc_estimate(t) == abi.PT_ERR_NOT_READY and b"pt_render_features" in t.lib.pt_last_error(t._ctx)
        before = t.error_state()
        t.render_features()
        assert rc_estimate(t) == abi.PT_OK                                       # ... and no refusal used the history up
        assert rc_estimate(t) == abi.PT_ERR_NOT_READY                            # one-shot
        assert (before[..., 0, 3] == 2).all() and (t.error_state()[..., 0, 3] == 2).any()
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
        assert rc_estimate(t) == abi.PT_OK
        st = t.reproject_stats()
        assert (st.pixels, st.pixels_hit, st.pixels_kept, st.samples_kept) == (0, 0, 0, 0)
    finally:
        t.close()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = context(sph, p, use_torch=True)   # binds the side stream as its launch stream
        t.render_passes(1)
        t.render_features()
        t.keep_history()
        torch.cuda.current_stream().synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            rc = rc_estimate(t)
            t.render_passes(1)  # (something to capture)
    assert rc == abi.PT_ERR_INVALID
    torch.cuda.synchronize()
    assert rc_estimate(t) == abi.PT_OK        # ... and the refused call did not use the history up
    t.close()
