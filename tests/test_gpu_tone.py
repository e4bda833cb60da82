"""The toned read-outs — pt_resolve_toned, pt_resolve_toned_rgba8 (pt_tone_kernel, csrc/pt_kernels_display.hip) — against the plain
restatement of their statements (tests/tone_ref.py): every curve, with and without the square root, as floats and as bytes, read
from the accumulation and from an external source image on the host and on the device, over the read-out tests' edge buffers
(tests/readout_ref.py: every rounding edge of unorm8, every kind of count, non-finite and negative radiance).  Also what the calls
leave alone, the order of their refusals, a rendered frame of config 4, and FrameLoop's toned canvas.

Floats are compared as bit patterns (NaN with NaN), bytes outright; there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import readout_ref as R
import tone_ref as T
from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer, PtError

pytestmark = pytest.mark.gpu

CURVES = (abi.PT_TONE_CLAMP, abi.PT_TONE_REINHARD, abi.PT_TONE_FILMIC)
WHITES = np.array([1.0, 4.0, 983.04, np.inf], np.float32)


def _same_bytes(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref), "%s: %d bytes differ, first at %s" % (what, int((got != ref).sum()), np.argwhere(got != ref)[:3].tolist())


def _context(w, h, use_torch=False, spp=1):
    sc = scenes.default_scene(R.WIDTH, R.HEIGHT, spp=spp, max_depth=6)
    p = sc.params.copy()
    p.width, p.height = w, h
    t = PathTracer(w, h, use_torch=use_torch)
    t.set_spheres(sc.spheres)
    t.set_params(p)
    return t, p


def _check_toned(t, buf, what, case, torch=None):
    """One buffer through every curve x gamma x {float, bytes}, from the accumulation, from host texels and (with torch) from
    device texels.  The exposure and the white point move with the case so that the whole list is met over the buffers."""
    t.load_accum(buf)
    dev = torch.from_numpy(buf).cuda() if torch is not None else None
    n = 0
    for curve in CURVES:
        for gamma in (0, 1):
            e = float(T.EXPOSURES[(case + n) % len(T.EXPOSURES)])
            w = float(WHITES[(case + n) % len(WHITES)])
            n += 1
            opt = abi.PtToneOptions(curve, gamma, e, w)
            for from_accum in (True, False):
                ref = T.toned(buf, from_accum, curve, gamma, e, w)
                ref8 = T.toned_rgba8(buf, from_accum, curve, gamma, e, w)
                srcs = [("accumulation", None)] if from_accum else [("host src", buf)] + ([("device src", dev)] if dev is not None else [])
                for name, src in srcs:
                    tag = "%s, %s, curve %d gamma %d exposure %g white %g" % (what, name, curve, gamma, e, w)
                    got, got8 = t.toned_image(opt, src), t.toned_rgba8(opt, src)
                    if name == "device src":
                        assert got.is_cuda and got8.is_cuda
                        got, got8 = got.cpu().numpy(), got8.cpu().numpy()
                    assert R.same_floats(got, ref), "%s: %s" % (tag, R.first_difference(got, ref))
                    _same_bytes(got8, ref8, tag)
    # PT_TONE_CLAMP at exposure 1 IS pt_resolve / pt_resolve_rgba8 of the same context
    for gamma in (0, 1):
        opt = abi.PtToneOptions(abi.PT_TONE_CLAMP, gamma, 1.0, 1.0)
        got, ref = t.toned_image(opt), t.resolve(bool(gamma))
        assert R.same_floats(got, ref), "%s, clamp at exposure 1 against pt_resolve, gamma %d: %s" % (what, gamma, R.first_difference(got, ref))
        _same_bytes(t.toned_rgba8(opt), t.resolve_rgba8(bool(gamma)), "%s, clamp at exposure 1 against pt_resolve_rgba8, gamma %d" % (what, gamma))


@pytest.mark.parametrize("i", range(6))
def test_toned_read_outs_on_the_edge_buffers(i):
    """64 x 36: every edge colour under a count whose reciprocal is exact, one whose is not and one that is none."""
    import torch

    bufs = R.edge_accums()
    assert len(bufs) == 6
    t, _ = _context(R.WIDTH, R.HEIGHT, use_torch=True)
    try:
        _check_toned(t, bufs[i], "edge buffer %d" % i, 7 * i, torch)
    finally:
        t.close()


@pytest.mark.parametrize("w,h,seed", [(1, 1, 8), (3, 5, 9), (17, 16, 10)])
def test_toned_read_outs_on_other_sizes(w, h, seed):
    """A single pixel, fifteen, and 272: a block and a bit."""
    import torch

    t, _ = _context(w, h, use_torch=True)
    try:
        _check_toned(t, R.small_accum(h, w, seed), "%dx%d" % (w, h), seed, torch)
    finally:
        t.close()


def test_past_the_launch_cap_the_last_row_is_toned():
    """1024 x 513: the smallest shape whose last row is the pixel kernels' second trip (2048 workgroups of 256)."""
    w, h = 1024, 513
    rng = np.random.default_rng(5)
    buf = R.accum_with(rng.choice(R.edge_colours(), h * w * 3), np.full(h * w, 3.0, np.float32), h, w)
    t, _ = _context(w, h)
    try:
        t.load_accum(buf)
        for curve, from_accum in ((abi.PT_TONE_REINHARD, True), (abi.PT_TONE_FILMIC, False)):
            opt = abi.PtToneOptions(curve, 1, 0.37, 4.0)
            got = t.toned_rgba8(opt, None if from_accum else buf)
            ref = T.toned_rgba8(buf[-2:], from_accum, curve, 1, 0.37, 4.0)
            _same_bytes(got[-2:], ref, "the last two rows, curve %d" % curve)
            assert (got[..., 3] == 255).all()
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ what the calls leave alone
def _snapshot(t):
    st = t.stats()
    return dict(accum=t.accum().view(np.uint32).copy(), err=t.error_state().view(np.uint32).copy(),
                stats=bytes(memoryview(st))[:], build=t.last_trace_build(), canvas=t.read_canvas().copy())


def _same_snapshot(a, b, what):
    for k in a:
        same = np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]
        assert same, "%s moved %s" % (what, k)


def test_the_calls_leave_the_context_alone():
    """The accumulation's bits, the estimate, PtStats (first_pass shows in the next pass's bits), pt_last_trace_build and the canvas
    before and after each new call; then two more passes give the bits of a context that never metered."""
    sc = scenes.default_scene(R.WIDTH, R.HEIGHT, spp=2, max_depth=6)
    sc.params.time_step = abi.PT_TIME_STEP_DECORRELATED

    def fresh():
        t = PathTracer(R.WIDTH, R.HEIGHT)
        t.set_spheres(sc.spheres)
        t.error_estimate(True)
        t.set_params(sc.params)
        t.reserve_passes(2)
        t.render_passes(2)
        return t

    t, plain = fresh(), fresh()
    try:
        t.tone_mapping(True)
        before = _snapshot(t)
        ext = R.edge_accums()[0]
        calls = [("pt_meter", lambda: t.meter()), ("pt_meter, window", lambda: t.meter(abi.PtMeterOptions(window=(3, 4, 200, 7)))),
                 ("pt_meter, host src", lambda: t.meter(src=ext)), ("pt_meter_read", lambda: t.exposure()),
                 ("pt_meter_set", lambda: t.set_exposure(t.exposure()[0])),
                 ("pt_resolve_toned", lambda: t.toned_image()), ("pt_resolve_toned_rgba8", lambda: t.toned_rgba8()),
                 ("pt_resolve_toned, host src", lambda: t.toned_image(abi.PtToneOptions(abi.PT_TONE_FILMIC, 1, 2.0, 1.0), ext)),
                 ("PT_OPT_TONEMAP off", lambda: t.tone_mapping(False))]
        for name, call in calls:
            call()
            _same_snapshot(before, _snapshot(t), name)
        for c in (t, plain):
            p = sc.params.copy()
            p.first_pass = 2
            c.set_params(p)
            c.render_passes(2)
        assert np.array_equal(t.accum().view(np.uint32), plain.accum().view(np.uint32))
        assert np.array_equal(t.error_state().view(np.uint32), plain.error_state().view(np.uint32))
    finally:
        t.close()
        plain.close()


def test_the_order_of_the_refusals():
    """Arguments, then the option (only where the device record is asked for), then the capture, then what pt_resolve answers."""
    import torch

    t, _ = _context(R.WIDTH, R.HEIGHT, use_torch=True)
    try:
        out = np.zeros((R.HEIGHT, R.WIDTH, 4), np.float32)
        po = out.ctypes.data_as(C.c_void_p)
        for fn in (t.lib.pt_resolve_toned, t.lib.pt_resolve_toned_rgba8):
            good = abi.PtToneOptions(abi.PT_TONE_CLAMP, 1, 1.0, 1.0)
            assert fn(None, None, C.byref(good), po) == abi.PT_ERR_INVALID
            assert fn(t._ctx, None, None, po) == abi.PT_ERR_INVALID and fn(t._ctx, None, C.byref(good), None) == abi.PT_ERR_INVALID
            for bad in (abi.PtToneOptions(3, 1, 1.0, 1.0), abi.PtToneOptions(-1, 1, 1.0, 1.0), abi.PtToneOptions(0, 1, -1.0, 1.0),
                        abi.PtToneOptions(0, 1, float("nan"), 1.0), abi.PtToneOptions(0, 1, float("inf"), 1.0),
                        abi.PtToneOptions(abi.PT_TONE_REINHARD, 1, 1.0, 0.0), abi.PtToneOptions(abi.PT_TONE_REINHARD, 1, 1.0, float("nan"))):
                assert fn(t._ctx, None, C.byref(bad), po) == abi.PT_ERR_INVALID, (bad.curve, bad.exposure, bad.white)
            # invalid arguments come before "nothing rendered yet"; with good ones that is the answer, as pt_resolve's
            assert fn(t._ctx, None, C.byref(good), po) == abi.PT_ERR_NOT_READY and b"nothing rendered yet" in t.lib.pt_last_error(t._ctx)
            assert t.lib.pt_resolve(t._ctx, po, 1) == abi.PT_ERR_NOT_READY
            # the device record: the option is off, then on and not valid
            rec = abi.PtToneOptions(abi.PT_TONE_CLAMP, 1, 0.0, 1.0)
            assert fn(t._ctx, None, C.byref(rec), po) == abi.PT_ERR_NOT_READY and b"PT_OPT_TONEMAP" in t.lib.pt_last_error(t._ctx)
            t.tone_mapping(True)
            assert fn(t._ctx, None, C.byref(rec), po) == abi.PT_ERR_NOT_READY and b"no exposure yet" in t.lib.pt_last_error(t._ctx)
            t.tone_mapping(False)
        # an explicit exposure needs neither the option nor a record — an external source not even a rendered frame
        ext = R.edge_accums()[1]
        opt = abi.PtToneOptions(abi.PT_TONE_FILMIC, 0, 15.0, 1.0)
        assert R.same_floats(t.toned_image(opt, ext), T.toned(ext, False, abi.PT_TONE_FILMIC, 0, 15.0, 1.0))
    finally:
        t.close()


def test_calls_inside_a_stream_capture_are_refused():
    """Every new call that enqueues or synchronises answers PT_ERR_INVALID inside a capture, before anything is enqueued."""
    import torch

    sc = scenes.default_scene(R.WIDTH, R.HEIGHT, spp=1, max_depth=6)
    ext = R.edge_accums()[1]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = PathTracer(R.WIDTH, R.HEIGHT, use_torch=True)  # binds the side stream as its launch stream
        t.set_spheres(sc.spheres)
        t.set_params(sc.params)
        t.tone_mapping(True)
        t.load_accum(ext)
        t.meter()
        rec0, hist0 = t.exposure()
        dev = torch.from_numpy(ext).cuda()
        out = torch.full((R.HEIGHT, R.WIDTH, 4), 0x5a, dtype=torch.uint8, device="cuda")
        torch.cuda.current_stream().synchronize()
        opt, mopt, rec = abi.PtToneOptions(abi.PT_TONE_FILMIC, 1, 1.0, 1.0), abi.PtMeterOptions(), abi.PtExposure()
        codes = {}
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for name, call in (("pt_meter", lambda: t.lib.pt_meter(t._ctx, C.c_void_p(dev.data_ptr()), C.byref(mopt))),
                               ("pt_meter_read", lambda: t.lib.pt_meter_read(t._ctx, C.byref(rec), None)),
                               ("pt_meter_set", lambda: t.lib.pt_meter_set(t._ctx, C.byref(rec0))),
                               ("pt_resolve_toned_rgba8", lambda: t.lib.pt_resolve_toned_rgba8(t._ctx, C.c_void_p(dev.data_ptr()), C.byref(opt),
                                                                                               C.c_void_p(out.data_ptr()))),
                               ("pt_resolve_toned", lambda: t.lib.pt_resolve_toned(t._ctx, None, C.byref(opt), C.c_void_p(out.data_ptr())))):
                codes[name] = (call(), t.lib.pt_last_error(t._ctx))
            t.render_passes(1)  # (something to capture)
    torch.cuda.synchronize()
    for name, (rc, msg) in codes.items():
        assert rc == abi.PT_ERR_INVALID and b"capture" in msg, (name, rc, msg)
    assert (out.cpu().numpy() == 0x5a).all(), "refused before anything was launched"
    rec1, hist1 = t.exposure()
    assert T.same_record(T.record_of(rec1), T.record_of(rec0)) and np.array_equal(hist0, hist1)
    t.close()


# ------------------------------------------------------------------------------------------------ a rendered frame
def test_config4_metered_and_toned_against_the_oracle(ora):
    """The closed room lit by a sphere of radiance 15, 64 x 64, two passes of 4 spp: pt_meter and the Reinhard and filmic bytes
    against the restatement ON THE ORACLE'S accumulation (the device accumulation is pinned to it here once more)."""
    sc = scenes.config4(width=64, height=64, spp_per_pass=4, n_passes=2)
    acc, _ = ora.render(sc.spheres, sc.params, 2)
    t = PathTracer(64, 64)
    try:
        t.set_spheres(sc.spheres)
        t.set_params(sc.params)
        t.reserve_passes(2)
        t.render_passes(2)
        assert np.array_equal(t.accum().view(np.uint32), acc.view(np.uint32))
        t.tone_mapping(True)
        t.meter()
        rec, hist = t.exposure()
        ref_hist, ref_below = T.meter(acc, True)
        assert [int(x) for x in hist] == ref_hist and rec.below == ref_below
        ref = T.solve(ref_hist, ref_below)
        assert T.same_record(T.record_of(rec), ref), (T.record_of(rec), ref)
        clipped = {"pt_resolve_rgba8": int((t.resolve_rgba8(True)[..., :3] == 255).sum())}
        for name, curve in (("reinhard", abi.PT_TONE_REINHARD), ("filmic", abi.PT_TONE_FILMIC)):
            got = t.toned_rgba8(abi.PtToneOptions(curve, 1, 0.0, 0.0))
            _same_bytes(got, T.toned_rgba8(acc, True, curve, 1, ref["exposure"], ref["white"]), name)
            clipped[name] = int((got[..., :3] == 255).sum())
        print("config 4, 64x64, 8 spp: exposure %g, white %g; channel values at 255: %r" % (rec.exposure, rec.white, clipped))
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ FrameLoop
def _ticks(loop, n):
    loop.state.set_flags(is_paused=False)
    out = []
    for k in range(n):
        assert loop.frame(100.0 + 16.5 * k)
        out.append(loop.canvas.copy())
    return out


def test_frame_loop_draws_its_canvas_through_the_tone_curve():
    """FrameLoop(mode="linear"): tone=None canvases are pt_resolve_rgba8's; with tone=... a 10-tick run equals the same calls issued by hand."""
    from ray_tracer_webgl_amd.app import FrameLoop

    w, h, n = R.WIDTH, R.HEIGHT, 10
    meter = abi.PtMeterOptions(rate=0.25)
    tone = abi.PtToneOptions(abi.PT_TONE_FILMIC, 1, 0.0, 1.0)
    plain, toned, hand = FrameLoop(w, h, mode="linear"), FrameLoop(w, h, mode="linear", tone=(meter, tone)), FrameLoop(w, h, mode="linear")
    try:
        a, b = _ticks(plain, n), _ticks(toned, n)
        hand.state.set_flags(is_paused=False)
        hand.tracer.tone_mapping(True)
        for k in range(n):
            assert hand.frame(100.0 + 16.5 * k)
            _same_bytes(a[k], hand.canvas, "tick %d without tone" % k)        # today's canvas, byte for byte
            _same_bytes(a[k], hand.tracer.resolve_rgba8(True), "tick %d: the canvas is pt_resolve_rgba8's" % k)
            hand.tracer.meter(meter)
            _same_bytes(b[k], hand.tracer.toned_rgba8(tone), "tick %d with tone" % k)
        rec, _ = toned.tracer.exposure()
        ref, _ = hand.tracer.exposure()
        assert rec.meterings == n and T.same_record(T.record_of(rec), T.record_of(ref))
        assert not np.array_equal(a[-1], b[-1])
        with pytest.raises(AssertionError):
            FrameLoop(w, h, mode="reference", tone=(meter, tone))
    finally:
        for loop in (plain, toned, hand):
            loop.close()
