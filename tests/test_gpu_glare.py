"""pt_glare (csrc/pt_kernels_glare.hip: down, gather, composite) against the plain restatement of its statements
(tests/glare_ref.py), bit for bit: every size and level count of the CPU tests, from the accumulation, from host texels and from
device texels, to host and device pointers and in place over a device source; a frame with more level-1 tiles than the down
kernel's grid; config 4 glared, metered and toned against the chained restatements; what the call leaves alone, the order of its
refusals, the option off and on, pt_resize, and FrameLoop's glared canvas.

Floats are compared as bit patterns (NaN with NaN), bytes outright; there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import glare_ref as G
import readout_ref as R
import tone_ref as T
from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer

pytestmark = pytest.mark.gpu


def _abi_opt(o):
    return abi.PtGlareOptions(o["strength"], o["threshold"], o["levels"], o["weights"])


def _weights(levels):
    w = np.arange(levels, 0, -1, dtype=np.float64)
    return tuple(float(np.float32(v)) for v in w / w.sum())


def _context(w, h, use_torch=False, spp=1):
    sc = scenes.default_scene(R.WIDTH, R.HEIGHT, spp=spp, max_depth=6)
    p = sc.params.copy()
    p.width, p.height = w, h
    t = PathTracer(w, h, use_torch=use_torch)
    t.set_spheres(sc.spheres)
    t.set_params(p)
    return t, p


def _same(got, ref, what):
    assert R.same_floats(got, ref), "%s: %s" % (what, R.first_difference(got, ref))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else C.c_void_p(a.data_ptr())


def _call(t, src, opt, out):
    """pt_glare with any mix of host arrays and device tensors"""
    o = _abi_opt(opt)
    t._check(t.lib.pt_glare(t._ctx, _ptr(src) if src is not None else None, C.byref(o), _ptr(out)))
    return out


def _option_sets(levels):
    w = _weights(levels)
    return (G.options(1.0, 0.0, levels, w), G.options(0.15, 0.75, levels, w), G.options(0.0, 0.0, levels, w))


# ------------------------------------------------------------------------------------------------ sizes, sources, destinations
@pytest.mark.parametrize("w,h", G.SIZES)
def test_every_size_level_count_source_and_destination(w, h):
    """1x1 (eight levels of one texel), 1x7, 3x5, 17x16 (a tile and a column), 33x130 (odd at several levels, nine tiles tall at
    level 1) and 64x36; levels 1, 2, 5 and 8.  Random texels as the accumulation (per-pixel counts, some zero), as host texels and
    as device texels; the output to a host array, to a device tensor and in place over the device source."""
    import torch

    t, _ = _context(w, h, use_torch=True)
    try:
        t.glare(True)
        n = 0
        for levels in G.LEVELS:
            for opt in _option_sets(levels):
                n += 1
                acc, lin = G.random_frame(w, h, 50 + n, True), G.random_frame(w, h, 80 + n, False)
                tag = "%dx%d levels %d strength %g threshold %g" % (w, h, levels, opt["strength"], opt["threshold"])
                t.load_accum(acc)
                ref = G.glare(acc, True, opt)
                _same(_call(t, None, opt, np.empty_like(acc)), ref, tag + ", accumulation to host")
                dev_out = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda")
                _same(_call(t, None, opt, dev_out).cpu().numpy(), ref, tag + ", accumulation to device")
                ref = G.glare(lin, False, opt)
                _same(_call(t, lin, opt, np.empty_like(lin)), ref, tag + ", host to host")
                _same(_call(t, lin, opt, dev_out).cpu().numpy(), ref, tag + ", host to device")
                dev = torch.from_numpy(lin).cuda()
                _same(_call(t, dev, opt, np.empty_like(lin)), ref, tag + ", device to host")
                assert np.array_equal(dev.cpu().numpy().view(np.uint32), lin.view(np.uint32)), tag + ": the source is only read"
                _same(_call(t, dev, opt, dev).cpu().numpy(), ref, tag + ", in place over the device source")
        # the wrappers: numpy in, numpy out; a device tensor in, a device tensor out
        opt = G.options(0.5, 0.0, 2, (0.5, 0.5))
        lin = G.random_frame(w, h, 3, False)
        _same(t.glared_image(lin, _abi_opt(opt)), G.glare(lin, False, opt), "glared_image, numpy")
        got = t.glared_image(torch.from_numpy(lin).cuda(), _abi_opt(opt))
        assert got.is_cuda
        _same(got.cpu().numpy(), G.glare(lin, False, opt), "glared_image, torch")
        _same(t.glared_image(), G.glare(t.accum(), True), "glared_image, the accumulation under the default options")
    finally:
        t.close()


def test_bad_texels_and_threshold_edges_on_the_device():
    """NaN, +inf, -inf, negative and -0 texels, and greys whose luminance is the threshold, one ulp below and one ulp above it."""
    t, _ = _context(33, 130)
    try:
        t.glare(True)
        for levels in (1, 5, 8):
            for threshold in (0.0, 0.5):
                img = G.odd_frame(33, 130, 100 + levels)
                opt = G.options(1.0, threshold, levels, _weights(levels))
                got = _call(t, img, opt, np.empty_like(img))
                _same(got, G.glare(img, False, opt), "odd texels, levels %d threshold %g" % (levels, threshold))
                bad = ~np.isfinite(img[..., :3]).all(axis=-1)
                assert np.isfinite(got[~bad]).all() and (got[..., 3] == 1.0).all()
        for nominal in (0.5, 1.0, 3.0):
            img, thr = G.threshold_frame(33, 130, nominal)
            opt = G.options(1.0, thr, 5, G.HALVES)
            _same(_call(t, img, opt, np.empty_like(img)), G.glare(img, False, opt), "threshold %g" % thr)
        for value in (0.75, 1.0, 15.0):   # a constant frame comes back bit for bit
            img = np.full((130, 33, 4), value, np.float32)
            want = img.copy()
            want[..., 3] = 1.0
            _same(_call(t, img, G.options(0.37, 0.0, 5, G.HALVES), np.empty_like(img)), want, "constant %g" % value)
    finally:
        t.close()


def test_a_rendered_accumulation():
    """The default scene at 64x36, two passes of 2 spp: the device accumulation itself through pt_glare."""
    t, _ = _context(R.WIDTH, R.HEIGHT, spp=2)
    try:
        t.reserve_passes(2)
        t.render_passes(2)
        acc = t.accum()
        t.glare(True)
        for levels in G.LEVELS:
            for opt in _option_sets(levels):
                _same(t.glared_image(None, _abi_opt(opt)), G.glare(acc, True, opt), "levels %d" % levels)
        _same(t.glared_image(), G.glare(acc, True), "default options")
        assert np.array_equal(t.accum().view(np.uint32), acc.view(np.uint32))
    finally:
        t.close()


def test_more_level_1_tiles_than_the_down_kernels_grid():
    """THE GRIDS ARE CAPPED AT 2048 WORKGROUPS (the down kernel's tiles and the pixel kernels alike), hence 2048 x 1026: level 1 is
    1024 x 513 = 64 x 33 = 2112 tiles of 16 x 16, its last tile row being the down kernel's second trip, and the frame is the pixel
    kernels' fifth.  The whole output under eight levels; then every level on its own — all the weight on level k, so the output
    is that level brought back up — with the last 2^k rows and columns, which hold the level's last row and last column, compared."""
    import torch

    w, h = 2048, 1026
    rng = np.random.default_rng(12)
    lin = np.ones((h, w, 4), np.float32)
    lin[..., :3] = rng.random((h, w, 3), dtype=np.float32) * np.float32(4.0)
    lin[-1, :, :3] += np.float32(9.0)   # (the last row and the last column differ from what a clamped read of their neighbours gives)
    lin[:, -1, :3] += np.float32(5.0)
    t, _ = _context(w, h, use_torch=True)
    try:
        t.glare(True)
        dev = torch.from_numpy(lin).cuda()
        out = torch.empty_like(dev)
        x, b = G.bright(lin, False, 0.0)
        D = G.pyramid(b, 8)
        assert [d.shape[:2] for d in D[1:]] == [(513, 1024), (257, 512), (129, 256), (65, 128), (33, 64), (17, 32), (9, 16), (5, 8)]
        opt = G.options(1.0, 0.0, 8, _weights(8))
        ref = G.composite(x, b, G.spread(b, opt, D=D), 1.0)
        _same(_call(t, dev, opt, out).cpu().numpy(), ref, "2048x1026, eight levels")
        for k in range(1, 9):
            opt = G.options(1.0, 0.0, k, (0.0,) * (k - 1) + (1.0,))
            ref = G.composite(x, b, G.spread(b, opt, D=D), 1.0)
            _call(t, dev, opt, out)
            n = 2 ** k
            _same(out[-n:].cpu().numpy(), ref[-n:], "level %d alone, the last %d rows" % (k, n))
            _same(out[:, -n:].cpu().numpy(), ref[:, -n:], "level %d alone, the last %d columns" % (k, n))
            _same(out[:n, :n].cpu().numpy(), ref[:n, :n], "level %d alone, the first corner" % k)
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ the chain on a rendered frame
def test_config4_glared_metered_and_toned_against_the_chained_restatements(ora):
    """The closed room lit by a sphere of radiance 15, 96 x 96, two passes of 4 spp: pt_glare with the default options into a device
    buffer, pt_meter and pt_resolve_toned_rgba8 from that buffer, against glare_ref -> tone_ref ON THE ORACLE'S accumulation (the
    device accumulation is pinned to it here once more)."""
    import torch

    sc = scenes.config4(width=96, height=96, spp_per_pass=4, n_passes=2)
    acc, _ = ora.render(sc.spheres, sc.params, 2)
    t = PathTracer(96, 96)
    try:
        t.set_spheres(sc.spheres)
        t.set_params(sc.params)
        t.reserve_passes(2)
        t.render_passes(2)
        assert np.array_equal(t.accum().view(np.uint32), acc.view(np.uint32))
        t.glare(True)
        t.tone_mapping(True)
        dev = torch.empty((96, 96, 4), dtype=torch.float32, device="cuda")
        src = C.c_void_p(dev.data_ptr())
        t.glare_into(src)
        glared = G.glare(acc, True)
        _same(dev.cpu().numpy(), glared, "the glared frame")
        t.meter(src=src)
        rec, hist = t.exposure()
        ref_hist, ref_below = T.meter(glared, False)
        assert [int(x) for x in hist] == ref_hist and rec.below == ref_below
        ref = T.solve(ref_hist, ref_below)
        assert T.same_record(T.record_of(rec), ref), (T.record_of(rec), ref)
        clipped = {}
        for name, curve in (("reinhard", abi.PT_TONE_REINHARD), ("filmic", abi.PT_TONE_FILMIC)):
            got = t.toned_rgba8(abi.PtToneOptions(curve, 1, 0.0, 0.0), src=src)
            want = T.toned_rgba8(glared, False, curve, 1, ref["exposure"], ref["white"])
            assert np.array_equal(got, want), name
            clipped[name] = int((got[..., :3] == 255).sum())
        print("config 4, 96x96, 8 spp, default glare: exposure %g, white %g; channel values at 255: %r" % (rec.exposure, rec.white, clipped))
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ what the call leaves alone
def _snapshot(t):
    st = t.stats()
    rec, hist = t.exposure()
    return dict(accum=t.accum().view(np.uint32).copy(), err=t.error_state().view(np.uint32).copy(), stats=bytes(memoryview(st))[:],
                build=t.last_trace_build(), canvas=t.read_canvas().copy(), exposure=bytes(memoryview(rec))[:], hist=hist.copy())


def test_the_call_leaves_the_context_alone():
    """The accumulation's bits, the estimate, PtStats (first_pass shows in the next passes' bits), pt_last_trace_build, the exposure
    record and the canvas before and after each call; then two more passes give the bits of a context that never glared."""
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
        t.meter()
        t.glare(True)
        before = _snapshot(t)
        ext = G.random_frame(R.WIDTH, R.HEIGHT, 4, False)
        calls = [("pt_glare", lambda: t.glared_image()), ("pt_glare, host src", lambda: t.glared_image(ext, abi.PtGlareOptions(1.0, 0.5, 8, _weights(8)))),
                 ("PT_OPT_GLARE off", lambda: t.glare(False)), ("PT_OPT_GLARE on", lambda: t.glare(True)), ("pt_glare again", lambda: t.glared_image())]
        for name, call in calls:
            call()
            after = _snapshot(t)
            for k in before:
                same = np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k]
                assert same, "%s moved %s" % (name, k)
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


# ------------------------------------------------------------------------------------------------ refusals
def test_the_order_of_the_refusals():
    """Arguments and option values; then the option; then a band context; (the capture has its own test;) then what pt_resolve
    answers for the accumulation."""
    t, p = _context(R.WIDTH, R.HEIGHT)
    try:
        fn, err = t.lib.pt_glare, lambda: t.lib.pt_last_error(t._ctx)
        out = np.zeros((R.HEIGHT, R.WIDTH, 4), np.float32)
        po = out.ctypes.data_as(C.c_void_p)
        good = abi.PtGlareOptions()
        assert fn(None, None, C.byref(good), po) == abi.PT_ERR_INVALID
        assert fn(t._ctx, None, None, po) == abi.PT_ERR_INVALID and fn(t._ctx, None, C.byref(good), None) == abi.PT_ERR_INVALID
        nan = float("nan")
        bads = [abi.PtGlareOptions(strength=nan), abi.PtGlareOptions(strength=1.5), abi.PtGlareOptions(strength=-0.1), abi.PtGlareOptions(threshold=-1.0),
                abi.PtGlareOptions(threshold=nan), abi.PtGlareOptions(levels=0), abi.PtGlareOptions(levels=9),
                abi.PtGlareOptions(weights=(0.5, -0.25, 0.25, 0.25, 0.25, 0.0)), abi.PtGlareOptions(weights=(0.5, 0.25, nan, 0.25, 0.0, 0.0))]
        for bad in bads:   # the option is still off: the values are looked at first
            assert fn(t._ctx, None, C.byref(bad), po) == abi.PT_ERR_INVALID, (bad.strength, bad.threshold, bad.levels, list(bad.weight))
        unused = abi.PtGlareOptions(levels=3, weights=(0.5, 0.25, 0.25, nan, -1.0, float("inf"), nan, nan))
        assert fn(t._ctx, None, C.byref(good), po) == abi.PT_ERR_NOT_READY and b"PT_OPT_GLARE" in err()
        assert fn(t._ctx, None, C.byref(unused), po) == abi.PT_ERR_NOT_READY
        # a band context is refused once the option is on — before "nothing rendered yet", and whatever the source
        t.glare(True)
        q = p.copy()
        q.band_rows, q.band_index, q.band_count = 4, 1, 2
        t.set_params(q)
        rows = abi.local_rows(R.HEIGHT, 4, 1, 2)
        ext = G.random_frame(R.WIDTH, rows, 1, False)
        assert fn(t._ctx, None, C.byref(good), po) == abi.PT_ERR_INVALID and b"band" in err()
        assert fn(t._ctx, ext.ctypes.data_as(C.c_void_p), C.byref(good), po) == abi.PT_ERR_INVALID and b"band" in err()
        for bad in bads[:2]:
            assert fn(t._ctx, None, C.byref(bad), po) == abi.PT_ERR_INVALID and b"band" not in err()
        t.set_params(p)
        # the whole frame again: the accumulation answers as pt_resolve does, an external source needs no rendered frame
        assert fn(t._ctx, None, C.byref(good), po) == abi.PT_ERR_NOT_READY and b"nothing rendered yet" in err()
        assert t.lib.pt_resolve(t._ctx, po, 1) == abi.PT_ERR_NOT_READY
        ext = G.random_frame(R.WIDTH, R.HEIGHT, 2, False)
        _same(t.glared_image(ext, unused), G.glare(ext, False, G.options(0.15, 0.0, 3, (0.5, 0.25, 0.25))), "unused weights are not read")
        t.render_passes(1)
        _same(t.glared_image(), G.glare(t.accum(), True), "after a pass")
    finally:
        t.close()


def test_the_call_inside_a_stream_capture_is_refused():
    """PT_ERR_INVALID inside a capture, before anything is enqueued — also where "nothing rendered yet" would be the next answer."""
    import torch

    sc = scenes.default_scene(R.WIDTH, R.HEIGHT, spp=1, max_depth=6)
    ext = G.random_frame(R.WIDTH, R.HEIGHT, 6, False)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = PathTracer(R.WIDTH, R.HEIGHT, use_torch=True)  # binds the side stream as its launch stream
        t.set_spheres(sc.spheres)
        t.set_params(sc.params)
        t.glare(True)
        dev = torch.from_numpy(ext).cuda()
        out = torch.full((R.HEIGHT, R.WIDTH, 4), 3.0, dtype=torch.float32, device="cuda")
        torch.cuda.current_stream().synchronize()
        opt = abi.PtGlareOptions()
        codes = {}
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            codes["device src"] = (t.lib.pt_glare(t._ctx, C.c_void_p(dev.data_ptr()), C.byref(opt), C.c_void_p(out.data_ptr())), t.lib.pt_last_error(t._ctx))
            codes["accumulation"] = (t.lib.pt_glare(t._ctx, None, C.byref(opt), C.c_void_p(out.data_ptr())), t.lib.pt_last_error(t._ctx))
            t.render_passes(1)  # (something to capture)
    torch.cuda.synchronize()
    for name, (rc, msg) in codes.items():
        assert rc == abi.PT_ERR_INVALID and b"capture" in msg, (name, rc, msg)
    assert (out.cpu().numpy() == 3.0).all(), "refused before anything was launched"
    got = t.glared_image(dev)
    _same(got.cpu().numpy(), G.glare(ext, False), "after the capture")
    t.close()


# ------------------------------------------------------------------------------------------------ the option and the extent
def test_the_option_off_and_on_and_a_resize_between_two_calls():
    """Off: PT_ERR_NOT_READY; on again: the same bits.  pt_resize between two calls — to a larger and odd frame, then to a
    smaller one — and a repartition back from bands: the pyramid follows each time."""
    t, p = _context(R.WIDTH, R.HEIGHT)
    try:
        opt = G.options(0.6, 0.2, 8, _weights(8))
        o = _abi_opt(opt)
        ext = G.random_frame(R.WIDTH, R.HEIGHT, 21, False)
        ref = G.glare(ext, False, opt)
        out = np.empty_like(ext)
        po = out.ctypes.data_as(C.c_void_p)
        t.glare(True)
        _same(t.glared_image(ext, o), ref, "on")
        t.glare(False)
        assert t.lib.pt_glare(t._ctx, ext.ctypes.data_as(C.c_void_p), C.byref(o), po) == abi.PT_ERR_NOT_READY
        t.glare(True)
        t.glare(True)   # (twice is once)
        _same(t.glared_image(ext, o), ref, "off and on again")
        for (w, h) in ((131, 77), (33, 130), (5, 3)):
            t._check(t.lib.pt_resize(t._ctx, w, h))
            t.width, t.height, t.local_rows = w, h, h
            q = p.copy()
            q.width, q.height = w, h
            t.set_params(q)
            ext = G.random_frame(w, h, 22 + w, False)
            _same(t.glared_image(ext, o), G.glare(ext, False, opt), "after pt_resize to %dx%d" % (w, h))
            bands = q.copy()
            bands.band_rows, bands.band_index, bands.band_count = 1, 0, 3
            t.set_params(bands)
            t.set_params(q)
            _same(t.glared_image(ext, o), G.glare(ext, False, opt), "after a repartition and back at %dx%d" % (w, h))
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


def test_frame_loop_glares_ahead_of_the_tone_curve():
    """FrameLoop(mode="linear", tone=...): glare=None draws the canvas of the loop without the argument, byte for byte; with glare
    every tick's canvas is the chained restatement — glare_ref on the tick's accumulation, tone_ref's metering and solve after the
    record of the tick before, tone_ref's bytes."""
    from ray_tracer_webgl_amd.app import FrameLoop

    w, h, n = R.WIDTH, R.HEIGHT, 6
    meter = abi.PtMeterOptions(rate=0.25)
    tone = abi.PtToneOptions(abi.PT_TONE_FILMIC, 1, 0.0, 1.0)
    glare = abi.PtGlareOptions(0.5, 0.0, 4, (0.4, 0.3, 0.2, 0.1))
    gopt = G.options(0.5, 0.0, 4, (0.4, 0.3, 0.2, 0.1))
    today, none = FrameLoop(w, h, mode="linear", tone=(meter, tone)), FrameLoop(w, h, mode="linear", tone=(meter, tone), glare=None)
    glared = FrameLoop(w, h, mode="linear", tone=(meter, tone), glare=glare)
    try:
        a, b = _ticks(today, n), _ticks(none, n)
        for k in range(n):
            assert np.array_equal(a[k], b[k]), "tick %d: glare=None is the loop without it" % k
        glared.state.set_flags(is_paused=False)
        prev = None
        for k in range(n):
            assert glared.frame(100.0 + 16.5 * k)
            frame = G.glare(glared.tracer.accum(), True, gopt)
            hist, below = T.meter(frame, False)
            prev = T.solve(hist, below, dict(rate=0.25), prev)
            want = T.toned_rgba8(frame, False, abi.PT_TONE_FILMIC, 1, prev["exposure"], prev["white"])
            assert np.array_equal(glared.canvas, want), "tick %d with glare" % k
        assert T.same_record(T.record_of(glared.tracer.exposure()[0]), prev)
        assert not np.array_equal(a[-1], glared.canvas)
        with pytest.raises(AssertionError):
            FrameLoop(w, h, mode="linear", glare=glare)   # (linear radiance needs a tone curve to be drawn)
    finally:
        for loop in (today, none, glared):
            loop.close()
