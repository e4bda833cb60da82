"""The kernels that turn traced sums into pictures — pt_resolve_kernel, pt_resolve_rgba8_kernel, pt_blend_rgba8_kernel,
pt_frame_blend_kernel, pt_frames_blend_kernel, pt_accumulate_kernel — on operands at and beyond their guards, against
the plain numpy restatement of their statements (tests/readout_ref.py, itself held against the oracle and counted for
coverage of every guard by tests/test_readout_ref.py, without a GPU).

What the trace tests never vary is varied here: the divisor is each pixel's own count (whole counts, 2^24 and beyond,
and counts that are none: 0, -0, negative, subnormal, infinite, NaN); colours sit next to every rounding edge of unorm8
and on the far side of sqrt_core's and div_core's ranges; the blend rule flips in the middle of a group of frames;
radiance is non-finite on its whole way from the trace kernel to the texture.  Floats are compared as bit patterns
except where both sides are NaN, bytes outright; no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import readout_ref as R
from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer

pytestmark = pytest.mark.gpu


def _same_bytes(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref), "%s: %d bytes differ, first at %s" % (what, int((got != ref).sum()), np.argwhere(got != ref)[:3].tolist())


def _context(w, h):
    """A context of the given size with uniforms in place (the read-out and blend entry points need no scene)."""
    sc = scenes.default_scene(R.WIDTH, R.HEIGHT, spp=1, max_depth=6)
    p = sc.params.copy()
    p.width, p.height = w, h
    t = PathTracer(w, h)
    t.set_spheres(sc.spheres)
    t.set_params(p)
    return t, p


def _check_read_outs(t, acc, what):
    t.load_accum(acc)
    assert R.same_floats(t.accum(), acc), "%s: the loaded buffer is not handed back as it was" % what
    for gamma in (0, 1):
        got = t.resolve(bool(gamma))
        ref = R.resolve(acc, gamma)
        assert R.same_floats(got, ref), "%s, pt_resolve gamma %d: %s" % (what, gamma, R.first_difference(got, ref))
        _same_bytes(t.resolve_rgba8(bool(gamma)), R.resolve_rgba8(acc, gamma), "%s, pt_resolve_rgba8 gamma %d" % (what, gamma))


# ------------------------------------------------------------------------------------------------ resolve kernels
def test_resolve_kernels_on_loaded_buffers_with_a_count_per_pixel():
    """pt_load_accum, then pt_resolve and pt_resolve_rgba8 with gamma 0 and 1, on six 64x36 buffers: every edge colour of
    readout_ref.edge_colours() under a count whose reciprocal is exact, one whose is not and one that is none, the counts
    changing from pixel to pixel."""
    t, _ = _context(R.WIDTH, R.HEIGHT)
    for i, acc in enumerate(R.edge_accums()):
        _check_read_outs(t, acc, "edge buffer %d" % i)
    t.close()


@pytest.mark.parametrize("w,h,seed", [(61, 7, 7), (1, 1, 8), (3, 5, 9)])
def test_resolve_kernels_on_other_sizes(w, h, seed):
    """427 pixels (no multiple of the block, and more than one), a single pixel, fifteen."""
    t, _ = _context(w, h)
    _check_read_outs(t, R.small_accum(h, w, seed), "%dx%d" % (w, h))
    t.close()


def test_load_accum_checks_the_count_of_the_first_and_last_pixel_only():
    """pt_load_accum takes a checkpoint whose first and last pixel carry the same whole count below 2^24 and refuses any other with
    PT_ERR_INVALID: so the buffers above keep 1 there (the nearest accepted value) and vary everything between.  A count of 0 there
    loads, and the read-out then has nothing to show (PT_ERR_NOT_READY)."""
    t, _ = _context(R.WIDTH, R.HEIGHT)
    good = R.edge_accums()[0]
    t.load_accum(good)
    for w0 in (np.nan, -1.0, -0.5, 2.0 ** 24, 0.5, np.inf, 3e38):
        bad = good.copy()
        bad[0, 0, 3] = bad[-1, -1, 3] = w0
        rc = t.lib.pt_load_accum(t._ctx, bad.ctypes.data_as(C.c_void_p), bad.nbytes)
        assert rc == abi.PT_ERR_INVALID and b"is not a count" in t.lib.pt_last_error(t._ctx), (w0, rc)
    bad = good.copy()
    bad[-1, -1, 3] = 2.0
    rc = t.lib.pt_load_accum(t._ctx, bad.ctypes.data_as(C.c_void_p), bad.nbytes)
    assert rc == abi.PT_ERR_INVALID and b"sample counts differ across the buffer" in t.lib.pt_last_error(t._ctx)
    assert R.same_floats(t.accum(), good)   # a refused checkpoint leaves the context as it was
    assert R.same_floats(t.resolve(False), R.resolve(good, 0))
    empty = good.copy()
    empty[0, 0, 3] = empty[-1, -1, 3] = 0.0
    t.load_accum(empty)
    out = np.zeros((R.HEIGHT, R.WIDTH, 4), np.float32)
    assert t.lib.pt_resolve(t._ctx, out.ctypes.data_as(C.c_void_p), 1) == abi.PT_ERR_NOT_READY
    assert b"nothing rendered yet" in t.lib.pt_last_error(t._ctx)
    t.close()


# ------------------------------------------------------------------------------------------------ the blend
def test_blend_rgba8_with_a_count_per_pixel():
    """The rule list of test_temporal_blend_rgba8_at_the_edges_of_its_fast_forms on a buffer whose counts vary from pixel to pixel."""
    t, p = _context(R.WIDTH, R.HEIGHT)
    acc = R.blend_accum()
    prev = R.seed_texture(R.HEIGHT, R.WIDTH, 45, every_byte=True)
    t.load_accum(acc)
    for rc, avg, wt in R.BLEND_RULES:
        q = p.copy()
        q.render_count, q.should_average, q.last_frame_weight = rc, avg, wt
        t.set_params(q)
        _same_bytes(t.blend_rgba8(prev), R.blend_rgba8(acc, prev, rc, avg, wt), "rule %r" % ((rc, avg, wt),))
    t.close()


# ------------------------------------------------------------------------------------------------ frame kernels
class _FramePair:
    """Two contexts of one scene: one replays groups of frames (pt_render_frames), one is stepped tick by tick by the host."""

    def __init__(self, spheres, p):
        self.p = p
        self.ctx = []
        for _ in range(2):
            t = PathTracer(p.width, p.height)
            t.set_spheres(spheres)
            t.set_params(p)
            self.ctx.append(t)
        self.rows = self.ctx[0].local_rows

    def run(self, s, seeds):
        """(canvas, texture 0, texture 1) of the grouped series and of the single ticks."""
        grouped, single = self.ctx
        for t in self.ctx:
            t.write_texture(0, seeds[0])
            t.write_texture(1, seeds[1])
        grouped.set_params(R.series_params(self.p, s))
        grouped.render_frames(s["e0"], s["max_rc"], s["n"])
        for k in range(s["n"]):
            single.set_params(R.tick_params(self.p, s, k))
            single.render_frame(s["e0"] + k)
        return [(t.read_canvas(), t.read_texture(0), t.read_texture(1)) for t in self.ctx]

    def close(self):
        for t in self.ctx:
            t.close()


@pytest.fixture(scope="module")
def frame_sets(ora):
    """Per row partition: the two contexts and the oracle's pass of every frame (it depends on the clock alone)."""
    out = {}
    n = max(s["n"] for s in R.FRAME_SERIES)
    for band in (None, (8, 1, 3)):
        spheres, p = R.frame_scene(band)
        out[band] = (_FramePair(spheres, p), R.oracle_passes(ora, spheres, p, n))
    yield out
    for pair, _ in out.values():
        pair.close()


def _check_series(pair, passes, s, seeds):
    got_grouped, got_single = pair.run(s, seeds)
    ref = R.frame_chain(passes[:s["n"]], seeds[0], seeds[1], s["rc0"], s["max_rc"], s["e0"], s["avg"], s["lfw"])
    for name, g, o, r in zip(("canvas", "texture 0", "texture 1"), got_grouped, got_single, ref):
        _same_bytes(o, r, "%s: single ticks vs the restatement's chain, %s" % (s["name"], name))
        _same_bytes(g, r, "%s: grouped frames vs the restatement's chain, %s" % (s["name"], name))
        _same_bytes(g, o, "%s: grouped frames vs single ticks, %s" % (s["name"], name))
    if not s["avg"]:
        _same_bytes(got_grouped[1], seeds[0], "texture 0 untouched")
        _same_bytes(got_grouped[2], seeds[1], "texture 1 untouched")


@pytest.mark.parametrize("s", R.FRAME_SERIES, ids=[s["name"] for s in R.FRAME_SERIES])
def test_frame_kernels_on_the_edges_of_the_rule(frame_sets, s):
    """pt_render_frames (groups of 16 and 4, then single frames) against pt_render_frame tick by tick with host-stepped uniforms and
    against the restatement's chain fed by the oracle's pass of each frame: canvas and both textures.  The series put the flips
    of the rule inside a group: averaging switching on, the total leaving div_core's range, the clamp at max_render_count, the
    64-bit sum, the parity across 2^32, weights on the far side of every guard."""
    pair, passes = frame_sets[s["band"]]
    assert pair.rows == (12 if s["band"] else R.HEIGHT)
    seeds = [R.seed_texture(pair.rows, R.WIDTH, 50), R.seed_texture(pair.rows, R.WIDTH, 51)]
    _check_series(pair, passes, s, seeds)


def test_frame_entry_points_take_every_count_and_weight():
    """Nothing of the frame series is validated away: pt_render_frames clamps max_render_count to 2^31 - 1 and takes 0; pt_set_params takes any
    last_frame_weight.  (Were one refused, its series would have failed above with the refusal's message.)"""
    t, p = _context(R.WIDTH, R.HEIGHT)
    q = p.copy()
    q.render_count, q.last_frame_weight = R.INT_MAX, float("nan")
    assert t.lib.pt_set_params(t._ctx, C.byref(q)) == abi.PT_OK
    assert t.lib.pt_render_frames(t._ctx, 0xFFFFFFFF, 0xFFFFFFFF, 1) == abi.PT_OK
    assert t.lib.pt_render_frames(t._ctx, 0, 0, 0) == abi.PT_OK
    t.synchronize()
    t.close()


# ------------------------------------------------------------------------------------------------ extreme radiance
@pytest.mark.parametrize("spp", [1, 2])
def test_extreme_radiance_from_the_trace_kernels_to_the_textures(ora, spp):
    """Emitters of 0, subnormal, 2^-100 ... 3e38, +inf, NaN, -0 and -1 behind a black sky: (a) three passes through the trace
    kernel, the slab and pt_accumulate_kernel's ordered adds equal the oracle's; (b) through the small-list and the scalar
    kernels alike; (d) their RGBA8 read-out; (c) nine averaging frames, grouped and tick by tick, equal the restatement's chain."""
    spheres, p = R.extreme_scene(spp)
    ref, seg = ora.render(spheres, p, 3)
    for path in (None, abi.PT_GEOM_SMALL, abi.PT_GEOM_SCALAR):
        t = PathTracer(p.width, p.height)
        if path is not None:
            t.set_geometry_path(path)
        t.set_spheres(spheres)
        t.set_params(p)
        t.reserve_passes(3)
        t.render_passes(3)
        got = t.accum()
        assert R.same_floats(got, ref), "path %r: %s" % (path, R.first_difference(got, ref))
        st = t.stats()
        assert st.segments == seg and (path is None or st.geometry_path == path)
        for gamma in (0, 1):
            _same_bytes(t.resolve_rgba8(bool(gamma)), R.resolve_rgba8(ref, gamma), "rgba8 read-out, gamma %d" % gamma)
            assert R.same_floats(t.resolve(bool(gamma)), R.resolve(ref, gamma))
        t.close()
    s = R.EXTREME_SERIES
    pair = _FramePair(spheres, p)
    seeds = [R.seed_texture(p.height, p.width, 60), R.seed_texture(p.height, p.width, 61)]
    _check_series(pair, R.oracle_passes(ora, spheres, p, s["n"]), s, seeds)
    pair.close()
