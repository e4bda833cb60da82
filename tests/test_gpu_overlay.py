"""The debug overlay (pt_set_debug_overlay; static/shader.frag:307-318) on the device, bit for bit.

Every comparison is equal uint32 views of the accumulation buffer (or equal bytes of the canvas) against the test-side
restatement tests/overlay_ref.c — the oracle's pass rebuilt from its exported pieces with the overlay test alive, itself
pinned to the oracle with the overlay off by tests/test_overlay_cpu.py, which also shows that every case below has a dot, an
outline and an overlay-ended path after a bounce — and PtStats.segments equal to the restatement's count.  Tolerance: none.

  (a) the cases      State::default with the State's own cursor and selection through the small-list kernel; the cover scene
                     (a one-layer grid) and a 1 500-sphere field (several layers; uuids that are not indices) through the
                     scalar walk, the hierarchy and the grid; the closed room with its EMISSIVE sphere selected.  Several passes
                     in one launch and one pass per launch.
  (b) every build    each of the twelve kernels of csrc/pt_kernels_debug.hip is launched and compared.
  (c) bands          a two-band row partition.
  (d) off again      enable = 0 after enable = 1 gives the bits of a context that never enabled it (the oracle's).
  (e) exclusion      overlay and roulette refuse each other with PT_ERR_INVALID.
  (f) frames         pt_render_frame / pt_render_frames: the canvas is ora_blend_rgba8 of the restatement's pass, a changed
                     selection shows in the next series (its graphs were captured again), FrameLoop(debugging=True) in flight.
"""
import numpy as np
import pytest

import overlay_ref as R
from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer, PtError
from test_gpu_fuzz import random_scene
from trace_builds import build_of

pytestmark = pytest.mark.gpu

KERNELS = ["small_t0_dbg", "small_t1_dbg", "small_t2_dbg", "small_t3_dbg", "scalar_dbg", "scalar_nolds_dbg", "bvh_dbg", "bvh_nodes_dbg",
           "bvh_gmem_dbg", "grid_dbg", "grid_cells_dbg", "grid_gmem_dbg"]
REACHED = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (
            what, len(bad), g.size, tuple(bad[0]), np.asarray(got)[tuple(bad[0])], np.asarray(ref)[tuple(bad[0])]))


def kernel_of(t):
    """the overlay kernel the last launch of this context was (kTraceKernels of csrc/pt_trace_table.hpp, by row)"""
    assert t.last_trace_build() == abi.BUILD_DEBUG_OVERLAY
    st = t.stats()
    if st.geometry_path == abi.PT_GEOM_LDS:
        raise AssertionError("the overlay through geometry path %d" % st.geometry_path)
    return build_of(st, "_dbg")


def context(sph, w, h, path, overlay):
    t = PathTracer(w, h)
    t.set_geometry_path(path)
    t.set_spheres(sph)
    if overlay is not None:
        t.set_debug_overlay(True, overlay[0], overlay[1])
    return t


def gpu(t, p, n_passes, per_launch=None):
    per_launch = per_launch or n_passes
    t.set_params(p)
    t.reserve_passes(per_launch)
    t.reset()
    done = 0
    while done < n_passes:
        q = p.copy()
        q.first_pass = p.first_pass + done
        t.set_params(q)
        n = min(per_launch, n_passes - done)
        t.render_passes(n)
        done += n
    return t.accum(), t.stats()


# ------------------------------------------------------------------------------------------------ (a) the cases
@pytest.mark.parametrize("name", ["default", "cover", "field", "room"])
def test_overlay_cases_equal_the_restatement(ora, name):
    c = R.CASES[name]()
    p, w, h = c.params, c.params.width, c.params.height
    ref, tally, flags = R.render(c.spheres, p, c.n_passes, c.overlay)
    plain, seg_plain = ora.render(c.spheres, p, c.n_passes)
    assert not np.array_equal(bits(ref), bits(plain))
    # (paths end early — except in the room, where the selected sphere is the light: a path that reaches it ends there anyway)
    assert (tally["segments"] == seg_plain) if name == "room" else (tally["segments"] < seg_plain)
    for path in c.paths:
        t = context(c.spheres, w, h, path, c.overlay)
        try:
            got, st = gpu(t, p, c.n_passes)
            assert st.geometry_path == path, (name, path, st.geometry_path)
            kernel = kernel_of(t)
            assert_bit_equal(got, ref, "%s through %s, %d passes in one launch" % (name, kernel, c.n_passes))
            assert st.segments == tally["segments"], (name, kernel, st.segments, tally["segments"])
            got, st = gpu(t, p, c.n_passes, per_launch=1)  # pt_render_passes against single passes
            assert st.render_launches == c.n_passes
            assert_bit_equal(got, ref, "%s through %s, one pass per launch" % (name, kernel))
            assert st.segments == tally["segments"]
            if path == abi.PT_GEOM_GRID:
                print("%s: grid %s, build %d, flat walk without the overlay %d" % (name, list(st.grid_cells), st.grid_kernel_build, st.grid_walk_flat))
                assert st.grid_cells[1] == (1 if name == "cover" else st.grid_cells[1])  # the cover scene: one layer of cells
                if name == "field":
                    assert st.grid_cells[1] > 1
            REACHED.setdefault(kernel, []).append(name)
        finally:
            t.close()


# ------------------------------------------------------------------------------------------------ (b) every build
def _small(n, seed):
    def make():
        sc = random_scene(np.random.default_rng(83000 + seed), n, 96, 54, 2, 8, 2)
        sc.spheres["uuid"] = (50 + 11 * np.arange(len(sc.spheres))).astype(np.int32)
        pick = R.center_pick(sc.spheres, sc.params)
        if pick is None:
            k = int(np.argmax(np.abs(sc.spheres["radius"])))
            pick = (int(sc.spheres["uuid"][k]), tuple(float(x) for x in sc.spheres["center"][k]))
        return R.Case("small%d" % n, sc.spheres, sc.params, sc.n_passes, pick, [abi.PT_GEOM_SMALL])
    return make


def _field(n, path):
    return lambda: R.field_case(n, 48, 27, True, [path])


BUILDS = [
    ("small_t0_dbg", _small(12, 3)), ("small_t1_dbg", _small(9, 0)), ("small_t2_dbg", _small(10, 1)), ("small_t3_dbg", _small(11, 2)),
    ("scalar_nolds_dbg", _field(12000, abi.PT_GEOM_SCALAR)),
    ("bvh_nodes_dbg", _field(3000, abi.PT_GEOM_BVH)), ("bvh_gmem_dbg", _field(20000, abi.PT_GEOM_BVH)),
    ("grid_cells_dbg", _field(10000, abi.PT_GEOM_GRID)), ("grid_gmem_dbg", _field(60000, abi.PT_GEOM_GRID)),
]


@pytest.mark.parametrize("case", BUILDS, ids=[b[0] for b in BUILDS])
def test_the_other_overlay_builds_equal_the_restatement(case):
    """the builds the four cases above do not reach: the small-list remainders, and the kernels of scenes beyond the LDS"""
    kernel, make = case
    c = make()
    p = c.params
    ref, tally, flags = R.render(c.spheres, p, c.n_passes, c.overlay)
    assert tally["blue_paths"] + tally["red_paths"] > 0, kernel
    t = context(c.spheres, p.width, p.height, c.paths[0], c.overlay)
    try:
        got, st = gpu(t, p, c.n_passes)
        assert kernel_of(t) == kernel, (kernel, kernel_of(t), st.geometry_path, st.n_spheres, st.bvh_nodes, st.bvh_slots, st.grid_kernel_build)
        assert_bit_equal(got, ref, kernel)
        assert st.segments == tally["segments"], (kernel, st.segments, tally["segments"])
        REACHED.setdefault(kernel, []).append(c.name)
    finally:
        t.close()


def test_every_overlay_kernel_was_reached():
    """(runs after the tests above) each of the twelve kernels of csrc/pt_kernels_debug.hip was launched and compared"""
    print("overlay kernels reached\n" + "\n".join("  %-18s %s" % (k, "; ".join(REACHED.get(k, [])) or "-") for k in KERNELS))
    assert sorted(REACHED) == sorted(KERNELS), sorted(set(KERNELS) - set(REACHED))


# ------------------------------------------------------------------------------------------------ (c) bands
def test_two_band_row_partition():
    c = R.default_case()
    whole, tally, _ = R.render(c.spheres, c.params, c.n_passes, c.overlay)
    seg = 0
    for r in range(2):
        q = c.params.copy()
        q.band_rows, q.band_index, q.band_count = 4, r, 2
        ref, tb, _ = R.render(c.spheres, q, c.n_passes, c.overlay)
        t = context(c.spheres, q.width, q.height, abi.PT_GEOM_SMALL, c.overlay)
        try:
            got, st = gpu(t, q, c.n_passes)
            ys = abi.owned_rows(q.height, 4, r, 2)
            assert got.shape[0] == len(ys)
            assert_bit_equal(got, ref, "band %d of 2 against the banded restatement" % r)
            assert_bit_equal(got, whole[ys], "band %d of 2 against the rows of the whole frame" % r)
            assert st.segments == tb["segments"]
            seg += st.segments
        finally:
            t.close()
    assert seg == tally["segments"]


# ------------------------------------------------------------------------------------------------ (d) off again
@pytest.mark.parametrize("name,path", [("default", abi.PT_GEOM_SMALL), ("cover", abi.PT_GEOM_GRID), ("cover", abi.PT_GEOM_LDS)])
def test_disabling_restores_the_plain_kernels_and_bits(ora, name, path):
    c = R.CASES[name]()
    p = c.params
    plain, seg = ora.render(c.spheres, p, c.n_passes)
    ref, tally, _ = R.render(c.spheres, p, c.n_passes, c.overlay)
    never = context(c.spheres, p.width, p.height, path, None)
    t = context(c.spheres, p.width, p.height, path, c.overlay)
    try:
        want, st0 = gpu(never, p, c.n_passes)
        assert never.last_trace_build() == abi.BUILD_PLAIN and st0.geometry_path == path
        got, st = gpu(t, p, c.n_passes)
        assert t.last_trace_build() == abi.BUILD_DEBUG_OVERLAY
        # (the LDS list walk has no overlay build: such a context renders through the scalar walk meanwhile)
        assert st.geometry_path == (abi.PT_GEOM_SCALAR if path == abi.PT_GEOM_LDS else path)
        assert_bit_equal(got, ref, "%s, overlay on" % name)
        t.set_debug_overlay(False)
        got, st = gpu(t, p, c.n_passes)
        assert t.last_trace_build() == abi.BUILD_PLAIN and st.geometry_path == path
        assert_bit_equal(got, want, "%s, overlay off again against a context that never enabled it" % name)
        assert_bit_equal(got, plain, "%s, overlay off again against the oracle" % name)
        assert st.segments == st0.segments == seg
        t.set_debug_overlay(True, *c.overlay)  # ... and on again
        got, st = gpu(t, p, c.n_passes)
        assert_bit_equal(got, ref, "%s, overlay on again" % name)
        assert st.segments == tally["segments"]
    finally:
        t.close()
        never.close()


# ------------------------------------------------------------------------------------------------ (e) exclusion
def test_overlay_and_roulette_exclude_each_other():
    c = R.default_case()
    t = context(c.spheres, c.params.width, c.params.height, abi.PT_GEOM_SMALL, None)
    try:
        t.set_russian_roulette(3)
        with pytest.raises(PtError) as e:
            t.set_debug_overlay(True, *c.overlay)
        assert e.value.code == abi.PT_ERR_INVALID and "ROULETTE" in str(e.value)
        t.set_debug_overlay(False)  # turning it off is always allowed
        t.set_russian_roulette(0)
        t.set_debug_overlay(True, *c.overlay)
        with pytest.raises(PtError) as e:
            t.set_russian_roulette(3)
        assert e.value.code == abi.PT_ERR_INVALID and "overlay" in str(e.value)
        t.set_russian_roulette(0)  # (0 = off: no conflict)
        ref, tally, _ = R.render(c.spheres, c.params, c.n_passes, c.overlay)
        got, st = gpu(t, c.params, c.n_passes)  # the refused calls left the overlay in place
        assert_bit_equal(got, ref, "after the refused calls")
        t.set_count_work(True)
        with pytest.raises(PtError) as e:
            t.render_passes(1)
        assert e.value.code == abi.PT_ERR_INVALID
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (f) frames
def _simulate(ora, sph, p, overlay, n, even_odd0, max_rc, tex):
    """n ticks of pt_render_frames' contract: frame k is one pass at u_time = time + float(first_pass + k) * time_step with
    render_count = min(render_count + k, max) blended into tex[(even_odd0 + k) % 2]; returns the last canvas"""
    canvas = None
    for k in range(n):
        q = p.copy()
        q.first_pass = p.first_pass + k
        q.render_count = min(p.render_count + k, max_rc)
        acc, _, _ = R.render(sph, q, 1, overlay)
        canvas = ora.blend_rgba8(acc, q.samples_per_pixel, q, tex[(even_odd0 + k + 1) % 2])
        if q.should_average:
            tex[(even_odd0 + k) % 2] = canvas
    return canvas


def test_frames_and_a_changed_selection(ora):
    c = R.default_case()
    w, h = c.params.width, c.params.height
    p = c.params.copy()
    p.samples_per_pixel, p.time, p.time_step, p.first_pass = 2, 100.0, 16.5, 0
    p.render_count, p.should_average, p.last_frame_weight = 1, 1, 1.0
    t = context(c.spheres, w, h, abi.PT_GEOM_SMALL, c.overlay)
    try:
        t.set_params(p)
        t.clear_textures()
        tex = [np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 4), np.uint8)]
        # one tick: the canvas of a first frame is the resolve of the restatement's pass
        t.render_frame(1)
        acc, _, _ = R.render(c.spheres, p, 1, c.overlay)
        first = _simulate(ora, c.spheres, p, c.overlay, 1, 1, 0x7fffffff, tex)
        assert np.array_equal(first, ora.resolve_rgba8(acc, p.samples_per_pixel, True))
        assert np.array_equal(t.read_canvas(), first), "pt_render_frame"
        assert (first[..., 2] == 255).sum() >= 20 and kernel_of(t) == "small_t1_dbg"
        # a series of five (a group of four and a single frame) replayed from graphs
        q = p.copy()
        q.render_count = 2
        t.set_params(q)
        want = _simulate(ora, c.spheres, q, c.overlay, 5, 2, 100000, tex)
        t.render_frames(2, 100000, 5)
        assert np.array_equal(t.read_canvas(), want), "pt_render_frames"
        assert np.array_equal(t.read_texture(0), tex[0]) and np.array_equal(t.read_texture(1), tex[1])
        # another selection and cursor (the left metal sphere): the next series must show it
        other = (2, (-1.1, 0.0, -0.5))
        t.set_debug_overlay(True, *other)
        q.render_count = 7
        t.set_params(q)
        tex_same = [x.copy() for x in tex]
        want = _simulate(ora, c.spheres, q, other, 5, 7, 100000, tex)
        stale = _simulate(ora, c.spheres, q, c.overlay, 5, 7, 100000, tex_same)
        assert not np.array_equal(want, stale)
        t.render_frames(7, 100000, 5)
        assert np.array_equal(t.read_canvas(), want), "pt_render_frames after the selection changed"
        # ... and off: the plain kernels' frames
        t.set_debug_overlay(False)
        q.render_count = 12
        t.set_params(q)
        want = None
        for k in range(5):
            r = q.copy()
            r.first_pass, r.render_count = k, 12 + k
            acc, _ = ora.render(c.spheres, r, 1)
            want = ora.blend_rgba8(acc, r.samples_per_pixel, r, tex[(12 + k + 1) % 2])
            tex[(12 + k) % 2] = want
        t.render_frames(12, 100000, 5)
        assert np.array_equal(t.read_canvas(), want), "pt_render_frames with the overlay off again"
        assert t.last_trace_build() == abi.BUILD_PLAIN
    finally:
        t.close()


def test_frame_loop_with_debugging_in_flight(ora):
    """FrameLoop(debugging=True) with 's' held: every tick moves the camera, the State picks again, the tick's three overlay
    uniforms go to the context before pt_render_frame.  A second State, stepped the same way, supplies the expectation."""
    from ray_tracer_webgl_amd.app import FrameLoop
    from ray_tracer_webgl_amd.state import State

    w, h, n = 160, 88, 6
    loop = FrameLoop(w, h, mode="reference", debugging=True)
    chk = State(w, h)
    try:
        for st in (loop.state, chk):
            st.set_flags(is_paused=False)
            st.set_quality(2, 8)
            st.set_keys(abi.KEY_S | abi.KEY_D)
        chk.set_debugging(True)
        loop.tracer.set_geometry_path(abi.PT_GEOM_SMALL)
        spheres = chk.spheres()
        tex = [np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 4), np.uint8)]
        cursors = set()
        for i in range(n):
            now = 100.0 + 16.5 * i
            assert loop.frame(now) is True
            chk.update_position(now if i == 0 else 16.5)
            chk.update_render_globals()
            v, p = chk.view(), chk.to_params(now)
            en, sel, cur = chk.debug_overlay()
            assert en and sel == 1
            cursors.add(cur)
            acc, tally, flags = R.render(spheres, p, 1, (sel, cur))
            assert (flags & 1).any() and tally["blue_paths"] > 0
            expect = ora.blend_rgba8(acc, p.samples_per_pixel, p, tex[(v.even_odd_count + 1) % 2])
            tex[v.even_odd_count % 2] = expect
            assert np.array_equal(loop.canvas, expect), "tick %d" % i
            assert kernel_of(loop.tracer) == "small_t1_dbg"
        assert len(cursors) == n  # the cursor moved with the camera
        # the keys released: a series of ticks is one pt_render_frames call with the overlay's uniforms baked into its graphs
        loop.state.set_keys(0)
        chk.set_keys(0)
        first = 100.0 + 16.5 * n
        assert loop.frames(5, first, 16.5) == 5
        for k in range(5):
            now = first + 16.5 * k
            chk.update_position(16.5)
            chk.update_render_globals()
            v, p = chk.view(), chk.to_params(now)
            en, sel, cur = chk.debug_overlay()
            acc, _, _ = R.render(spheres, p, 1, (sel, cur))
            expect = ora.blend_rgba8(acc, p.samples_per_pixel, p, tex[(v.even_odd_count + 1) % 2])
            tex[v.even_odd_count % 2] = expect
        assert np.array_equal(loop.canvas, expect), "replayed frames"
    finally:
        loop.close()
        chk.close()
