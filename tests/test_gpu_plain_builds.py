"""The plain column of kTraceKernels (csrc/pt_trace_table.hpp) — the fourteen kernels that ship and that bench.py times — and the five
measuring twins, build by build and bit for bit.

The roulette, overlay and feature columns each have such a matrix (test_gpu_roulette_exact.py, test_gpu_overlay.py,
test_gpu_features.py); the plain kernels were covered by the tests written as each kernel appeared, and nothing checked that
every one of them is reached — pt_trace_kernel_bvh_gmem was not, nor the LDS list walk with its 1024-thread workgroup.  Here
every row gets a scene that is known to reach it, at a size whose WHOLE frame the CPU oracle renders, with the lens on and
PT_TIME_STEP_DECORRELATED; the tolerance is none: equal uint32 views of the accumulation buffer (NaNs by bit pattern) and
equal segment counts.

  (a) whole frame   every pass in one launch against the oracle, then one pass per launch: the same bits and segments;
  (b) row bands     three bands of band_rows = 4, a context each (K.band_count > 1 in the item decode, csrc/pt_refill.hpp):
                    each band is the rows of the whole frame, band 1 is the oracle's banded render, the segments add up;
  (c) the twin      PT_OPT_COUNT_WORK: the same bits and segments from the measuring twin (bench.py's roofline tallies come
                    from it), or from the plain kernel again where the row has no twin;
  (d) frames        pt_render_frames (a group of four frames traced as the four passes of one launch, and a single frame:
                    frame_k in the item decode) against five pt_render_frame calls with host-made uniforms — canvas, both
                    textures, segments —, and the tick-by-tick canvas against the oracle's simulation of the reference's loop.
Which kernel a launch was is read from PtStats (tests/trace_builds.py) after EVERY launch and collected in REACHED; the last
test fails unless all fourteen rows and all five twins were reached, and names the missing ones.
"""
import os

import numpy as np
import pytest

from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer
from test_gpu_fuzz import random_scene
from trace_builds import ROWS, TWINS, grid_staging, row_of, twin_of

pytestmark = pytest.mark.gpu

ORACLE_THREADS = min(16, os.cpu_count() or 1)
REACHED = {}  # row or twin -> what was compared through it


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (
            what, len(bad), g.size, tuple(bad[0]), np.asarray(got)[tuple(bad[0])], np.asarray(ref)[tuple(bad[0])]))


def with_lens_and_step(p):
    p = p.copy()
    p.time_step = abi.PT_TIME_STEP_DECORRELATED
    if p.lens_radius == 0.0:
        p.lens_radius = 0.03
    return p


def small_list(n, seed):
    return lambda: random_scene(np.random.default_rng(47000 + seed), n, 96, 54, 2, 8, 3)


def cover():
    return scenes.config2(96, 54, 2, 3, 8)


def field(n):
    return lambda: scenes.config5(64, 36, 2, 2, 8, n=n)


# (row, scene, forced geometry path, workgroup of the list walk or None)
BUILDS = [
    ("small_t0", small_list(12, 3), abi.PT_GEOM_SMALL),
    ("small_t1", small_list(9, 0), abi.PT_GEOM_SMALL),
    ("small_t2", small_list(10, 1), abi.PT_GEOM_SMALL),
    ("small_t3", small_list(11, 2), abi.PT_GEOM_SMALL),
    ("list_lds", cover, abi.PT_GEOM_LDS),           # 256 threads
    ("list_lds", field(3000), abi.PT_GEOM_LDS),     # LDS copy over 40 KiB: 1024 threads (list_block_threads)
    ("scalar", cover, abi.PT_GEOM_SCALAR),
    ("scalar_nolds", field(12000), abi.PT_GEOM_SCALAR),
    ("bvh", cover, abi.PT_GEOM_BVH),
    ("bvh_nodes", field(5000), abi.PT_GEOM_BVH),    # (well inside the row: tests/test_gpu_hierarchy_edges.py goes to its ends)
    ("bvh_gmem", field(20000), abi.PT_GEOM_BVH),
    ("grid", cover, abi.PT_GEOM_GRID),              # one layer of cells: the two-axis walk
    ("grid_layers", field(1500), abi.PT_GEOM_GRID),
    ("grid_cells", field(10000), abi.PT_GEOM_GRID),
    ("grid_gmem", field(60000), abi.PT_GEOM_GRID),
]


def oracle(ora, sph, p, n_passes):
    return ora.render(sph, p, n_passes, nthreads=ORACLE_THREADS)


def context(sph, w, h, path):
    t = PathTracer(w, h)
    t.set_geometry_path(path)
    t.set_spheres(sph)
    return t


def gpu(t, p, n_passes, per_launch=None):
    """(accumulation, statistics) of n_passes passes on a context that has its scene"""
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


def describe(st):
    return (st.geometry_path, st.n_spheres, st.bvh_nodes, st.bvh_slots, tuple(st.grid_cells), st.grid_entries, st.grid_kernel_build,
            st.grid_walk_flat)


def assert_plain(t, st, row):
    assert row_of(st) == row, (row, row_of(st), describe(st))
    assert t.last_trace_build() == abi.BUILD_PLAIN
    if st.geometry_path == abi.PT_GEOM_GRID:  # the library's report of its own staging is the staging rule's
        assert st.grid_fit_stale != 1
        cells = st.grid_cells[0] * st.grid_cells[1] * st.grid_cells[2]
        assert grid_staging(cells, st.grid_entries)[0] == st.grid_kernel_build, describe(st)
        assert st.grid_walk_flat == (1 if st.grid_kernel_build == 1 and st.grid_cells[1] == 1 else 0)
    assert sum(st.work) == 0  # a plain kernel tallies nothing


CASE_IDS = ["%s-%d" % (b[0], i) for i, b in enumerate(BUILDS)]


@pytest.fixture(scope="module")
def whole(ora):
    """per case: the scene, its uniforms and the oracle's whole frame, made once and left unchanged"""
    cache = {}

    def get(i):
        if i not in cache:
            row, make, path = BUILDS[i]
            sc = make()
            p = with_lens_and_step(sc.params)
            assert p.max_depth == 8 and sc.n_passes >= 2
            ref, seg = oracle(ora, sc.spheres, p, sc.n_passes)
            ref.setflags(write=False)
            cache[i] = (sc.spheres, p, sc.n_passes, ref, seg)
        return cache[i]
    return get


@pytest.mark.parametrize("i", range(len(BUILDS)), ids=CASE_IDS)
def test_every_plain_build_equals_the_oracle(ora, whole, i):
    """(a) and (b)"""
    row, _, path = BUILDS[i]
    sph, p, n_passes, ref, seg = whole(i)
    w, h = p.width, p.height
    t = context(sph, w, h, path)
    try:
        got, st = gpu(t, p, n_passes)
        assert_plain(t, st, row)
        assert st.render_launches == 1
        if row == "list_lds":  # list_block_threads (csrc/pt_launch_plan.hpp): 1024 threads once the copy is over 40 KiB
            assert ((((len(sph) + 7) & ~7) + 4) * 16 > 40 * 1024) == (len(sph) > 2560)
        assert_bit_equal(got, ref, "%s, %d passes in one launch" % (row, n_passes))
        assert st.segments == seg, (row, st.segments, seg)
        got, st = gpu(t, p, n_passes, per_launch=1)
        assert_plain(t, st, row)
        assert st.render_launches == n_passes
        assert_bit_equal(got, ref, "%s, one pass per launch" % row)
        assert st.segments == seg, (row, st.segments, seg)
    finally:
        t.close()
    seg_bands = 0
    for r in range(3):
        q = p.copy()
        q.band_rows, q.band_index, q.band_count = 4, r, 3
        tb = context(sph, w, h, path)
        try:
            part, st = gpu(tb, q, n_passes)
            assert_plain(tb, st, row)
            ys = abi.owned_rows(h, 4, r, 3)
            assert part.shape[0] == len(ys) > 0
            assert_bit_equal(part, ref[ys], "%s, band %d of 3 against the rows of the whole frame" % (row, r))
            if r == 1:
                banded, seg_b = oracle(ora, sph, q, n_passes)
                assert_bit_equal(part, banded, "%s, band 1 of 3 against the oracle's banded render" % row)
                assert st.segments == seg_b
            seg_bands += st.segments
        finally:
            tb.close()
    assert seg_bands == seg
    REACHED.setdefault(row, []).append("%d spheres, %dx%d, whole and in bands" % (len(sph), w, h))


@pytest.mark.parametrize("i", range(len(BUILDS)), ids=CASE_IDS)
def test_every_measuring_twin_equals_its_plain_build(whole, i):
    """(c) PT_OPT_COUNT_WORK: the twin where the row has one — another binary, the same control flow — and the plain kernel
    where it has none; either way the oracle's bits, which the plain launch gave in (a)."""
    row, _, path = BUILDS[i]
    sph, p, n_passes, ref, seg = whole(i)
    t = context(sph, p.width, p.height, path)
    try:
        plain, st = gpu(t, p, n_passes)
        assert_plain(t, st, row)
        seg_plain = st.segments
        t.set_count_work(True)
        got, st = gpu(t, p, n_passes)
        assert row_of(st) == row, (row, row_of(st), describe(st))
        assert_bit_equal(got, plain, "%s under PT_OPT_COUNT_WORK against the plain launch" % row)
        assert_bit_equal(got, ref, "%s under PT_OPT_COUNT_WORK against the oracle" % row)
        assert st.segments == seg_plain == seg, (row, st.segments, seg_plain, seg)
        twin, work = twin_of(row), list(st.work)
        if twin is not None:
            assert t.last_trace_build() == abi.BUILD_TWIN
            assert work[6] > 0 and work[1] <= 64 * work[0], work
            assert work[6] * 64 >= seg  # wave steps x 64 lanes bound the shaded segments
            REACHED.setdefault(twin, []).append("%s, %d spheres" % (row, len(sph)))
        else:
            assert sum(work) == 0, (row, work)  # no twin: the plain kernel ran, and it tallies nothing
    finally:
        t.close()


N_TICKS, T0, DT = 5, 100.0, 16.5  # a group of four frames and a single one; start and interval exact in fp32


@pytest.mark.parametrize("i", range(len(BUILDS)), ids=CASE_IDS)
def test_frames_through_every_plain_build(ora, i):
    """(d) Five ticks of the reference's loop (one pass, then the shader's render() blend into the ping-pong textures) through
    this row's kernel: replayed by pt_render_frames — frames 0..3 are the four passes of ONE launch, frame 4 a launch of its own,
    u_time, render_count and the texture choice counted on the device — against five pt_render_frame calls whose uniforms the
    host steps.  The tick-by-tick canvas is the oracle's: tick 0 (one pass, blended with nothing) for every row, and tick 4 —
    which needs the oracle's five-tick simulation — for the rows below 10 000 spheres; the larger ones are held to the oracle
    at tick 0 and to the tick-by-tick context after it, so that a case stays at a few seconds."""
    row, make, path = BUILDS[i]
    sc = make()
    sph, (w, h) = sc.spheres, (sc.params.width, sc.params.height)
    p = with_lens_and_step(sc.params)
    p.should_average, p.last_frame_weight, p.render_count = 1, 1.0, 1
    p.time, p.time_step, p.first_pass = T0, DT, 0
    rc_max, e0 = 100000, 0

    def tick(k):
        q = p.copy()
        q.time, q.render_count = T0 + DT * k, min(p.render_count + k, rc_max)
        return q

    a, b = context(sph, w, h, path), context(sph, w, h, path)
    try:
        for t in (a, b):
            t.clear_textures()
        canvases = []
        for k in range(N_TICKS):
            a.set_params(tick(k))
            a.render_frame(e0 + k)
            assert_plain(a, a.stats(), row)
            if k in (0, N_TICKS - 1):
                canvases.append(a.read_canvas())
        b.set_params(p)
        b.render_frames(e0, rc_max, N_TICKS)
        assert_plain(b, b.stats(), row)
        assert np.array_equal(b.read_canvas(), canvases[1]), "%s: canvas of the replayed frames" % row
        for k in range(2):
            assert np.array_equal(a.read_texture(k), b.read_texture(k)), "%s: texture %d" % (row, k)
        assert a.stats().segments == b.stats().segments
        # the oracle's loop
        tex = [np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 4), np.uint8)]
        segs = 0
        for k in range(N_TICKS if len(sph) < 10000 else 1):
            q = tick(k)
            acc, seg = oracle(ora, sph, q, 1)
            expect = ora.blend_rgba8(acc, q.samples_per_pixel, q, tex[(e0 + k + 1) % 2])
            tex[(e0 + k) % 2] = expect
            segs += seg
            if k in (0, N_TICKS - 1):
                assert np.array_equal(canvases[0 if k == 0 else 1], expect), "%s: canvas of tick %d against the oracle" % (row, k)
        if len(sph) < 10000:
            assert a.stats().segments == segs
            for k in range(2):
                assert np.array_equal(a.read_texture(k), tex[k]), "%s: texture %d against the oracle" % (row, k)
        assert len(np.unique(canvases[1][..., :3])) > 16  # (a picture, not a constant)
    finally:
        a.close()
        b.close()
    REACHED.setdefault(row, []).append("frames")


def test_every_plain_kernel_and_twin_was_reached():
    """(runs after the tests above) each of the fourteen plain kernels and the five measuring twins was launched and compared"""
    print("plain kernels and measuring twins reached\n" + "\n".join("  %-18s %s" % (k, "; ".join(REACHED.get(k, [])) or "-") for k in ROWS + TWINS))
    assert len(ROWS) == 14 and len(TWINS) == 5
    missing = [k for k in ROWS + TWINS if k not in REACHED]
    assert not missing, "never reached: %s" % ", ".join(missing)
    assert sorted(REACHED) == sorted(ROWS + TWINS)
