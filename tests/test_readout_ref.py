"""The numpy restatement of the read-out and frame statements (tests/readout_ref.py) against the CPU oracle, on the
very arrays tests/test_gpu_readout_edges.py feeds the kernels — and the proof, without a GPU, that those arrays reach
the guards: every class of operand the GPU tests are about is present in at least 32 texels.

The oracle's read-out takes ONE sample count for a frame, so it can speak for a buffer of varying counts only pixel
set by pixel set: one call per distinct positive whole count, stitched (readout_ref.oracle_stitched).  For counts
that are none (0, -0, negative, subnormal, infinite, NaN, or beyond uint32) the restatement alone states what pixel_scale
(pt_kernels.hip) does.  Floats are compared as bit patterns except where both sides are NaN, bytes outright; there is no
tolerance anywhere."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import readout_ref as R

MIN_TEXELS = 32


def _same_bytes(got, ref, what):
    assert np.array_equal(got, ref), "%s: %d bytes differ, first at %s" % (what, int((got != ref).sum()), np.argwhere(got != ref)[:3].tolist())


def _all_buffers():
    out = [("edge%d" % i, a) for i, a in enumerate(R.edge_accums())]
    out += [("61x7", R.small_accum(7, 61, 7)), ("1x1", R.small_accum(1, 1, 8)), ("3x5", R.small_accum(5, 3, 9)), ("blend", R.blend_accum())]
    return out


def test_fma32_is_fmaf():
    """The one fused operation of the restatement against the C library's fmaf: random operands, the special list,
    exact cancellation (a * b - fl(a * b): the low half of a product, which only a single rounding returns)."""
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(11)
    pool = np.concatenate([R.SPECIAL, rng.standard_normal(64).astype(np.float32), (rng.standard_normal(64) * 1e-20).astype(np.float32),
                           np.array([1, 255, 2.0 ** 24, 1 / 255, 3, 1e30, 1e-30, 2.0 ** 20], np.float32)])
    n = 6000
    a, b, c = rng.choice(pool, n), rng.choice(pool, n), rng.choice(pool, n)
    a[:2000], b[:2000] = rng.random(2000).astype(np.float32), rng.random(2000).astype(np.float32)
    c[:2000] = -(a[:2000] * b[:2000])
    a[2000:3000] = rng.integers(0, 256, 1000).astype(np.float32) / np.float32(255)   # the blend's own shape: px * w + pr * rc
    ref = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    assert R.same_floats(R.fma32(a, b, c), ref), R.first_difference(R.fma32(a, b, c), ref)
    assert (ref[:2000] != 0).sum() > 1000   # the cancellation cases did leave a low half


@pytest.mark.parametrize("gamma", [0, 1])
def test_resolve_restatement_equals_the_oracle(ora, gamma):
    spoken = 0
    for name, acc in _all_buffers():
        ref, known = R.oracle_stitched(lambda a, n: ora.resolve(a, n, bool(gamma)), acc)
        got = R.resolve(acc, gamma)
        assert R.same_floats(got[known], ref[known]), "%s: %s" % (name, R.first_difference(got[known], ref[known]))
        ref8, known8 = R.oracle_stitched(lambda a, n: ora.resolve_rgba8(a, n, bool(gamma)), acc)
        _same_bytes(R.resolve_rgba8(acc, gamma)[known8], ref8[known8], name)
        spoken += int(known.sum())
    assert spoken > 6 * R.WIDTH * R.HEIGHT // 2   # the oracle spoke for more than half of the pixels
    # a uniform whole count: the oracle speaks for the whole buffer
    acc = R.edge_accums()[0].copy()
    acc[..., 3] = 4.0
    assert R.same_floats(R.resolve(acc, gamma), ora.resolve(acc, 4, bool(gamma)))
    _same_bytes(R.resolve_rgba8(acc, gamma), ora.resolve_rgba8(acc, 4, bool(gamma)), "uniform count")


def test_counts_that_are_none_read_as_the_contract_says():
    """pixel_scale (pt_kernels.hip), DESIGN.md §3: a count of 0, -0, below 0, NaN or +inf scales by 0 — a finite sum reads as 0 (as -0 when it
    is negative), a non-finite one as NaN, byte 0 either way; a subnormal count scales by +inf."""
    rgb = np.array([[0.5, -0.5, 0.0], [np.inf, np.nan, -np.inf], [1e-40, 3e38, -0.0]], np.float32)
    for w in (0.0, -0.0, -1.0, np.inf, np.nan):
        acc = np.concatenate([rgb, np.full((3, 1), w, np.float32)], axis=1)
        out = R.resolve(acc, 0)
        assert R.same_floats(out[:, :3], np.array([[0.0, -0.0, 0.0], [np.nan, np.nan, np.nan], [0.0, 0.0, -0.0]], np.float32)), (w, out)
        assert not R.resolve_rgba8(acc, 0)[:, :3].any() and not R.resolve_rgba8(acc, 1)[:, :3].any()
    acc = np.concatenate([rgb, np.full((3, 1), R.SUBNORMAL_COUNT, np.float32)], axis=1)
    assert R.same_floats(R.resolve(acc, 0)[:, :3], np.array([[np.inf, -np.inf, np.nan], [np.inf, np.nan, -np.inf], [np.inf, np.inf, np.nan]], np.float32))
    assert np.array_equal(R.resolve_rgba8(acc, 0)[:, :3], np.array([[255, 0, 0], [255, 0, 0], [255, 255, 0]], np.uint8))


def test_a_contracted_multiply_add_in_unorm8_changes_no_byte():
    """unorm8 rounds twice (the product, then the sum).  The two roundings can part from the single one of a contracted
    multiply-add only where the sum crosses into a coarser binade, and next to an integer that happens at 0.5 / 255
    alone, where no float lands in the window: an exhaustive run over all 1 065 353 215 floats of (0, 1) found no operand
    whose byte differs.  So that perturbation is not observable, by these tests or any; here the neighbourhoods of all
    rounding edges (64 floats each side) say so again, cheaply."""
    k = np.arange(255, dtype=np.float64)
    v = R._neighbours(((k + 0.5) / 255.0).astype(np.float32), 64)
    v = np.concatenate([v, R.edge_colours()])
    with np.errstate(all="ignore"):
        v = np.concatenate([v, np.sqrt(v)])
    assert np.array_equal(R.unorm8(v), R.unorm8(v, fused=True))


def test_the_edge_buffers_reach_every_guard_of_the_resolve_kernels():
    """The condition that keeps the GPU tests from passing on inputs that never reach a guard (the resolve kernels' buffers): each class of
    colour, after the per-pixel scale, and each count in at least 32 texels — in the buffers as a whole and, for the
    counts, in every single buffer."""
    accs = R.edge_accums()
    for gamma in (0, 1):
        tot = {}
        for acc in accs:
            for name, n in R.colour_classes(acc, gamma).items():
                tot[name] = tot.get(name, 0) + n
        for name, n in tot.items():
            assert n >= MIN_TEXELS, (gamma, name, n)
    for acc in accs:
        for name, n in R.count_classes(acc).items():
            assert n >= MIN_TEXELS, (name, n)
        # ... and the counts do vary within the buffer, next to each other
        a = acc[..., 3].reshape(-1)
        assert (R.bits(a[1:]) != R.bits(a[:-1])).mean() > 0.9
    # a rounding edge is an operand whose byte changes within two floats of it: all 255 edges, on both sides
    x = np.concatenate([R.scaled_colour(acc, 0).reshape(-1) for acc in accs])
    by = R.unorm8(x)
    inside = (x > 0) & (x < 1)
    flips = inside & (R.unorm8(np.nextafter(x, np.float32(2))) != R.unorm8(np.nextafter(x, np.float32(-1))))
    assert len(np.unique(by[flips])) >= 255 and flips.sum() >= 255 * 3


def test_blend_restatement_equals_the_oracle_and_its_input_reaches_the_guards(ora):
    """The per-pixel blend test's input: the existing edge test's rules on a buffer of varying counts."""
    from ray_tracer_webgl_amd import scenes

    acc = R.blend_accum()
    prev = R.seed_texture(R.HEIGHT, R.WIDTH, 45, every_byte=True)
    p = scenes.default_scene(R.WIDTH, R.HEIGHT, spp=4, max_depth=8).params
    for rc, avg, wt in R.BLEND_RULES:
        q = p.copy()
        q.render_count, q.should_average, q.last_frame_weight = rc, avg, wt
        ref, known = R.oracle_stitched(lambda a, n: ora.blend_rgba8(a, n, q, prev), acc)
        got = R.blend_rgba8(acc, prev, rc, avg, wt)
        _same_bytes(got[known], ref[known], (rc, avg, wt))
        assert known.sum() > acc.shape[0] * acc.shape[1] // 2
    # the uniform count of the existing test, whole buffer
    uni = acc.copy()
    uni[..., 3] = 4.0
    for rc, avg, wt in R.BLEND_RULES:
        q = p.copy()
        q.render_count, q.should_average, q.last_frame_weight = rc, avg, wt
        _same_bytes(R.blend_rgba8(uni, prev, rc, avg, wt), ora.blend_rgba8(uni, 4, q, prev), (rc, avg, wt))
    # the guards of blend_texel: colours that sqrt_core does not cover, previous texels with and without data, every byte value
    cls = R.colour_classes(acc, 0)
    for name in ("nan", "negative", "subnormal", "below_2^-96", "pos_inf", "zero", "above_one"):
        assert cls[name] >= MIN_TEXELS, (name, cls[name])
    for name, n in R.count_classes(acc).items():
        assert n >= MIN_TEXELS, (name, n)
    for a in (0, 1, 128, 255):
        assert (prev[..., 3] == a).sum() >= MIN_TEXELS
    for ch in range(3):
        assert len(np.unique(prev[..., ch])) == 256


@pytest.fixture(scope="module")
def frame_passes(ora):
    """The oracle's pass of every frame the series draw: whole image, and the band of the banded series."""
    n = max(s["n"] for s in R.FRAME_SERIES)
    out = {}
    for band in (None, (8, 1, 3)):
        spheres, p = R.frame_scene(band)
        out[band] = R.oracle_passes(ora, spheres, p, n)
    return out


@pytest.mark.parametrize("s", R.FRAME_SERIES, ids=[s["name"] for s in R.FRAME_SERIES])
def test_frame_chain_restatement_equals_the_oracles_simulation(ora, frame_passes, s):
    """The frame series: the restatement's chain against the tick loop of __graft_entry__.smoke() built on ora_blend_rgba8."""
    spheres, p = R.frame_scene(s["band"])
    passes = frame_passes[s["band"]][:s["n"]]
    h, w = passes[0].shape[:2]
    seeds = [R.seed_texture(h, w, 50), R.seed_texture(h, w, 51)]
    tex = [seeds[0].copy(), seeds[1].copy()]
    for k in range(s["n"]):
        q = R.tick_params(p, s, k)
        eo = (s["e0"] + k) & 0xFFFFFFFF
        canvas = ora.blend_rgba8(passes[k], 1, q, tex[(eo + 1) & 1])
        if s["avg"]:
            tex[eo & 1] = canvas
    got = R.frame_chain(passes, seeds[0], seeds[1], s["rc0"], s["max_rc"], s["e0"], s["avg"], s["lfw"])
    _same_bytes(got[0], canvas, "canvas")
    _same_bytes(got[1], tex[0], "texture 0")
    _same_bytes(got[2], tex[1], "texture 1")
    # the series does what its name says
    rcs = [min(s["rc0"] + k, s["max_rc"]) for k in range(s["n"])]
    if s["name"] == "averaging_starts_mid_group":
        assert [rc > 1 for rc in rcs[:4]] == [False, False, True, True]
    if s["name"] == "total_leaves_the_fast_range":
        tot = [np.float32(rc) + np.float32(s["lfw"]) for rc in rcs]
        assert tot[0] < 2.0 ** 20 <= tot[3] and tot[2] >= 2.0 ** 20   # leaves [2^-20, 2^20) inside the first group of four
    if s["name"] == "clamp_reached_mid_group":
        assert rcs[:4] == [5, 6, 7, 7]
    if s["name"] in ("max_one", "max_zero", "clamp_below_the_start"):
        assert len(set(rcs)) == 1
    if s["name"] == "sum_beyond_int32":
        assert s["rc0"] + s["n"] - 1 > R.INT_MAX and rcs[-1] == R.INT_MAX
    if s["name"] == "parity_across_the_wrap":
        assert s["e0"] + 3 == 1 << 32


def test_the_frame_passes_and_seeds_reach_the_blends_guards(frame_passes):
    acc = frame_passes[None][0]
    assert (acc[..., 3] == 1.0).all()
    x = R.scaled_colour(acc, 1)
    assert ((x > 0) & (x < 1)).sum() >= MIN_TEXELS and (x >= 1).sum() >= MIN_TEXELS
    seed = R.seed_texture(R.HEIGHT, R.WIDTH, 50)
    for a in (0, 1, 128, 255):
        assert (seed[..., 3] == a).sum() >= MIN_TEXELS


@pytest.mark.parametrize("spp", [1, 2])
def test_extreme_radiance_scene_reaches_every_class_in_the_oracles_pass(ora, spp):
    """The extreme-radiance scene: the classes of radiance, counted in the oracle's own one-pass output (a -0 emission cannot be counted: a pixel's
    sum starts at +0, and +0 + -0 is +0).  And the restatement's read-out of three passes equals the oracle's."""
    spheres, p = R.extreme_scene(spp)
    assert len(spheres) <= 15 and p.lens_radius == 0.0
    one, _ = ora.render(spheres, p, 1)
    cls = R.radiance_classes(one[..., :3])
    for name, n in cls.items():
        assert n >= MIN_TEXELS, (spp, name, n, cls)
    lit = np.isnan(one[..., :3]) | (one[..., :3] != 0)
    assert lit.any(axis=-1).mean() > 0.5   # the emitters and their reflections fill most of the view
    acc, _ = ora.render(spheres, p, 3)
    assert (acc[..., 3] == 3.0 * spp).all()
    for gamma in (0, 1):
        assert R.same_floats(R.resolve(acc, gamma), ora.resolve(acc, 3 * spp, bool(gamma)))
        _same_bytes(R.resolve_rgba8(acc, gamma), ora.resolve_rgba8(acc, 3 * spp, bool(gamma)), "rgba8")
    # its averaging frame series
    s = R.EXTREME_SERIES
    passes = R.oracle_passes(ora, spheres, p, s["n"])
    h, w = passes[0].shape[:2]
    seeds = [R.seed_texture(h, w, 60), R.seed_texture(h, w, 61)]
    tex = [seeds[0].copy(), seeds[1].copy()]
    for k in range(s["n"]):
        q = R.tick_params(p, s, k)
        eo = (s["e0"] + k) & 0xFFFFFFFF
        canvas = ora.blend_rgba8(passes[k], spp, q, tex[(eo + 1) & 1])
        tex[eo & 1] = canvas
    got = R.frame_chain(passes, seeds[0], seeds[1], s["rc0"], s["max_rc"], s["e0"], s["avg"], s["lfw"])
    _same_bytes(got[0], canvas, "canvas")
    _same_bytes(got[1], tex[0], "texture 0")
    _same_bytes(got[2], tex[1], "texture 1")
