"""A plain restatement of the read-out and frame statements, independent of the oracle's C, and the edge inputs the
read-out tests share (tests/test_readout_ref.py on the CPU, tests/test_gpu_readout_edges.py on the device).

TEST INFRASTRUCTURE ONLY.  np.float32 arrays throughout, one IEEE operation per statement, nothing fused — with the
one exception the blend itself states: `fmaf(px, last_frame_weight, pr * render_count)` (oracle/pt_oracle.c
ora_blend_rgba8, pt_kernels.hip blend_texel), restated here as fma32().  The accumulation buffer is taken as it is:
the divisor is each pixel's own `.a`.

What the statements do with a count that is no count (include/ptrace.h says only that the divisor is each pixel's `.a`;
pt_kernels.hip pixel_scale and DESIGN.md §3 say the rest):
    scale = w > 0 ? 1 / w : 0          0, -0, negative and NaN counts give scale 0; +inf gives 0 as 1 / inf; a subnormal
                                       count gives +inf (1 / w overflows)
    x = v * scale                      so a finite sum reads as 0 (-0 for a negative sum) under scale 0, and a non-finite
                                       sum reads as NaN (inf * 0); unorm8 maps both to the byte 0
"""
import numpy as np

from ray_tracer_webgl_amd import abi, scenes

F = np.float32
WIDTH, HEIGHT = 64, 36   # the image of every test that does not say otherwise


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def bits(a):
    return _f32(a).view(np.uint32)


def same_floats(got, ref):
    """Bit patterns equal, except where both sides are NaN."""
    got, ref = _f32(got), _f32(ref)
    return got.shape == ref.shape and bool(np.all((bits(got) == bits(ref)) | (np.isnan(got) & np.isnan(ref))))


def first_difference(got, ref):
    got, ref = _f32(got), _f32(ref)
    bad = np.argwhere(~((bits(got) == bits(ref)) | (np.isnan(got) & np.isnan(ref))))
    if len(bad) == 0:
        return "equal"
    i = tuple(bad[0])
    return "%d of %d values differ, first at %s: %r (0x%08x) vs %r (0x%08x)" % (
        len(bad), got.size, i, got[i], bits(got)[i], ref[i], bits(ref)[i])


# ------------------------------------------------------------------------------------------------ the statements
def fma32(a, b, c):
    """fmaf on float32 arrays: the product of two floats is exact in float64, the sum is rounded to odd there (TwoSum
    gives the sum's error exactly) and then once to float32 — 53 bits >= 2 * 24 + 2, so that is the single rounding."""
    a, b, c = np.broadcast_arrays(_f32(a), _f32(b), _f32(c))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0.0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where(err > 0.0, np.inf, -np.inf)
        s = np.where(inexact, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def pixel_scale(w):
    w = _f32(w)
    with np.errstate(all="ignore"):
        q = F(1.0) / w
    return np.where(w > F(0.0), q, F(0.0)).astype(np.float32)


def scaled_colour(accum, gamma):
    """x = v.rgb * scale, then the optional sqrt: (..., 3) float32."""
    accum = _f32(accum)
    scale = pixel_scale(accum[..., 3])
    with np.errstate(all="ignore"):
        x = accum[..., :3] * scale[..., None]
        if gamma:
            x = np.sqrt(x)
    return x.astype(np.float32)


def resolve(accum, gamma):
    x = scaled_colour(accum, gamma)
    out = np.empty(x.shape[:-1] + (4,), np.float32)
    out[..., :3] = x
    out[..., 3] = F(1.0)
    return out


def unorm8(v, fused=False):
    """!(v > 0) -> 0;  v >= 1 -> 255;  else truncate float32(float32(v * 255) + 0.5).
    fused: with the ONE rounding of a contracted multiply-add instead — not what the kernels do; test_readout_ref.py uses it to
    show that no operand tells the two apart."""
    v = _f32(v)
    with np.errstate(all="ignore"):
        if fused:
            t = fma32(v, F(255.0), F(0.5))
        else:
            t = v * F(255.0)
            t = t + F(0.5)
        inside = (v > F(0.0)) & ~(v >= F(1.0))
        q = np.where(inside, t, F(0.0)).astype(np.uint32)   # truncation; operands outside (0, 1) never reach it
    return np.where(~(v > F(0.0)), 0, np.where(v >= F(1.0), 255, q)).astype(np.uint8)


def resolve_rgba8(accum, gamma):
    x = scaled_colour(accum, gamma)
    out = np.empty(x.shape[:-1] + (4,), np.uint8)
    out[..., :3] = unorm8(x)
    out[..., 3] = 255
    return out


def blend_rgba8(accum, prev, render_count, should_average, last_frame_weight):
    """static/shader.frag:387-404 as ora_blend_rgba8 states it, on the frame's colour sqrt(v.rgb * scale)."""
    prev = np.ascontiguousarray(prev, dtype=np.uint8)
    px = scaled_colour(accum, True)
    out = np.empty(prev.shape, np.uint8)
    out[..., 3] = 255
    straight = unorm8(px)
    if not should_average:
        out[..., :3] = straight
        return out
    rc = F(int(render_count))
    lfw = F(last_frame_weight)
    with np.errstate(all="ignore"):
        pa = prev[..., 3].astype(np.float32) / F(255.0)
        no_data = (pa == F(0.0)) | (int(render_count) <= 1)
        total = rc + lfw
        pr = prev[..., :3].astype(np.float32) / F(255.0)
        t = pr * rc
        num = fma32(px, lfw, t)
        merged = (num / total).astype(np.float32)
    out[..., :3] = np.where(no_data[..., None], straight, unorm8(merged))
    return out


def frame_chain(passes, tex0, tex1, render_count0, max_render_count, even_odd0, should_average, last_frame_weight):
    """n ticks of src/lib.rs:92-102 on the two RGBA8 textures; `passes` are the frames' accumulation buffers.
    Returns (canvas, texture 0, texture 1)."""
    tex = [np.array(tex0, np.uint8), np.array(tex1, np.uint8)]
    canvas = None
    for k, acc in enumerate(passes):
        rc = min(int(render_count0) + k, int(max_render_count))
        eo = (int(even_odd0) + k) & 0xFFFFFFFF
        canvas = blend_rgba8(acc, tex[(eo + 1) & 1], rc, should_average, last_frame_weight)
        if should_average:
            tex[eo & 1] = canvas
    return canvas, tex[0], tex[1]


# ------------------------------------------------------------------------------------------------ the edge inputs
# the special list of test_temporal_blend_rgba8_at_the_edges_of_its_fast_forms (tests/test_gpu_parity.py)
SPECIAL = np.array([0.0, 1e-45, 1e-40, 2.0 ** -100, 2.0 ** -96 * 4 * 0.999, 2.0 ** -96 * 4, 2.0 ** -94, 1e-20, 1e-10, 0.5, 4.0, 7.99, 1e10,
                    3e38, np.inf, np.nan, -0.0, -1e-30, -1.0], np.float32)
# ... and its rule list: (render_count, should_average, last_frame_weight)
BLEND_RULES = [(0, 1, 1.0), (1, 1, 1.0), (2, 1, 1.0), (37, 1, 0.5), (5, 0, 1.0), (3, 1, 1e-30), (3, 1, 1e-38), (2, 1, 1e30), (2, 1, 0.0),
               (1 << 20, 1, 1.0), ((1 << 20) - 1, 1, 0.5), (2_000_000_000, 1, 1.0), (2, 1, 3e38), (7, 1, float("inf")), (7, 1, float("nan")),
               (9, 1, -9.0), (9, 1, -1.0)]

SUBNORMAL_COUNT = F(1e-40)
# counts whose reciprocal is a power of two (v * count * scale == v exactly), other counts, and counts that are none
COUNTS_EXACT = np.array([1.0, 2.0, 4.0, 2.0 ** 24, 1.0, 2.0], np.float32)
COUNTS_INEXACT = np.array([3.0, 7.0, 255.0, 2.0 ** 24 + 2.0, 3e38, 3.0], np.float32)
COUNTS_NONE = np.array([0.0, -0.0, -1.0, SUBNORMAL_COUNT, np.inf, np.nan], np.float32)
COUNTS = np.concatenate([COUNTS_EXACT, COUNTS_INEXACT, COUNTS_NONE])
# what the oracle can speak for: positive integers that fit its uint32 total_spp
ORACLE_COUNTS = (1, 2, 3, 4, 7, 255, 1 << 24, (1 << 24) + 2)


def _neighbours(v, n=2):
    """v and its n float32 neighbours on each side."""
    v = _f32(v)
    out = [v]
    lo = hi = v
    for _ in range(n):
        lo = np.nextafter(lo, F(-np.inf))
        hi = np.nextafter(hi, F(np.inf))
        out += [lo, hi]
    return np.stack(out, axis=-1).reshape(-1).astype(np.float32)


def edge_colours():
    """The colours the resolve kernels are loaded with: the special list; for every byte k in 0..254 the float nearest (k + 0.5) / 255 with two
    neighbours on each side (the operands next to unorm8's rounding edge in linear mode), their squares with two
    neighbours on each side (the same edge behind the sqrt of gamma mode); and 1 with its neighbours, squared too."""
    k = np.arange(255, dtype=np.float64)
    lin = _neighbours(((k + 0.5) / 255.0).astype(np.float32))
    ones = np.array([np.nextafter(F(1), F(0)), F(1), np.nextafter(F(1), F(2))], np.float32)
    with np.errstate(all="ignore"):
        sq = _neighbours(lin * lin)
        ones_sq = _neighbours(ones * ones)
    # (the specials and the ones 48 times over: each meets every count of the cycle, and each class fills 32 texels and more)
    return np.concatenate([np.tile(SPECIAL, 48), np.tile(ones, 48), lin, np.tile(ones_sq, 8), sq]).astype(np.float32)


def _counts_for(n_pix, shift):
    c = COUNTS[(np.arange(n_pix) + 6 * shift) % len(COUNTS)].copy()
    # pt_load_accum takes a checkpoint whose first and last pixel carry the same whole count below 2^24
    c[0] = c[-1] = F(1.0)
    return c


def accum_with(colours, counts, h, w):
    """(h, w, 4): channel slot s holds colours[s] times its pixel's count where that product means anything (a positive
    finite normal count), the colour itself elsewhere."""
    colours = _f32(colours).reshape(h, w, 3)
    counts = _f32(counts).reshape(h, w)
    with np.errstate(all="ignore"):
        usable = (counts >= F(2.0 ** -126)) & np.isfinite(counts)
        rgb = np.where(usable[..., None], colours * counts[..., None], colours)
    acc = np.empty((h, w, 4), np.float32)
    acc[..., :3] = rgb
    acc[..., 3] = counts
    return acc


def edge_accums(h=HEIGHT, w=WIDTH):
    """The buffers the resolve kernels are loaded with: every edge colour under three counts — one whose reciprocal is exact, one whose is
    not, one that is no count — varying from pixel to pixel.  The colour list is laid over as many pages of h*w*3
    channel slots as it needs (the tail of the last page repeats it), each page under the three shifts of the count
    cycle."""
    col = edge_colours()
    slots = h * w * 3
    pages = -(-len(col) // slots)
    col = np.resize(col, pages * slots)
    out = []
    for page in range(pages):
        for shift in range(3):
            out.append(accum_with(col[page * slots:(page + 1) * slots], _counts_for(h * w, shift), h, w))
    return out


def small_accum(h, w, seed):
    """Other sizes for the resolve kernels (one block and a bit, 1x1, 3x5): a random draw from the edge colours and the count cycle."""
    rng = np.random.default_rng(seed)
    col = rng.choice(edge_colours(), h * w * 3)
    counts = rng.choice(COUNTS, h * w)
    counts[0] = counts[-1] = F(3.0)
    return accum_with(col, counts, h, w)


def blend_accum(h=HEIGHT, w=WIDTH, seed=44):
    """The per-pixel blend test's buffer: half special colours, half ordinary ones, under the count cycle."""
    rng = np.random.default_rng(seed)
    ordinary = (rng.random(h * w * 3) * rng.choice(np.array([0.01, 0.3, 1.0, 3.0]), h * w * 3)).astype(np.float32)
    col = np.where(rng.random(h * w * 3) < 0.5, rng.choice(SPECIAL, h * w * 3), ordinary)
    return accum_with(col, _counts_for(h * w, 1), h, w)


def seed_texture(h, w, seed, every_byte=False):
    """Random bytes with alpha in {0, 1, 128, 255}; every_byte: every byte value in every channel, as the existing edge test."""
    rng = np.random.default_rng(seed)
    tex = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if every_byte and w >= 48:
        ramp = np.arange(h * 16).reshape(h, 16)
        tex[:, :16, 0] = ramp % 256
        tex[:, 16:32, 1] = (ramp + 97) % 256
        tex[:, 32:48, 2] = (ramp + 191) % 256
    tex[..., 3] = rng.choice(np.array([0, 1, 128, 255], np.uint8), (h, w))
    return tex


def oracle_stitched(fn, accum, *args):
    """What the oracle says about a buffer of varying counts: one call per distinct positive whole count, stitched.
    Returns (result, mask of the pixels it could speak for)."""
    accum = _f32(accum)
    out, known = None, np.zeros(accum.shape[:-1], bool)
    for n in ORACLE_COUNTS:
        sel = accum[..., 3] == F(n)
        if not sel.any():
            continue
        r = fn(accum, n, *args)
        if out is None:
            out = np.zeros_like(r)
        out[sel] = r[sel]
        known |= sel
    return out, known


def colour_classes(accum, gamma):
    """How many channel values of the buffer land in each class of operand, after the scale (and the sqrt)."""
    accum = _f32(accum)
    x_lin = scaled_colour(accum, False)
    x = scaled_colour(accum, gamma)
    one = F(1.0)
    with np.errstate(all="ignore"):
        z = x.astype(np.float64) * 255.0 + 0.5
        inside = (x > 0) & (x < 1)
        near = inside & (np.abs(z - np.rint(z)) < 1e-4)
        c = {
            "nan": np.isnan(x_lin), "neg_zero": (x_lin == 0) & np.signbit(x_lin), "negative": x_lin < 0, "pos_inf": np.isposinf(x_lin),
            "subnormal": (x_lin > 0) & (x_lin < F(2.0 ** -126)), "below_2^-96": (x_lin >= F(2.0 ** -126)) & (x_lin < F(2.0 ** -96)),
            "zero": (x_lin == 0) & ~np.signbit(x_lin), "one": x == one, "just_below_one": x == np.nextafter(one, F(0)),
            "just_above_one": x == np.nextafter(one, F(2)), "above_one": x > one,
            "edge_rounds_down": near & (z < np.rint(z)), "edge_rounds_up": near & (z >= np.rint(z)),
        }
    return {k: int(v.sum()) for k, v in c.items()}


def count_classes(accum):
    """How many pixels of the buffer carry each count of the cycle."""
    a = _f32(accum)[..., 3]
    out = {}
    for v in np.concatenate([COUNTS_EXACT[:4], COUNTS_INEXACT[:5], COUNTS_NONE]):
        if np.isnan(v):
            out["nan"] = int(np.isnan(a).sum())
        else:
            out[repr(float(v))] = int(((a == v) & (np.signbit(a) == np.signbit(v))).sum())
    return out


# ------------------------------------------------------------------------------------------------ frame series
T0, DT = 200.0, 16.5          # exact in fp32, and so is every T0 + k * DT used here
INT_MAX = (1 << 31) - 1


def _series(name, rc0=3, max_rc=100000, e0=5, n=9, lfw=1.0, avg=1, band=None):
    return dict(name=name, rc0=rc0, max_rc=max_rc, e0=e0, n=n, lfw=lfw, avg=avg, band=band)


FRAME_SERIES = [
    _series("averaging_starts_mid_group", rc0=0, n=9),
    _series("total_leaves_the_fast_range", rc0=(1 << 20) - 3, max_rc=INT_MAX, n=9),
    _series("clamp_reached_mid_group", rc0=5, max_rc=7, n=9),
    _series("clamp_below_the_start", rc0=9, max_rc=3, n=9),
    _series("max_one", rc0=3, max_rc=1, n=5),
    _series("max_zero", rc0=3, max_rc=0, n=5),
    _series("sum_beyond_int32", rc0=INT_MAX - 2, max_rc=INT_MAX, n=5),
    _series("parity_across_the_wrap", e0=(1 << 32) - 3, n=9),
    _series("weight_1e-30", lfw=1e-30, n=5),
    _series("weight_1e30", lfw=1e30, n=5),
    _series("weight_zero", lfw=0.0, n=5),
    _series("weight_minus_one", lfw=-1.0, n=5),
    _series("weight_inf", lfw=float("inf"), n=5),
    _series("weight_nan", lfw=float("nan"), n=5),
    # the total passes through 0 inside the first group (-2, -1, 0, 1 ...), where the plain division gives
    # +-inf or NaN and div_core's reciprocal does not: the one total found to tell a forced `total_ok` from the guard in bytes
    _series("total_is_zero_mid_group", rc0=3, lfw=-5.0, n=9),
    _series("n1", n=1), _series("n4", n=4), _series("n5", n=5), _series("n16", n=16), _series("n19", n=19), _series("n23", n=23),
    _series("no_averaging", n=9, avg=0),
    _series("banded", rc0=1, n=9, band=(8, 1, 3)),
]


def frame_scene(band=None, w=WIDTH, h=HEIGHT):
    """The default scene at 1 spp; (spheres, params) with the series' clock."""
    sc = scenes.default_scene(w, h, spp=1, max_depth=6)
    p = sc.params.copy()
    p.time, p.time_step, p.first_pass = T0, DT, 0
    if band is not None:
        p.band_rows, p.band_index, p.band_count = band
    return sc.spheres, p


def tick_params(p, s, k):
    """Frame k's uniforms as a host that steps them itself uploads them."""
    q = p.copy()
    q.time = T0 + DT * k
    q.render_count = min(s["rc0"] + k, s["max_rc"])
    q.should_average, q.last_frame_weight = s["avg"], s["lfw"]
    return q


def series_params(p, s):
    q = p.copy()
    q.render_count, q.should_average, q.last_frame_weight = s["rc0"], s["avg"], s["lfw"]
    return q


def oracle_passes(ora, spheres, p, n):
    """The oracle's pass of each of n frames (it depends on the clock alone, not on the blend's uniforms)."""
    out = []
    for k in range(n):
        q = p.copy()
        q.time = T0 + DT * k
        out.append(ora.render(spheres, q, 1)[0])
    return out


# ------------------------------------------------------------------------------------------------ extreme radiance
EMISSIONS = np.array([0.0, 1e-45, 1e-40, 2.0 ** -100, 2.0 ** -96, 2.0 ** -94, 0.5, 4.0, 1e10, 3e38, np.inf, np.nan, -0.0, -1.0], np.float32)


def extreme_scene(spp, w=WIDTH, h=HEIGHT):
    """Black background, lens off, 15 spheres: a diffuse floor, one metal sphere and thirteen PT_EMISSIVE spheres that fill most of
    the view, their 39 albedo channels running three times (nearly) through EMISSIONS."""
    S = scenes._sphere
    items = [S((0.0, -101.2, -1.0), 100.0, abi.PT_DIFFUSE, (0.8, 0.6, 0.4)),
             S((0.0, -0.8, -1.0), 0.36, abi.PT_METAL, (0.9, 0.8, 0.7), fuzz=0.1)]
    centres = [(x, 0.7, -1.0) for x in (-1.6, -0.8, 0.0, 0.8, 1.6)] + [(x, -0.05, -1.0) for x in (-1.2, -0.4, 0.4, 1.2)] + \
              [(x, -0.8, -1.0) for x in (-1.6, -0.8, 0.8, 1.6)]
    for c in centres:
        items.append(S(c, 0.36, abi.PT_EMISSIVE, (0.0, 0.0, 0.0)))
    spheres = scenes._pack(items)
    for i in range(len(centres)):
        # (written as float32: _pack goes through float64, which would not keep a subnormal's bits otherwise)
        spheres[2 + i]["albedo"] = EMISSIONS[(3 * i + np.arange(3)) % len(EMISSIONS)]
    p = scenes._base_params(spp, 6, background=abi.PT_BG_BLACK)
    scenes._look_at(scenes._lib(), p, w, h, (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), 60.0, 0.0, 2.0)
    p.time, p.time_step, p.first_pass = T0, DT, 0
    return spheres, p


def radiance_classes(rgb):
    rgb = _f32(rgb)
    c = {"nan": np.isnan(rgb), "pos_inf": np.isposinf(rgb), "negative": rgb < 0, "zero": rgb == 0,
         "subnormal": (rgb > 0) & (rgb < F(2.0 ** -126)), "below_2^-96": (rgb >= F(2.0 ** -126)) & (rgb < F(2.0 ** -96)),
         "at_2^-96_and_2^-94": (rgb >= F(2.0 ** -96)) & (rgb <= F(2.0 ** -93)), "ordinary": (rgb >= F(0.01)) & (rgb <= F(8.0)),
         "huge": (rgb >= F(1e9)) & np.isfinite(rgb)}
    return {k: int(v.sum()) for k, v in c.items()}


# the averaging frame series of the extreme-radiance scene
EXTREME_SERIES = _series("extreme_radiance", rc0=0, n=9)
