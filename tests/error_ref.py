"""A plain restatement of the per-pixel error estimate (include/ptrace.h PT_OPT_ERROR_ESTIMATE): the fold,
the read-out, the tile tree and the host sums, independent of the kernels, and the inputs its tests share
(tests/test_error_ref.py on the CPU, tests/test_gpu_error_estimate.py on the device).

TEST INFRASTRUCTURE ONLY.  np.float32 arrays throughout, one IEEE operation per statement, nothing fused; numpy's float32
`/` and sqrt are correctly rounded.  The state of a pixel is A = {mean.r, mean.g, mean.b, n}, B = {M2.r, M2.g, M2.b, k}; a state
array has the shape (rows, width, 2, 4).

    fold, per pass p in order, s = slab[p][i]:
        accum.c = accum.c + s.c                      (c = r, g, b, w)
        n = n + 1;  k = k + s.w
        d = s.c - mean.c;  mean.c = mean.c + d / n;  e = s.c - mean.c;  M2.c = M2.c + d * e
    read-out:
        if (!(n >= 2) || !(k > 0)) se = 0, m = 0
        else q = n / k;  v.c = M2.c / (n * (n - 1));  se.c = sqrt(v.c) * q;  m.c = mean.c * q
    tile (8x8, lane l owns (8 tx + l % 8, 8 ty + l / 8)), counted = inside, n >= 2, k > 0, finite se and m:
        e = (se.r*se.r + se.g*se.g) + se.b*se.b;  m2 = (m.r*m.r + m.g*m.g) + m.b*m.b;  +0 from every other lane
        for off in 32, 16, 8, 4, 2, 1:  v[l] = v[l] + v[l + off]  (l < off)
        record = {sum e, sum m2, counted lanes, min n over counted lanes (0 if none)}
    host: E, M, counted summed in tile index order in double; rel_error = M > 0 ? sqrt(E / M) : 0;
        rms_error = counted ? sqrt(E / (3 counted)) : 0
"""
import math

import numpy as np

from ray_tracer_webgl_amd import abi, scenes

F = np.float32
WIDTH, HEIGHT = 64, 36


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
    if got.shape != ref.shape:
        return "shapes %s vs %s" % (got.shape, ref.shape)
    bad = np.argwhere(~((bits(got) == bits(ref)) | (np.isnan(got) & np.isnan(ref))))
    if len(bad) == 0:
        return "equal"
    i = tuple(bad[0])
    return "%d of %d values differ, first at %s: %r (0x%08x) vs %r (0x%08x)" % (
        len(bad), got.size, i, got[i], bits(got)[i], ref[i], bits(ref)[i])


# ------------------------------------------------------------------------------------------------ the fold
def empty_state(rows, width):
    return np.zeros((rows, width, 2, 4), np.float32)


def fold(state, accum, passes):
    """Fold the pass sums `passes` (each (rows, width, 4): {sum r, sum g, sum b, spp}) in order; returns (state, accum)."""
    st = _f32(state).copy()
    acc = _f32(accum).copy()
    mean, n = st[..., 0, :3], st[..., 0, 3]
    m2, k = st[..., 1, :3], st[..., 1, 3]
    with np.errstate(all="ignore"):
        for s in passes:
            s = _f32(s)
            acc[...] = acc + s
            n[...] = n + F(1.0)
            k[...] = k + s[..., 3]
            x = s[..., :3]
            d = x - mean
            q = d / n[..., None]
            mean[...] = mean + q
            e = x - mean
            t = d * e
            m2[...] = m2 + t
    return st, acc


# ------------------------------------------------------------------------------------------------ the read-out
def pixel_error(state):
    """(se, m, known): se and m (rows, width, 3) float32, 0 where the pixel is not known (n < 2 or k <= 0, NaN included)."""
    st = _f32(state)
    mean, n = st[..., 0, :3], st[..., 0, 3]
    m2, k = st[..., 1, :3], st[..., 1, 3]
    with np.errstate(all="ignore"):
        known = (n >= F(2.0)) & (k > F(0.0))
        q = n / k
        n1 = n - F(1.0)
        nn = n * n1
        v = m2 / nn[..., None]
        s = np.sqrt(v)
        se = s * q[..., None]
        m = mean * q[..., None]
    zero = np.zeros_like(se)
    return np.where(known[..., None], se, zero).astype(np.float32), np.where(known[..., None], m, zero).astype(np.float32), known


def resolve_error(state):
    """pt_resolve_error: {se.r, se.g, se.b, n} per pixel."""
    se, _, _ = pixel_error(state)
    out = np.empty(se.shape[:-1] + (4,), np.float32)
    out[..., :3] = se
    out[..., 3] = _f32(state)[..., 0, 3]
    return out


def _tree_add(v):
    """The wave's fixed tree on (tiles, 64) float32: v[l] = v[l] + v[l + off] for l < off, off = 32 ... 1."""
    v = v.copy()
    with np.errstate(all="ignore"):
        for off in (32, 16, 8, 4, 2, 1):
            v[:, :off] = v[:, :off] + v[:, off:2 * off]
    return v[:, 0]


def _lanes(a, fill):
    """(rows, width) -> (tiles_y * tiles_x, 64): lane l of tile (tx, ty) is pixel (8 tx + l % 8, 8 ty + l / 8); `fill` outside."""
    rows, width = a.shape
    ty, tx = (rows + 7) // 8, (width + 7) // 8
    pad = np.full((ty * 8, tx * 8), fill, a.dtype)
    pad[:rows, :width] = a
    return pad.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty * tx, 64)


def tiles(state):
    """pt_error_tiles: ((tiles_y, tiles_x, 4) float32 records, tallies) — tallies = dict of per-tile integer arrays `short`
    (pixels with !(n >= 2)), `nonfinite` (n >= 2 and not counted) and float32 `nmax` (max n over counted, 0 if none)."""
    st = _f32(state)
    rows, width = st.shape[:2]
    ty, tx = (rows + 7) // 8, (width + 7) // 8
    se, m, known = pixel_error(st)
    n = st[..., 0, 3]
    with np.errstate(all="ignore"):
        counted = known & np.isfinite(se).all(axis=-1) & np.isfinite(m).all(axis=-1)
        e = se[..., 0] * se[..., 0]
        t = se[..., 1] * se[..., 1]
        e = e + t
        t = se[..., 2] * se[..., 2]
        e = e + t
        q = m[..., 0] * m[..., 0]
        t = m[..., 1] * m[..., 1]
        q = q + t
        t = m[..., 2] * m[..., 2]
        q = q + t
    zero = np.zeros_like(e)
    e = np.where(counted, e, zero).astype(np.float32)
    q = np.where(counted, q, zero).astype(np.float32)
    rec = np.zeros((ty * tx, 4), np.float32)
    rec[:, 0] = _tree_add(_lanes(e, F(0.0)))
    rec[:, 1] = _tree_add(_lanes(q, F(0.0)))
    cl = _lanes(counted, False)
    rec[:, 2] = cl.sum(axis=1).astype(np.float32)
    nl = _lanes(n, F(0.0))
    rec[:, 3] = np.where(cl.any(axis=1), np.where(cl, nl, np.inf).min(axis=1), 0.0).astype(np.float32)
    with np.errstate(all="ignore"):
        short = ~(n >= F(2.0))
    tallies = {"short": _lanes(short, False).sum(axis=1), "nonfinite": _lanes(~short & ~counted, False).sum(axis=1),
               "nmax": np.where(cl, nl, 0.0).max(axis=1).astype(np.float32)}
    return rec.reshape(ty, tx, 4), tallies


def stats(state):
    """pt_error_stats: the records summed in tile index order in double."""
    rec, tal = tiles(state)
    rows, width = _f32(state).shape[:2]
    rec = rec.reshape(-1, 4)
    E = M = 0.0
    counted = 0
    for r in rec:
        E += float(r[0])
        M += float(r[1])
        counted += int(r[2])
    with np.errstate(all="ignore"):
        rel = math.sqrt(E / M) if M > 0.0 else 0.0
        rms = math.sqrt(E / (3.0 * counted)) if counted else 0.0
    has = rec[:, 2] > 0
    return {"sum_e2": E, "sum_m2": M, "rel_error": rel, "rms_error": rms, "pixels": rows * width, "pixels_counted": counted,
            "pixels_short": int(tal["short"].sum()), "pixels_nonfinite": int(tal["nonfinite"].sum()),
            "passes_min": int(rec[has, 3].min()) if has.any() else 0, "passes_max": int(tal["nmax"][has].max()) if has.any() else 0}


def same_stats(st, ref):
    """A PtErrorStats against stats(): doubles as bit patterns (NaN against NaN excepted), counts outright."""
    for k in ("sum_e2", "sum_m2", "rel_error", "rms_error"):
        a, b = float(getattr(st, k)), float(ref[k])
        if not (np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64) or (math.isnan(a) and math.isnan(b))):
            return "%s: %r vs %r" % (k, a, b)
    for k in ("pixels", "pixels_counted", "pixels_short", "pixels_nonfinite", "passes_min", "passes_max"):
        if int(getattr(st, k)) != int(ref[k]):
            return "%s: %r vs %r" % (k, int(getattr(st, k)), int(ref[k]))
    return ""


def predicted_stop(passes, passes_per_launch, target, max_passes):
    """What pt_render_until does, on pass sums obtained elsewhere: (passes rendered, reached, state, accum)."""
    rows, width = passes[0].shape[:2]
    st, acc = empty_state(rows, width), np.zeros((rows, width, 4), np.float32)
    done = 0
    while True:
        k = min(passes_per_launch, max_passes - done)
        st, acc = fold(st, acc, passes[done:done + k])
        done += k
        s = stats(st)
        reached = s["rel_error"] <= float(F(target)) and s["pixels_short"] == 0
        if reached or done >= max_passes:
            return done, reached, st, acc


# ------------------------------------------------------------------------------------------------ inputs
T0, T1 = 200.0, 5000.25   # the clocks of two independent sets of passes


def estimate_scene(w=WIDTH, h=HEIGHT, spp=4, clock=T0, band=None, black=False):
    """The default scene, depth 6, independent passes (PT_TIME_STEP_DECORRELATED)."""
    sc = scenes.default_scene(w, h, spp=spp, max_depth=6)
    p = sc.params.copy()
    p.time, p.time_step, p.first_pass = clock, abi.PT_TIME_STEP_DECORRELATED, 0
    if black:
        p.background_mode = abi.PT_BG_BLACK
    if band is not None:
        p.band_rows, p.band_index, p.band_count = band
    return sc.spheres, p


def oracle_passes(ora, spheres, p, n, first=0):
    """The oracle's sums of passes first ... first + n - 1, each rendered alone."""
    out = []
    for k in range(first, first + n):
        q = p.copy()
        q.first_pass = p.first_pass + k
        out.append(ora.render(spheres, q, 1)[0])
    return out


def calibration_ratio(state_a, state_b):
    """sum (m_A - m_B)^2 / sum (se_A^2 + se_B^2) over all pixels and channels of two independent estimates, in double: 1 when
    the standard errors say how far the means lie apart."""
    se_a, m_a, _ = pixel_error(state_a)
    se_b, m_b, _ = pixel_error(state_b)
    num = ((m_a.astype(np.float64) - m_b.astype(np.float64)) ** 2).sum()
    den = (se_a.astype(np.float64) ** 2 + se_b.astype(np.float64) ** 2).sum()
    return float(num / den)


# hand-made states: every class of n, k and M2, each filling at least one full tile and one edge tile
HAND_N = np.array([0.0, 1.0, 2.0, 3.0, 2.0 ** 24], np.float32)
HAND_K = np.array([0.0, -0.0, 1e-40, np.inf, np.nan], np.float32)
HAND_M2 = np.array([0.0, 1e-42, 3e38, np.inf, np.nan, -1.0], np.float32)
HAND_W, HAND_H = 8 * 16 + 3, 8 + 5   # 17 x 2 tiles: the last column of tiles is 3 wide, the last row 5 high


def hand_state(w=HAND_W, h=HAND_H):
    """Columns of tiles carry one class each (16 full columns: 5 of n, 5 of k, 6 of M2), so every class fills the full tile of
    the first tile row and the edge tile (5 rows high) of the second; the last, 3 wide, column of tiles repeats the first class
    of M2 mixed with ordinary pixels.  Everything that is not the column's subject is ordinary: n = 8, k = 32, mean and M2 from
    a generator."""
    rng = np.random.default_rng(5)
    st = empty_state(h, w)
    st[..., 0, :3] = rng.uniform(0.5, 8.0, (h, w, 3)).astype(np.float32)
    st[..., 0, 3] = 8.0
    st[..., 1, :3] = rng.uniform(0.0, 4.0, (h, w, 3)).astype(np.float32)
    st[..., 1, 3] = 32.0
    classes = []
    col = 0
    for v in HAND_N:
        st[:, 8 * col:8 * col + 8, 0, 3] = v
        classes.append(("n", v, col))
        col += 1
    for v in HAND_K:
        st[:, 8 * col:8 * col + 8, 1, 3] = v
        classes.append(("k", v, col))
        col += 1
    for v in HAND_M2:
        st[:, 8 * col:8 * col + 8, 1, :3] = v
        classes.append(("M2", v, col))
        col += 1
    st[::2, 8 * col:, 1, 0] = 0.0
    return st, classes


def hand_classes(state):
    """How many pixels of a state fall into each class of the read-out's operands."""
    st = _f32(state)
    n, k, m2 = st[..., 0, 3], st[..., 1, 3], st[..., 1, :3]
    c = {"n_0": n == 0, "n_1": n == 1, "n_2": n == 2, "n_3": n == 3, "n_2^24": n == F(2.0 ** 24),
         "k_0": (k == 0) & ~np.signbit(k), "k_-0": (k == 0) & np.signbit(k), "k_subnormal": (k > 0) & (k < F(2.0 ** -126)),
         "k_inf": np.isposinf(k), "k_nan": np.isnan(k),
         "M2_0": (m2 == 0).all(axis=-1), "M2_tiny": ((m2 > 0) & (m2 < F(2.0 ** -126))).all(axis=-1),
         "M2_huge": ((m2 > F(1e38)) & np.isfinite(m2)).all(axis=-1), "M2_inf": np.isposinf(m2).all(axis=-1),
         "M2_nan": np.isnan(m2).all(axis=-1), "M2_negative": (m2 < 0).all(axis=-1)}
    return {name: int(v.sum()) for name, v in c.items()}
