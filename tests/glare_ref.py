"""A plain restatement of the glare pyramid (include/ptrace.h pt_glare), written from the header's statement list and independent of
the library: it never calls it.  Shared by tests/test_glare_ref.py on the CPU and tests/test_gpu_glare.py on the device.

TEST INFRASTRUCTURE ONLY.  Whole-image numpy arrays, one IEEE operation per statement, nothing fused; `dtype` is np.float32 — the
contract — or np.float64, which runs the SAME statements (the fp32 constants included) at the other precision for the rounding
bound of test_glare_ref.py.  Floats are compared as bit patterns (NaN with NaN).
"""
import numpy as np

F = np.float32
MAX_LEVELS = 8
DEFAULT = dict(strength=0.15, threshold=0.0, levels=6, weights=(0.35, 0.25, 0.18, 0.12, 0.06, 0.04, 0.0, 0.0))
SIZES = ((1, 1), (1, 7), (3, 5), (17, 16), (33, 130), (64, 36))   # (width, rows)
LEVELS = (1, 2, 5, 8)
HALVES = (0.5, 0.25, 0.125, 0.0625, 0.0625)   # five weights, exact in fp32, that add up to 1


def options(strength=DEFAULT["strength"], threshold=DEFAULT["threshold"], levels=DEFAULT["levels"], weights=DEFAULT["weights"]):
    w = tuple(weights) + (0.0,) * (MAX_LEVELS - len(tuple(weights)))
    return dict(strength=strength, threshold=threshold, levels=int(levels), weights=w)


def half_up(n):
    return (n + 1) // 2


def level_sizes(w, h, levels):
    """[(w_1, h_1), ..., (w_levels, h_levels)]"""
    out = []
    for _ in range(levels):
        w, h = half_up(w), half_up(h)
        out.append((w, h))
    return out


def pyramid_texels(w, h, levels=MAX_LEVELS):
    return 0 if w == 0 or h == 0 else sum(a * b for a, b in level_sizes(w, h, levels))


def source(texels, from_accum, dtype=F):
    """x of every texel, (h, w, 3): an accumulation texel is scaled by its own count (scale = w > 0 ? 1 / w : 0)."""
    t = np.asarray(texels, np.float32).astype(dtype)
    x = t[..., :3].copy()
    if from_accum:
        with np.errstate(all="ignore"):
            cnt = t[..., 3]
            scale = np.where(cnt > 0, dtype(1.0) / np.where(cnt > 0, cnt, dtype(1.0)), dtype(0.0)).astype(dtype)
            x = (x * scale[..., None]).astype(dtype)
    return x


def luminance(x, dtype=F):
    with np.errstate(all="ignore"):
        Y = dtype(F(0.2126)) * x[..., 0]
        t = dtype(F(0.7152)) * x[..., 1]
        Y = Y + t
        t = dtype(F(0.0722)) * x[..., 2]
        Y = Y + t
    return Y.astype(dtype)


def bright(texels, from_accum, threshold, dtype=F):
    """(x, b), each (h, w, 3)"""
    x = source(texels, from_accum, dtype)
    Y = luminance(x, dtype)
    thr = dtype(F(threshold))
    with np.errstate(all="ignore"):
        bad = ~((Y - Y) == 0)
        if thr == 0:
            b = x.copy()
        else:
            t = (Y - thr).astype(dtype)
            spills = t > 0
            m = (t / np.where(spills, Y, dtype(1.0))).astype(dtype)
            b = np.where(spills[..., None], (x * m[..., None]).astype(dtype), dtype(0.0)).astype(dtype)
        b = np.where(bad[..., None], dtype(0.0), b).astype(dtype)
    return x, b


def _down_axis(img, axis, dtype):
    n = img.shape[axis]
    X = np.arange(half_up(n))
    t = [np.take(img, np.clip(2 * X + k, 0, n - 1), axis=axis) for k in (-1, 0, 1, 2)]
    with np.errstate(all="ignore"):
        o = t[0] + t[3]
        i = t[1] + t[2]
        i = dtype(3.0) * i
        s = o + i
        v = s * dtype(0.125)
    return v.astype(dtype)


def down(img, dtype=F):
    """D_k (h_k, w_k, 3) from D_{k-1}: first along x, then along y"""
    return _down_axis(_down_axis(img, 1, dtype), 0, dtype)


def _up_axis(A, n, axis, dtype):
    N = A.shape[axis]
    X = np.arange(n)
    p = X >> 1
    q = np.where(X & 1, p + 1, p - 1)
    Ap = np.take(A, np.clip(p, 0, N - 1), axis=axis)
    Aq = np.take(A, np.clip(q, 0, N - 1), axis=axis)
    with np.errstate(all="ignore"):
        t = dtype(3.0) * Ap
        t = t + Aq
        v = t * dtype(0.25)
    return v.astype(dtype)


def up(A, w, h, dtype=F):
    """up(A) at a (w, h) level: first along x, then along y"""
    return _up_axis(_up_axis(A, w, 1, dtype), h, 0, dtype)


def pyramid(b, levels, dtype=F):
    """[D_0 = b, D_1, ..., D_levels]"""
    D = [b]
    for _ in range(levels):
        D.append(down(D[-1], dtype))
    return D


def spread(b, opt, dtype=F, D=None):
    """G (h, w, 3): the pyramid of b (`D`: pyramid(b, at least opt's levels), when the caller has it already), gathered and
    brought back to the frame's size"""
    h, w = b.shape[:2]
    L = opt["levels"]
    if D is None:
        D = pyramid(b, L, dtype)
    with np.errstate(all="ignore"):
        U = (dtype(F(opt["weights"][L - 1])) * D[L]).astype(dtype)
        for k in range(L - 1, 0, -1):
            a = (dtype(F(opt["weights"][k - 1])) * D[k]).astype(dtype)
            U = (a + up(U, D[k].shape[1], D[k].shape[0], dtype)).astype(dtype)
    return up(U, w, h, dtype)


def composite(x, b, G, strength, dtype=F):
    """(h, w, 4): out.c = x.c + (G.c - b.c) * strength, out.w = 1"""
    out = np.ones(x.shape[:2] + (4,), dtype)
    with np.errstate(all="ignore"):
        d = G - b
        d = d * dtype(F(strength))
        out[..., :3] = x + d
    return out


def glare(texels, from_accum, opt=None, dtype=F):
    """(h, w, 4) of pt_glare over a (h, w, 4) image"""
    opt = opt or options()
    texels = np.asarray(texels, np.float32)
    h, w = texels.shape[:2]
    if h == 0 or w == 0:
        return np.ones((h, w, 4), dtype)
    x, b = bright(texels, from_accum, opt["threshold"], dtype)
    return composite(x, b, spread(b, opt, dtype), opt["strength"], dtype)


# ------------------------------------------------------------------------------------------------ frames
def random_frame(w, h, seed, from_accum):
    """(h, w, 4) fp32: colours over six decades, a few exact zeros; as accumulation texels with per-pixel counts, some zero"""
    rng = np.random.default_rng(seed)
    rgb = np.exp(rng.uniform(-7.0, 7.0, (h, w, 3))).astype(np.float32)
    rgb[rng.random((h, w)) < 0.1] = 0.0
    img = np.empty((h, w, 4), np.float32)
    if from_accum:
        cnt = rng.integers(0, 9, (h, w)).astype(np.float32)   # (0 among them: scale 0)
        cnt.flat[0] = cnt.flat[-1] = 3.0   # (pt_load_accum takes the first and the last texel's count for the checkpoint's)
        img[..., :3] = rgb * cnt[..., None]
        img[..., 3] = cnt
    else:
        img[..., :3] = rgb
        img[..., 3] = rng.uniform(-2.0, 2.0, (h, w)).astype(np.float32)   # (not read)
    return img


def odd_frame(w, h, seed):
    """a random linear frame with NaN, +inf, -inf, negative and -0 texels strewn in (at most a fifth of the pixels)"""
    img = random_frame(w, h, seed, False)
    rng = np.random.default_rng(seed + 1)
    odd = np.array([np.nan, np.inf, -np.inf, -1.5, -0.0], np.float32)
    n = max(1, (w * h) // 5)
    ys, xs, cs = rng.integers(0, h, n), rng.integers(0, w, n), rng.integers(0, 3, n)
    img[ys, xs, cs] = odd[rng.integers(0, len(odd), n)]
    return img


def _grey_with_luminance(y):
    """a grey g whose luminance (the five statements) is exactly y, or None: not every float is some grey's luminance"""
    g = F(y)
    for _ in range(16):
        got = luminance(np.array([[g, g, g]], np.float32))[0]
        if got == y:
            return g
        g = np.nextafter(g, F(np.inf) if got < y else F(0))
    return None


def threshold_frame(w, h, nominal):
    """(image, threshold): a grey frame whose luminances fall exactly on the threshold, one ulp below it, one ulp above it, at four
    times and at half of it, pixel k holding case k % 5; the threshold is the first float at or above `nominal` for which greys
    with the first three luminances exist."""
    thr = F(nominal)
    for _ in range(256):
        want = [thr, np.nextafter(thr, F(0)), np.nextafter(thr, F(np.inf)), thr * F(4), thr * F(0.5)]
        greys = [_grey_with_luminance(y) for y in want[:3]] + [want[3], want[4]]
        if all(g is not None for g in greys[:3]):
            break
        thr = np.nextafter(thr, F(np.inf))
    else:
        raise AssertionError("no threshold near %g" % nominal)
    img = np.ones((h, w, 4), np.float32)
    k = np.arange(w * h).reshape(h, w) % 5
    img[..., :3] = np.array(greys, np.float32)[k][..., None]
    return img, float(thr)
