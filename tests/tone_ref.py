"""A plain restatement of exposure metering and the tone curves (include/ptrace.h pt_meter, pt_resolve_toned), written from the
header's statement lists and independent of the library: it never calls it.  Shared by tests/test_tone_ref.py on the CPU and
tests/test_gpu_tone.py, tests/test_gpu_meter.py on the device.

TEST INFRASTRUCTURE ONLY.  np.float32 arrays throughout, one IEEE operation per statement, nothing fused; the histogram and the
ranks are Python integers.  Floats are compared as bit patterns (NaN with NaN), bytes and counts outright.
"""
import numpy as np

import readout_ref as rr

F = np.float32
CLAMP, REINHARD, FILMIC = 0, 1, 2
BIN0 = 888
DEFAULTS = dict(key=0.18, key_permille=500, high_permille=990, e_min=2.0 ** -8, e_max=2.0 ** 8, white_min=1.0, rate=1.0)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ------------------------------------------------------------------------------------------------ the source image
def source(texels, from_accum):
    """x of every texel, (..., 3): an accumulation texel is scaled by its own count (pt_resolve, gamma 0), an external one is its rgb."""
    texels = _f32(texels)
    if from_accum:
        return rr.scaled_colour(texels, 0)
    return texels[..., :3].copy()


# ------------------------------------------------------------------------------------------------ kernel 1
def luminance(x):
    x = _f32(x)
    with np.errstate(all="ignore"):
        Y = F(0.2126) * x[..., 0]
        t = F(0.7152) * x[..., 1]
        Y = Y + t
        t = F(0.0722) * x[..., 2]
        Y = Y + t
    return Y.astype(np.float32)


def tally_of(Y):
    """Per luminance: its bin 0..255, or 256 for `below`."""
    Y = _f32(Y)
    with np.errstate(all="ignore"):
        lit = Y >= F(2.0 ** -16)
    k = (Y.view(np.uint32).astype(np.int64) >> 20) - BIN0
    k = np.where(k > 255, 255, k)
    return np.where(lit, k, 256).astype(np.int64)


def edge(k):
    return np.array([(int(k) + BIN0) << 20], np.uint32).view(np.float32)[0]


def band_row(band_rows, band_index, band_count, ly):
    if band_count <= 1 or band_rows == 0:
        return ly
    return (ly // band_rows * band_count + band_index) * band_rows + ly % band_rows


def window_mask(rows, width, window=(0, 0, 0, 0), band=(0, 0, 1)):
    """(rows, width) bool: the local pixels a metering looks at."""
    x0, y0, w, h = window
    if w == 0 or h == 0:
        return np.ones((rows, width), bool)
    px = np.arange(width)
    y = np.array([band_row(band[0], band[1], band[2], ly) for ly in range(rows)], np.int64)
    in_x = (px >= x0) & (px < x0 + w)
    in_y = (y >= y0) & (y < y0 + h)
    return in_y[:, None] & in_x[None, :]


def meter(texels, from_accum, window=(0, 0, 0, 0), band=(0, 0, 1)):
    """(hist: 256 Python ints, below) of a (rows, width, 4) image."""
    texels = _f32(texels)
    rows, width = texels.shape[:2]
    slot = tally_of(luminance(source(texels, from_accum)))
    slot = slot[window_mask(rows, width, window, band)]
    counts = np.bincount(slot.reshape(-1), minlength=257)
    return [int(c) for c in counts[:256]], int(counts[256])


# ------------------------------------------------------------------------------------------------ kernel 2
def solve(hist, below, opt=None, prev=None):
    """The record as a dict; `opt` a dict over DEFAULTS, `prev` a record dict or None (never valid)."""
    o = dict(DEFAULTS)
    o.update(opt or {})
    key, e_min, e_max, white_min, rate = (F(o[k]) for k in ("key", "e_min", "e_max", "white_min", "rate"))
    rec = dict(exposure=F(prev["exposure"]) if prev else F(1.0), white=F(prev["white"]) if prev else white_min,
               y_key=F(prev["y_key"]) if prev else F(0.0), y_high=F(prev["y_high"]) if prev else F(0.0),
               lit=0, below=int(below), meterings=((prev["meterings"] if prev else 0) + 1) & 0xFFFFFFFF)
    hist = [int(h) for h in hist]
    N = sum(hist)
    if N == 0:
        return rec

    def bin_of(p):
        rank = min(N - 1, (N * int(p)) // 1000)
        cum = 0
        for k in range(256):
            cum += hist[k]
            if cum > rank:
                return k
        raise AssertionError("no bin")

    y_key = edge(bin_of(o["key_permille"]))
    y_high = edge(bin_of(o["high_permille"]))
    with np.errstate(all="ignore"):
        e_t = F(key / y_key)
        if e_t < e_min:
            e_t = e_min
        if e_t > e_max:
            e_t = e_max
        if prev and rate < F(1.0):
            e_prev = F(prev["exposure"])
            if not (rate > F(0.0)):
                e = e_prev
            else:
                d = F(e_t - e_prev)
                d = F(d * rate)
                e = F(e_prev + d)
        else:
            e = e_t
        white = F(y_high * e)
        if not (white >= white_min):
            white = white_min
    rec.update(exposure=F(e), white=F(white), y_key=y_key, y_high=y_high, lit=N)
    return rec


def options_valid(opt=None):
    o = dict(DEFAULTS)
    o.update(opt or {})
    for k in ("key", "e_min", "e_max", "white_min"):
        v = F(o[k])
        if not (v > 0 and np.isfinite(v)):
            return False
    if F(o["e_min"]) > F(o["e_max"]):
        return False
    if o["key_permille"] > 1000 or o["high_permille"] > 1000 or o["key_permille"] > o["high_permille"]:
        return False
    return not np.isnan(F(o["rate"]))


# ------------------------------------------------------------------------------------------------ the curves
def curve(which, x, white):
    """y of exposed channel values x (any shape)."""
    x = _f32(x)
    with np.errstate(all="ignore"):
        if which == REINHARD:
            w2 = F(white) * F(white)
            a = x / w2
            a = a + F(1.0)
            n = x * a
            d = x + F(1.0)
            return (n / d).astype(np.float32)
        if which == FILMIC:
            a = F(2.51) * x
            a = a + F(0.03)
            n = x * a
            b = F(2.43) * x
            b = b + F(0.59)
            d = x * b
            d = d + F(0.14)
            return (n / d).astype(np.float32)
    assert which == CLAMP
    return x.copy()


def toned_colour(x, which, gamma, exposure, white):
    x = _f32(x)
    with np.errstate(all="ignore"):
        xe = x * F(exposure)
        y = curve(which, xe, white)
        if gamma:
            y = np.sqrt(y)
    return y.astype(np.float32)


def toned(texels, from_accum, which, gamma, exposure, white):
    """(..., 4) float32: {y.rgb, 1}."""
    y = toned_colour(source(texels, from_accum), which, gamma, exposure, white)
    out = np.empty(y.shape[:-1] + (4,), np.float32)
    out[..., :3] = y
    out[..., 3] = F(1.0)
    return out


def toned_rgba8(texels, from_accum, which, gamma, exposure, white):
    y = toned_colour(source(texels, from_accum), which, gamma, exposure, white)
    out = np.empty(y.shape[:-1] + (4,), np.uint8)
    out[..., :3] = rr.unorm8(y)
    out[..., 3] = 255
    return out


# ------------------------------------------------------------------------------------------------ shared inputs
EXPOSURES = np.array([2.0 ** -8, 0.37, 1.0, 15.0, 2.0 ** 8], np.float32)


def edge_luminances():
    """The 257 bin edges with both float32 neighbours each, and the read-outs' special list."""
    e = np.array([edge(k) for k in range(257)], np.float32)
    lo = np.nextafter(e, F(-np.inf))
    hi = np.nextafter(e, F(np.inf))
    return np.concatenate([np.stack([lo, e, hi], axis=-1).reshape(-1), rr.SPECIAL]).astype(np.float32)


def meter_image(h=rr.HEIGHT, w=rr.WIDTH):
    """(h, w, 4) external texels whose luminances run through edge_luminances(), as r-only, g-only, b-only and mixed pixels in
    turn: a single-channel pixel carries Y / weight in its channel (the product then lands on or next to the wanted luminance),
    a mixed one a third of it in each.  What each pixel's luminance IS is the restatement's business, not this function's."""
    Y = np.resize(edge_luminances(), h * w)
    img = np.zeros((h * w, 4), np.float32)
    kind = np.arange(h * w) % 4
    with np.errstate(all="ignore"):
        for c, wgt in enumerate((0.2126, 0.7152, 0.0722)):
            sel = kind == c
            img[sel, c] = (Y[sel].astype(np.float64) / wgt).astype(np.float32)
        sel = kind == 3
        img[sel, 0] = img[sel, 1] = img[sel, 2] = Y[sel]
    img[:, 3] = np.resize(np.array([1.0, 0.0, np.nan, -3.0], np.float32), h * w)   # (not read)
    return img.reshape(h, w, 4)


def record_of(rec):
    """A ctypes PtExposure (or anything with its attributes) as the dict solve() returns."""
    return dict(exposure=F(rec.exposure), white=F(rec.white), y_key=F(rec.y_key), y_high=F(rec.y_high), lit=int(rec.lit),
                below=int(rec.below), meterings=int(rec.meterings))


def same_record(got, ref):
    return all(rr.same_floats(got[k], ref[k]) for k in ("exposure", "white", "y_key", "y_high")) and \
        all(got[k] == ref[k] for k in ("lit", "below", "meterings"))
