"""The glare pyramid without a device: csrc/pt_glare.hpp's host loop through tests/glare_shim.cpp against the plain restatement
tests/glare_ref.py, bit for bit; pins of the restatement itself (constants, energy, the impulse response, the fp32 rounding bound);
the stand-alone program tests/glare_main.cpp under the address and undefined-behaviour sanitizers; the GlareSet of
csrc/pt_buffers.hpp against a stand-in allocator; the ABI of the new struct and symbol.  Floats are compared as bit patterns (NaN
with NaN: the payload is not pinned).  CPU only."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import glare_ref as G
import readout_ref as R
from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd._lib import ADDED_WITHIN_ABI_5, SIGNATURES

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "ptrace.h")
F = np.float32


def _abi_opt(o):
    return abi.PtGlareOptions(o["strength"], o["threshold"], o["levels"], o["weights"])


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(tempfile.mkdtemp(prefix="glare_"), "libglare_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror", os.path.join(HERE, "glare_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    fp, vp, u32, u64 = C.POINTER(C.c_float), C.c_void_p, C.c_uint32, C.c_uint64
    lib.glare_run.restype, lib.glare_run.argtypes = C.c_int, [fp, u32, u32, C.c_int, C.POINTER(abi.PtGlareOptions), fp]
    lib.glare_options_valid.restype, lib.glare_options_valid.argtypes = C.c_int, [C.POINTER(abi.PtGlareOptions)]
    lib.glare_level_size.restype, lib.glare_level_size.argtypes = u32, [u32, u32]
    lib.glare_pyramid_texels.restype, lib.glare_pyramid_texels.argtypes = u64, [u32, u32, u32]
    lib.alloc_fail_at.restype, lib.alloc_fail_at.argtypes = None, [C.c_long]
    lib.alloc_live.restype, lib.alloc_live.argtypes = C.c_long, []
    lib.set_new.restype, lib.set_new.argtypes = vp, []
    lib.set_delete.restype, lib.set_delete.argtypes = None, [vp]
    lib.set_toggle.restype, lib.set_toggle.argtypes = C.c_int, [vp, C.c_int, u32, u32]
    lib.set_fit.restype, lib.set_fit.argtypes = C.c_int, [vp, u32, u32, C.POINTER(u32)]
    lib.set_in_place.restype, lib.set_in_place.argtypes = C.c_int, [vp, u32, u32]
    lib.set_on.restype, lib.set_on.argtypes = C.c_int, [vp]
    lib.set_capacity.restype, lib.set_capacity.argtypes = u64, [vp]
    lib.set_held.restype, lib.set_held.argtypes = C.c_int, [vp]
    lib.set_texels.restype, lib.set_texels.argtypes = u64, [u32, u32]
    return lib


def _run(shim, img, from_accum, opt):
    img = np.ascontiguousarray(img, np.float32)
    h, w = img.shape[:2]
    out = np.empty_like(img)
    o = _abi_opt(opt)
    rc = shim.glare_run(img.ctypes.data_as(C.POINTER(C.c_float)), w, h, int(from_accum), C.byref(o), out.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0
    return out


def _weights(levels):
    """`levels` distinct weights that add up to 1 within rounding"""
    w = np.arange(levels, 0, -1, dtype=np.float64)
    return tuple(float(F(v)) for v in w / w.sum())


def _cases():
    """(width, rows, levels): every size with every level count — 8 on the 1x1 frame among them"""
    return [(w, h, l) for (w, h) in G.SIZES for l in G.LEVELS]


# ------------------------------------------------------------------------------------------------ the header against the restatement
@pytest.mark.parametrize("w,h,levels", _cases())
def test_header_against_the_restatement(shim, w, h, levels):
    """Random frames of both source kinds (accumulation texels with per-pixel counts, some zero), threshold 0 and a threshold
    inside the frame's range, strengths 1, 0.15 and 0."""
    for from_accum in (False, True):
        img = G.random_frame(w, h, 7 * w + h + levels, from_accum)
        for threshold, strength in ((0.0, 1.0), (0.75, 0.15), (0.0, 0.0), (20.0, 1.0)):
            opt = G.options(strength, threshold, levels, _weights(levels))
            got, ref = _run(shim, img, from_accum, opt), G.glare(img, from_accum, opt)
            assert R.same_floats(got, ref), "%dx%d levels %d accum %d threshold %g: %s" % (w, h, levels, from_accum, threshold, R.first_difference(got, ref))


@pytest.mark.parametrize("w,h", G.SIZES)
def test_luminances_on_below_and_above_the_threshold(shim, w, h):
    """Greys whose luminance is exactly the threshold, one ulp below, one ulp above, four times and half of it: on and below it
    nothing spills (b = 0: the pixel only loses nothing and gains the veil), above it the share m = (Y - threshold) / Y does."""
    for nominal in (0.5, 1.0, 3.0):
        img, thr = G.threshold_frame(w, h, nominal)
        Y = G.luminance(G.source(img, False))
        flat = Y.reshape(-1)[: min(5, w * h)]
        assert list(flat[:3]) == [F(thr), np.nextafter(F(thr), F(0)), np.nextafter(F(thr), F(np.inf))][: len(flat)], (thr, flat)
        assert len(flat) < 5 or (flat[3] > F(2 * thr) and flat[4] < F(thr))
        _, b = G.bright(img, False, thr)
        spills = (b != 0).any(axis=-1).reshape(-1)[: len(flat)]
        assert list(spills) == [False, False, True, True, False][: len(flat)]
        for levels in (1, 5):
            opt = G.options(1.0, thr, levels, _weights(levels))
            got, ref = _run(shim, img, False, opt), G.glare(img, False, opt)
            assert R.same_floats(got, ref), (thr, levels, R.first_difference(got, ref))


@pytest.mark.parametrize("w,h", G.SIZES)
def test_bad_texels_do_not_veil_the_frame(shim, w, h):
    """NaN, +inf, -inf, negative and -0 texels: bit for bit against the restatement (NaN with NaN), and a pixel with a NaN or an
    infinite channel leaves every output texel finite except its own."""
    for levels in (1, 5, 8):
        for threshold in (0.0, 0.5):
            img = G.odd_frame(w, h, 100 + levels)
            opt = G.options(1.0, threshold, levels, _weights(levels))
            got, ref = _run(shim, img, False, opt), G.glare(img, False, opt)
            assert R.same_floats(got, ref), (levels, threshold, R.first_difference(got, ref))
            bad = ~np.isfinite(img[..., :3]).all(axis=-1)
            assert np.isfinite(got[~bad]).all(), (levels, threshold)
            assert (got[..., 3] == 1.0).all()
    # one NaN pixel alone in a finite frame: its own texel is NaN, nothing else is
    img = G.random_frame(w, h, 5, False)
    img[h // 2, w // 2, 1] = np.nan
    got = _run(shim, img, False, G.options(1.0, 0.0, 5, G.HALVES))
    assert np.isnan(got[h // 2, w // 2, 1])
    got[h // 2, w // 2] = 0.0
    assert np.isfinite(got).all()


def test_in_place_and_accumulation_scaling(shim):
    """An accumulation is glared as its resolved frame is: scaling by the count first, then the same statements."""
    acc = G.random_frame(33, 130, 3, True)
    opt = G.options(0.4, 0.3, 5, G.HALVES)
    lin = np.ones_like(acc)
    lin[..., :3] = G.source(acc, True)
    assert R.same_floats(_run(shim, acc, True, opt), _run(shim, lin, False, opt))


# ------------------------------------------------------------------------------------------------ pins of the restatement
@pytest.mark.parametrize("w,h", G.SIZES)
def test_a_constant_frame_comes_back_bit_for_bit(shim, w, h):
    """down's taps (1 3 3 1)/8 and up's (3 1)/4 are exact on a constant c: 2c, 2c, 6c, 8c, c and 3c, 4c, c are all exact for 0.75, 1
    and 15; the weights 1/2 .. 1/16, 1/16 and their partial sums times c are exact as well: G = c = b, d = 0, out = x, whatever
    the strength."""
    for value in (0.75, 1.0, 15.0):
        img = np.full((h, w, 4), value, np.float32)
        for strength in (0.0, 0.15, 0.5, 1.0):
            opt = G.options(strength, 0.0, 5, G.HALVES)
            ref = G.glare(img, False, opt)
            want = img.copy()
            want[..., 3] = 1.0
            assert R.same_floats(ref, want), (value, strength)
            assert R.same_floats(_run(shim, img, False, opt), want), (value, strength)


def _impulse(x, y, w=96, h=64):
    img = np.zeros((h, w, 4), np.float32)
    img[y, x, :3] = 1.0
    return img


def test_an_impulse_keeps_its_energy():
    """A unit impulse at the middle and at the corner of a 96x64 frame, weights 1/2 .. 1/16, 1/16, strength 1: G sums (in float64)
    to 1 within 1e-6 — the clamped taps at the rim give back what they would have read outside — and out = x + (G - b) = G."""
    opt = G.options(1.0, 0.0, 5, G.HALVES)
    for (x, y) in ((48, 32), (0, 0), (95, 63)):
        out = G.glare(_impulse(x, y), False, opt)
        for c in range(3):
            assert abs(float(out[..., c].astype(np.float64).sum()) - 1.0) < 1e-6, (x, y, c)
        assert (out[..., :3] >= 0).all()


def test_the_impulse_response():
    """WHAT THE RESPONSE IS.  One level, along one axis: an impulse at an EVEN texel x0 leaves D_1 = {1/8 at x0/2 - 1, 3/8 at x0/2}
    and comes back as G = (1, 3, 6, 10, 9, 3)/32 at x0 - 3 .. x0 + 2; at an ODD texel it is the mirror image, (3, 9, 10, 6, 3, 1)/32
    at x0 - 2 .. x0 + 3; in two dimensions the outer product of the two axes.  So the response is NOT mirror-symmetric about the
    impulse texel — a level's texel X covers the frame's texels 2X and 2X + 1, and the impulse sits half a texel off its centre —,
    but its first moment is zero (the veil is centred on the light: -3 - 6 - 6 + 0 + 9 + 6 = 0), and the symmetry that does hold, for
    any number of levels whose sizes halve exactly (96x64: levels 1 .. 5), is that of the whole operator: glare(mirror(frame)) ==
    mirror(glare(frame)), bit for bit, in x, in y and in both — the taps are read in mirrored order and the statements add the
    outer pair and the inner pair, so the order does not reach the bits.  The response of the impulse at the middle texel (48, 32)
    is therefore the mirror image of the response at (47, 31), about the point between the two."""
    even = np.array([1, 3, 6, 10, 9, 3], np.float64) / 32.0
    one = G.options(1.0, 0.0, 1, (1.0,))
    out = G.glare(_impulse(48, 32), False, one)[..., 0].astype(np.float64)
    want = np.zeros((64, 96))
    want[32 - 3:32 + 3, 48 - 3:48 + 3] = np.outer(even, even)
    assert np.array_equal(out, want)   # (every value a multiple of 2^-10: exact)
    out = G.glare(_impulse(47, 31), False, one)[..., 0].astype(np.float64)
    want = np.zeros((64, 96))
    want[31 - 2:31 + 4, 47 - 2:47 + 4] = np.outer(even[::-1], even[::-1])
    assert np.array_equal(out, want)
    ys, xs = np.mgrid[0:64, 0:96]
    rng_img = G.random_frame(96, 64, 11, False)
    for levels in (1, 2, 3, 4, 5):
        opt = G.options(1.0, 0.0, levels, _weights(levels))
        mid = G.glare(_impulse(48, 32), False, opt)
        twin = G.glare(_impulse(47, 31), False, opt)
        assert R.same_floats(mid, twin[::-1, ::-1]), levels
        if levels <= 2:  # (the support stays clear of the rim: the first moment is the impulse's own place)
            g = mid[..., 0].astype(np.float64)
            assert abs((g * xs).sum() / g.sum() - 48.0) < 1e-6 and abs((g * ys).sum() / g.sum() - 32.0) < 1e-6, levels
        full = G.glare(rng_img, False, opt)
        assert R.same_floats(G.glare(rng_img[:, ::-1], False, opt), full[:, ::-1]), levels
        assert R.same_floats(G.glare(rng_img[::-1], False, opt), full[::-1]), levels


def test_fp32_against_float64():
    """THE BOUND.  A non-negative linear frame of largest value M, threshold 0, weights that add up to at most 1: every value of
    the pyramid is a convex combination of inputs, so it lies in [0, M], and a statement's rounding error is at most 2^-24 times
    its result — at most 2^-24 M once the result is scaled back by the exact power of two that follows it (s * 0.125, t * 0.25).
    Errors pass through the convex combinations without growing.  Rounding statements on the longest path to an output texel, with
    L levels: bright 0 (b = x); down 4 per axis (o, i, 3 i, s), 8 per level, 8 L to the top level; gather 1 at the top (weight * D)
    and, per level below it, 4 for up (3 A, t + A on each axis), 1 for weight * D and 1 for the sum: 6 (L - 1); composite 4 for
    up(U_1) and 3 for d = G - b (|d| <= M), d * strength, x + d (in [0, M]).  N = 8 L + 1 + 6 (L - 1) + 7 = 14 L + 2: 114 for eight
    levels.  The float64 run's own error is 2^-29 of that.  |fp32 - float64| <= N * 2^-24 * M; not tuned."""
    for (w, h) in G.SIZES:
        img = G.random_frame(w, h, 31, False)
        M = float(img[..., :3].max())
        for levels in G.LEVELS:
            opt = G.options(1.0, 0.0, levels, _weights(levels))
            assert sum(F(v) for v in opt["weights"]) <= 1.0 + 2.0 ** -22
            a = G.glare(img, False, opt).astype(np.float64)
            b = G.glare(img, False, opt, dtype=np.float64)
            bound = (14 * levels + 2) * 2.0 ** -24 * M
            err = float(np.abs(a - b).max())
            assert err <= bound, (w, h, levels, err, bound)


# ------------------------------------------------------------------------------------------------ level sizes and the GlareSet
def test_level_sizes_and_texel_counts(shim):
    for (w, h) in G.SIZES + ((2, 2), (96, 64), (1920, 1080), (1, 0), (0, 9), (0xFFFFFFFF, 1)):
        for k in range(0, 10):
            n = w
            for _ in range(k):
                n = (n + 1) // 2
            assert shim.glare_level_size(w, k) == n
        for levels in range(1, 9):
            assert shim.glare_pyramid_texels(w, h, levels) == G.pyramid_texels(w, h, levels), (w, h, levels)
    assert G.level_sizes(33, 130, 8) == [(17, 65), (9, 33), (5, 17), (3, 9), (2, 5), (1, 3), (1, 2), (1, 1)]   # odd at several levels
    assert G.pyramid_texels(64, 36) == 32 * 18 + 16 * 9 + 8 * 5 + 4 * 3 + 2 * 2 + 1 + 1 + 1


def test_glare_set_in_place_or_refused(shim):
    """The GlareSet against the stand-in allocator: off holds nothing; on holds exactly the eight levels' texels of the width and
    rows in place (odd and even frames; a frame without rows counts as one texel); a changed extent refits and says so; a refused
    allocation leaves the set not in place and holding nothing, and a later fit mends it; nothing leaks."""
    live0 = shim.alloc_live()
    s = shim.set_new()
    fresh = C.c_uint32(0)
    assert not shim.set_on(s) and not shim.set_in_place(s, 64, 36) and not shim.set_held(s)
    assert shim.set_fit(s, 64, 36, C.byref(fresh)) == 0 and fresh.value == 0 and not shim.set_held(s)   # off: a fit does nothing
    for (w, h) in ((64, 36), (33, 130), (17, 16), (1, 1), (1920, 1080)):
        assert shim.set_texels(w, h) == G.pyramid_texels(w, h, 8) == sum(a * b for a, b in G.level_sizes(w, h, 8))
    assert shim.set_texels(64, 0) == 1 and shim.set_texels(0, 0) == 1
    assert shim.set_toggle(s, 1, 64, 36) == 0 and shim.set_on(s) and shim.set_in_place(s, 64, 36)
    assert shim.set_capacity(s) == G.pyramid_texels(64, 36) and not shim.set_in_place(s, 64, 37) and not shim.set_in_place(s, 33, 130)
    assert shim.set_fit(s, 64, 36, C.byref(fresh)) == 0 and fresh.value == 0    # in place: nothing is reallocated
    assert shim.set_fit(s, 33, 130, C.byref(fresh)) == 0 and fresh.value == 1   # a resize: the pyramid follows
    assert shim.set_capacity(s) == G.pyramid_texels(33, 130) and shim.set_in_place(s, 33, 130) and not shim.set_in_place(s, 64, 36)
    assert shim.set_fit(s, 33, 0, C.byref(fresh)) == 0 and fresh.value == 1 and shim.set_capacity(s) == 1 and shim.set_in_place(s, 33, 0)
    shim.alloc_fail_at(1)                                                       # the refit's allocation is refused
    assert shim.set_fit(s, 17, 16, C.byref(fresh)) == 1 and fresh.value == 0
    assert shim.set_on(s) and not shim.set_held(s) and shim.set_capacity(s) == 0 and not shim.set_in_place(s, 17, 16) and not shim.set_in_place(s, 33, 0)
    shim.alloc_fail_at(0)
    assert shim.set_fit(s, 17, 16, C.byref(fresh)) == 0 and fresh.value == 1 and shim.set_in_place(s, 17, 16)   # a later fit mends it
    assert shim.set_toggle(s, 0, 17, 16) == 0 and not shim.set_on(s) and not shim.set_held(s)
    shim.alloc_fail_at(1)                                                       # turning the option on is refused: it stays off
    assert shim.set_toggle(s, 1, 64, 36) == 1 and not shim.set_on(s) and not shim.set_held(s)
    shim.alloc_fail_at(0)
    assert shim.set_toggle(s, 1, 64, 36) == 0 and shim.set_in_place(s, 64, 36)
    shim.set_delete(s)
    assert shim.alloc_live() == live0


def test_header_loop_under_address_and_undefined_behaviour_sanitizers():
    """tests/glare_main.cpp: a stand-alone program (its own main) over ptglare::run on exactly sized heap arrays — the six sizes,
    levels 1, 2, 5 and 8 (8 on the 1x1 frame too) —, built with -fsanitize=address,undefined and run as a child; nothing sanitized
    is loaded into this process"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "glare_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                               os.path.join(HERE, "glare_main.cpp"), "-o", exe])
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and "glare: ok" in out.stdout, out.stdout[-2000:]


# ------------------------------------------------------------------------------------------------ the surface
def test_symbol_and_signature(lib):
    assert hasattr(lib, "pt_glare") and "pt_glare" in SIGNATURES and "pt_glare" in ADDED_WITHIN_ABI_5
    assert lib.pt_abi_version() == 5 == abi.PT_ABI_VERSION   # added within the version
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint pt_glare\(pt_ctx\* ctx, const float\* src, const PtGlareOptions\* options, float\* rgba_out\);", header)
    # NULL arguments are refused before anything else is looked at
    good, hp = abi.PtGlareOptions(), (C.c_float * 4)()
    assert lib.pt_glare(None, None, C.byref(good), hp) == abi.PT_ERR_INVALID


def test_struct_and_constants_match_the_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "ptrace.h"
int main(void){
 PtGlareOptions d = PT_GLARE_OPTIONS_DEFAULT;
 printf("%zu %zu %zu %zu %zu %zu %d %d\n", sizeof(PtGlareOptions), offsetof(PtGlareOptions, strength), offsetof(PtGlareOptions, threshold),
   offsetof(PtGlareOptions, levels), offsetof(PtGlareOptions, _pad), offsetof(PtGlareOptions, weight), (int)PT_OPT_GLARE, (int)PT_GLARE_MAX_LEVELS);
 printf("%.9g %.9g %u %u", (double)d.strength, (double)d.threshold, d.levels, d._pad);
 for (int k = 0; k < PT_GLARE_MAX_LEVELS; k++) printf(" %.9g", (double)d.weight[k]);
 printf("\n");
 return 0; }'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        l1, l2 = subprocess.check_output([exe], text=True).strip().split("\n")
    O = abi.PtGlareOptions
    assert [int(x) for x in l1.split()] == [C.sizeof(O), O.strength.offset, O.threshold.offset, O.levels.offset, O._pad.offset, O.weight.offset,
                                            abi.PT_OPT_GLARE, abi.PT_GLARE_MAX_LEVELS]
    assert [int(x) for x in l1.split()] == [48, 0, 4, 8, 12, 16, 12, 8]
    d = O()
    assert [F(x) for x in l2.split()] == [F(v) for v in [d.strength, d.threshold, d.levels, d._pad] + list(d.weight)]
    assert (d.strength, d.threshold, d.levels) == (F(0.15), 0.0, 6) and list(d.weight) == [F(v) for v in (0.35, 0.25, 0.18, 0.12, 0.06, 0.04, 0, 0)]
    assert abs(sum(float(v) for v in d.weight) - 1.0) < 1e-6   # the default conserves energy
    ref = G.options()
    assert (F(ref["strength"]), ref["threshold"], ref["levels"]) == (d.strength, d.threshold, d.levels) and [F(v) for v in ref["weights"]] == list(d.weight)
    e = d.copy()
    e.levels = 3
    assert d.levels == 6 and e.levels == 3 and list(e.weight) == list(d.weight)


def test_rust_binding_declares_the_same():
    text = open(os.path.join(ROOT, "bindings", "rust", "ptrace_sys.rs")).read()
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    r = re.search(r"pub fn pt_glare\(([^)]*)\)", text)
    h = re.search(r"\bpt_glare\s*\(([^)]*)\)", header)
    assert r and h
    assert len([a for a in r.group(1).split(",") if a.strip()]) == len([a for a in h.group(1).split(",") if a.strip()]) == len(SIGNATURES["pt_glare"][1]) == 4
    body = re.search(r"pub struct PtGlareOptions \{(.*?)\n\}", text, flags=re.S).group(1)
    assert len(re.findall(r"pub \w+:", body)) == 5 == len(abi.PtGlareOptions._fields_)
    assert re.search(r"PT_OPT_GLARE: c_int = 12", text) and re.search(r"PT_GLARE_MAX_LEVELS: usize = 8", text)
    assert re.search(r"strength: 0\.15, threshold: 0\.0, levels: 6, _pad: 0, weight: \[0\.35, 0\.25, 0\.18, 0\.12, 0\.06, 0\.04, 0\.0, 0\.0\]", text)


def test_the_header_carries_the_statement_list():
    text = open(HEADER).read()
    for line in ("if !(Y - Y == 0):         b.c = 0", "else: t = Y - threshold ; if !(t > 0) b.c = 0 else { m = t / Y ;  b.c = x.c * m }",
                 "o = t0 + t3 ;  i = t1 + t2 ;  i = 3 * i ;  s = o + i ;  v = s * 0.125", "p = X >> 1 ;  q = (X odd) ? p + 1 : p - 1 ;  both clamped to [0, W - 1]",
                 "t = 3 * A[p] ;  t = t + A[q] ;  v = t * 0.25", "U_levels = weight[levels] * D_levels", "a = weight[k] * D_k ;  U_k = a + up(U_{k+1})",
                 "d = G.c - b.c ;  d = d * strength ;  out.c = x.c + d ;  out.w = 1"):
        assert line in text, line


def test_the_option_check_refuses_each_bad_field(shim):
    def valid(**kw):
        o = abi.PtGlareOptions()
        for k, v in kw.items():
            if k == "weight":
                o.weight[v[0]] = v[1]
            else:
                setattr(o, k, v)
        return shim.glare_options_valid(C.byref(o)) == 1

    nan, inf = float("nan"), float("inf")
    assert valid() and valid(strength=0.0) and valid(strength=1.0) and valid(levels=1) and valid(levels=8) and valid(threshold=1e30)
    for bad in (dict(strength=nan), dict(strength=1.0000001), dict(strength=-0.001), dict(strength=inf), dict(threshold=-1.0), dict(threshold=nan),
                dict(threshold=inf), dict(levels=0), dict(levels=9), dict(levels=0xFFFFFFFF), dict(weight=(0, -0.5)), dict(weight=(5, nan)),
                dict(weight=(2, inf)), dict(weight=(3, -inf))):
        assert not valid(**bad), bad
    # an unused weight may be anything (the default uses six levels)
    assert valid(weight=(6, nan)) and valid(weight=(7, -1.0)) and valid(levels=3, weight=(3, -inf))
    assert not valid(levels=7, weight=(6, nan))
    # weights are used as they are: they need not add up to 1
    assert valid(weight=(0, 100.0))


def test_render_tool_options():
    """--glare / --glare-levels / --glare-threshold: the default weights of the levels in use, rescaled to add up to 1; six levels are
    the header's default; values out of range give no options."""
    from ray_tracer_webgl_amd.render import glare_options

    d = abi.PtGlareOptions()
    o = glare_options(0.15, 6, 0.0)
    assert (o.strength, o.threshold, o.levels) == (d.strength, 0.0, 6) and np.allclose(list(o.weight), list(d.weight), rtol=0, atol=1e-7)
    for levels in range(1, 9):
        o = glare_options(0.4, levels, 2.0)
        assert o.levels == levels and o.threshold == 2.0 and abs(sum(list(o.weight)[:levels]) - 1.0) < 1e-6 and not any(list(o.weight)[levels:])
    for bad in ((-0.1, 6, 0.0), (1.5, 6, 0.0), (float("nan"), 6, 0.0), (0.15, 0, 0.0), (0.15, 9, 0.0), (0.15, 6, -1.0), (0.15, 6, float("inf"))):
        assert glare_options(*bad) is None, bad
