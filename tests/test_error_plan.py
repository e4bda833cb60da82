"""The host arithmetic of the error estimate (csrc/pt_error_plan.hpp: the sums of pt_error_stats, THE SELECTION RULE, a tile's
in-image pixels) on the CPU, through tests/error_plan_shim.cpp, against the restatements the GPU tests use: tests/error_ref.py
(stats, same_stats: doubles as bit patterns) and tests/adaptive_ref.py (select, the per-tile pixel count).

The records and tallies come from error_ref.tiles(state), laid out as pt_error_stats copies them from the device.  States:
oracle passes folded by error_ref.fold, and hand-made ones for the branches oracle passes never reach.  Then the stand-alone
program tests/error_plan_main.cpp under the address and undefined-behaviour sanitizers.  CPU only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import adaptive_ref as A
import error_ref as E
import test_adaptive_ref as TA
from ray_tracer_webgl_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
SHAPES = {"64x36": (64, 36), "61x37": (61, 37), "9x9": (9, 9), "8x8": (8, 8), "1x1": (1, 1)}   # (width, rows)
TARGETS = (0.5, 0.2, 0.1, 0.05, 0.025, 0.01, 1e-6)
SATURATED = 4294967040.0   # the largest float below 2^32: from here on passes_min / passes_max read 0xffffffff


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(tempfile.mkdtemp(prefix="error_plan_"), "liberror_plan_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", os.path.join(HERE, "error_plan_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    fp, u32p, stp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(abi.PtErrorStats)
    lib.error_plan_stats.restype = None
    lib.error_plan_stats.argtypes = [fp, C.c_uint64, C.c_uint64, stp]
    lib.error_plan_reached.restype = C.c_int
    lib.error_plan_reached.argtypes = [stp, C.c_float]
    lib.error_plan_select.restype = C.c_uint32
    lib.error_plan_select.argtypes = [stp, C.c_float, fp, C.c_uint64, u32p]
    lib.error_plan_tile_pixels.restype = C.c_uint32
    lib.error_plan_tile_pixels.argtypes = [C.c_uint32] * 4
    return lib


def copied(state):
    """What pt_error_stats copies from the device for `state`: (2 n_tiles, 4) float32, records then tallies."""
    rec, tal = E.tiles(state)
    rec = rec.reshape(-1, 4)
    aux = np.zeros_like(rec)
    aux[:, 0], aux[:, 1], aux[:, 2] = tal["short"], tal["nonfinite"], tal["nmax"]
    return np.ascontiguousarray(np.concatenate([rec, aux]), dtype=np.float32)


def check(lib, state, what):
    """Stats, flags at every target and the reached rule of `state` against the restatements; returns (stats, flags per target)."""
    rows, width = state.shape[:2]
    h = copied(state)
    n_tiles = len(h) // 2
    hp = h.ctypes.data_as(C.POINTER(C.c_float))
    st = abi.PtErrorStats()
    st.passes_rendered, st.reached = 77, 99   # not the header's to set
    lib.error_plan_stats(hp, n_tiles, rows * width, C.byref(st))
    ref = E.stats(state)
    for k in ("passes_min", "passes_max"):   # error_ref.stats does not saturate; the header does, as pt_error_stats always has
        if ref[k] >= SATURATED:
            ref[k] = 0xffffffff
    assert E.same_stats(st, ref) == "", (what, E.same_stats(st, ref))
    assert (st.passes_rendered, st.reached) == (77, 99), what
    out = {}
    own = float(F(ref["rel_error"]))   # ... and the state's own figure as the target: tiles above the average, not those below
    for target in TARGETS + ((own,) if 0.0 < own < float("inf") else ()):
        flags = np.full(n_tiles, 7, np.uint32)
        n_active = lib.error_plan_select(C.byref(st), target, hp, n_tiles, flags.ctypes.data_as(C.POINTER(C.c_uint32)))
        want = A.select(state, target)
        assert flags.tolist() == want.astype(np.uint32).tolist(), (what, target)
        assert n_active == int(want.sum()), (what, target)
        reached = ref["rel_error"] <= float(F(target)) and ref["pixels_short"] == 0
        assert lib.error_plan_reached(C.byref(st), target) == int(reached), (what, target)
        out[target] = want
    return st, out


def ordinary(width, rows, seed=11):
    """n = 8, k = 32, means and M2 from a generator (the left half of the image a hundred times the M2 of the right): every pixel
    counted."""
    rng = np.random.default_rng(seed)
    st = E.empty_state(rows, width)
    st[..., 0, :3] = rng.uniform(0.5, 8.0, (rows, width, 3)).astype(np.float32)
    st[..., 0, 3] = 8.0
    st[..., 1, :3] = (rng.uniform(0.0, 4.0, (rows, width, 3)) * rng.choice([0.01, 1.0, 30.0], (rows, width, 1))).astype(np.float32)
    st[:, :(width + 1) // 2, 1, :3] *= F(100.0)
    st[..., 1, 3] = 32.0
    return st


# ------------------------------------------------------------------------------------------------ tile_pixels
@pytest.mark.parametrize("name", list(SHAPES))
def test_tile_pixels_against_the_restatement(shim, name):
    width, rows = SHAPES[name]
    ty, tx = A.tile_shape(rows, width)
    inside = A.pixel_mask(np.ones(ty * tx, bool), rows, width)
    per_tile = E._lanes(inside, False).sum(axis=1)          # as adaptive_ref.predicted counts them
    got = [shim.error_plan_tile_pixels(width, rows, tx, t) for t in range(ty * tx)]
    assert got == per_tile.tolist() and sum(got) == rows * width
    assert shim.error_plan_tile_pixels(width, rows, tx, ty * tx) == 0   # below the image


# ------------------------------------------------------------------------------------------------ oracle passes
@pytest.mark.parametrize("name", ["64x36", "61x37"])
def test_oracle_pass_states(shim, ora, name):
    width, rows = SHAPES[name]
    passes = TA._frame(ora, width, rows)
    st, acc = E.empty_state(rows, width), np.zeros((rows, width, 4), np.float32)
    mixed = done = 0
    for k in (1, 2, 4, 6):      # one pass: every pixel short
        st, acc = E.fold(st, acc, passes[done:k])
        done = k
        assert np.all(st[..., 0, 3] == k)
        stats, flags = check(shim, st, "%s after %d passes" % (name, k))
        assert stats.pixels_short == (rows * width if k == 1 else 0) and stats.passes_max == (0 if k == 1 else k)
        mixed += sum(1 for f in flags.values() if f.any() and not f.all())
    assert mixed >= 3   # not vacuous: the rule chose a proper subset of the tiles


# ------------------------------------------------------------------------------------------------ hand-made states
def _short(st):
    st[..., 0, 3] = 1.0


def _flat(st):
    st[..., 1, :3] = 0.0


def _dead_tile(st):      # n >= 2 and k = 0: not counted, not short
    st[:8, :8, 1, 3] = 0.0


def _nonfinite_tile(st):
    st[-1:, -1:, 0, 0] = np.inf          # the last tile holds one pixel of infinite radiance ...
    st[:8, :8, 0, :3] = np.nan           # ... and the first nothing else


def _saturated(st):
    st[..., 0, 3] = SATURATED
    st[:8, :8, 0, 3] = 2.0 ** 33


def _below_saturation(st):
    st[:8, :8, 0, 3] = 4294966784.0      # the float before SATURATED: passes_max reads it as it is


HAND = {"every pixel short": _short, "M2 = 0 everywhere": _flat, "a tile with no counted and no short pixel": _dead_tile,
        "non-finite radiance": _nonfinite_tile, "n at and above 4294967040": _saturated, "n below 4294967040": _below_saturation,
        "ordinary": lambda st: None}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind", list(HAND))
def test_hand_made_states(shim, shape, kind):
    width, rows = SHAPES[shape]
    state = ordinary(width, rows)
    HAND[kind](state)
    st, flags = check(shim, state, "%s, %s" % (shape, kind))
    n_tiles = len(flags[TARGETS[0]])
    if kind == "every pixel short":
        assert st.pixels_short == rows * width and st.pixels_counted == 0 and (st.passes_min, st.passes_max) == (0, 0)
        assert all(f.all() for f in flags.values())
    elif kind == "M2 = 0 everywhere":
        assert st.sum_e2 == 0.0 and st.rel_error == 0.0 and st.rms_error == 0.0 and st.sum_m2 > 0.0
        assert not any(f.any() for f in flags.values())
    elif kind == "a tile with no counted and no short pixel":
        assert st.pixels_nonfinite == min(8, rows) * min(8, width) and st.pixels_short == 0
        assert not any(f[0] for f in flags.values())
        assert (st.passes_min, st.passes_max) == ((8, 8) if n_tiles > 1 else (0, 0))
    elif kind == "non-finite radiance":
        assert st.pixels_nonfinite >= 1 and np.isfinite(st.sum_e2) and np.isfinite(st.sum_m2)
        assert not any(f[0] for f in flags.values())
    elif kind == "n at and above 4294967040":
        assert (st.passes_min, st.passes_max) == (0xffffffff, 0xffffffff)
    elif kind == "n below 4294967040":
        assert st.passes_max == 4294966784 and st.passes_min == (8 if n_tiles > 1 else 4294966784)
    else:
        assert st.pixels_counted == rows * width and (st.passes_min, st.passes_max) == (8, 8)
        if n_tiles > 1:
            assert any(f.any() and not f.all() for f in flags.values())


def test_no_tiles_at_all(shim):
    st = abi.PtErrorStats()
    shim.error_plan_stats(None, 0, 0, C.byref(st))
    assert (st.sum_e2, st.sum_m2, st.rel_error, st.rms_error, st.pixels, st.pixels_counted, st.passes_min, st.passes_max) == (0,) * 8
    assert shim.error_plan_select(C.byref(st), 0.1, None, 0, None) == 0


# ------------------------------------------------------------------------------------------------ sanitizers
def test_both_plans_under_address_and_undefined_behaviour_sanitizers():
    """tests/error_plan_main.cpp: a stand-alone program (its own main) over pt_error_plan.hpp and pt_tile_order.hpp at the shapes
    above, built with -fsanitize=address,undefined and run as a child; nothing sanitized is loaded into this process"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "error_plan_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(HERE, "error_plan_main.cpp"), "-o", exe])
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and "error plan: ok" in out.stdout, out.stdout[-2000:]
