"""Temporal reprojection with the error estimate on the CPU (include/ptrace.h pt_reproject_estimate): the
properties of the contract shown on its numpy restatement tests/reproject_estimate_ref.py; the header the kernel runs per thread
(csrc/pt_reproject.hpp reproject_pixel_estimate, through tests/reproject_estimate_shim.cpp) held against that restatement bit
for bit on every frame used here — its accumulation output against reproject_ref.reproject, i.e. pt_reproject's bits; the
stand-alone program tests/reproject_estimate_main.cpp under the address and undefined-behaviour sanitizers; the surface of the
entry point; and THE QUALITY CONDITION.  CPU only; nothing sanitized is loaded into this process.

THE QUALITY CONDITION, on §4.8g's eight-frame flight at 96x54 (default scene, depth 6, tolerance 2 px, caps 32 / 8, 4 passes of
1 spp per tick, truth 16 x 64 spp at clock 777777): at frames 4 and 8 the carried state folded with the tick's fresh passes and read
through patch_filter_ref.filtered(state, 2, 1, 1.5) must have strictly less squared error than (a) the reprojected accumulation,
unfiltered, and (b) the fresh passes alone through the same filter.  The restatement's figures, squared error over the squared
error of the tick's 4 fresh samples unfiltered:
    frame   carried + filter   (a) reprojected, unfiltered   (b) fresh + filter   carried / better of (a), (b)
      4         0.214                  0.266                       0.334                  0.80
      8         0.265                  0.286                       0.339                  0.93
CALIBRATION of the carried estimate, sum (m - truth)^2 / sum se^2 over the known pixels of the state the filter reads (1 = the
standard error says how far the mean lies from the truth): frame 1: 0.93, frame 4: 0.95, frame 8: 1.26.  It drifts upwards:
what lags behind the camera (reflections, refractions) is bias the standard error does not know of.  The carried estimate steers
a filter; it is no stopping criterion.  Recorded, and asserted only to be finite and positive.
"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import error_ref as ER
import feature_ref as FR
import patch_filter_ref as PF
import reproject_estimate_ref as REF
import reproject_ref as RR
from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd._lib import ADDED_WITHIN_ABI_5, SIGNATURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
W, H = 96, 54
CAPS = (32.0, 8.0)
TOL = 2.0


@pytest.fixture(scope="module")
def shim():
    return REF.build_shim(tempfile.mkdtemp(prefix="reproject_estimate_ref_"))


def run(shim, f, state, S, prev, params, caps=CAPS, tol=TOL):
    """the restatement's (out, state', tallies); the shared C++ header must give the same bits for both outputs, and the
    accumulation's are reproject_ref.reproject's"""
    args = (f["cur_ids"], f["cur_pnt"], f["hist_ids"], f["hist_pnt"], f["acc"])
    out, new, tallies = REF.reproject_estimate(*args, state, S, prev, params, caps[0], caps[1], tol)
    base, _ = RR.reproject(*args, prev, params, caps[0], caps[1], tol)
    assert RR.same_floats(out, base)
    got_out, got_new = REF.shim_reproject_estimate(shim, *args, state, S, prev, params, caps[0], caps[1], tol)
    assert RR.same_floats(got_out, base), "accumulation: " + RR.first_difference(got_out, base)
    assert RR.same_floats(got_new, new), "state: " + RR.first_difference(got_new, new)
    return out, new, tallies


def assert_well_formed(new, S):
    """n' is a whole number >= 2 and k' = n' S exactly, or the texel is all zero"""
    n, k = new[..., 0, 3], new[..., 1, 3]
    empty = ~(n >= 2)
    assert not new[empty].any()
    assert np.all(n[~empty] == np.floor(n[~empty])) and np.all(k[~empty] == n[~empty] * F(S))


@pytest.fixture(scope="module")
def view(ora):
    """the default scene at 96x54: its planes, and a state of eight folded passes of 4 spp"""
    sph, p = ER.estimate_scene(W, H)
    st, acc = ER.fold(ER.empty_state(H, W), np.zeros((H, W, 4), np.float32), ER.oracle_passes(ora, sph, p, 8))
    return sph, p, FR.planes(sph, p), st, acc


@pytest.fixture(scope="module")
def hand():
    sph, p = ER.estimate_scene(131, 13)
    f = RR.hand_frame(p)
    st, cls = REF.hand_state(13, 131)
    return p, f, st, cls


# ------------------------------------------------------------------------------------------------ the surface
def test_the_symbol_is_exported_declared_and_refuses_null(lib):
    name = "pt_reproject_estimate"
    assert hasattr(lib, name) and name in SIGNATURES and name in ADDED_WITHIN_ABI_5
    assert SIGNATURES[name] == SIGNATURES["pt_reproject"]
    assert lib.pt_abi_version() == 5 == abi.PT_ABI_VERSION
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptrace.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "ptrace_sys.rs")).read()
    h = re.search(r"\bint %s\s*\(([^)]*)\)" % name, header)
    r = re.search(r"pub fn %s\(([^)]*)\)" % name, rust)
    assert h and r and len(h.group(1).split(",")) == len(r.group(1).split(",")) == 2
    opt = abi.PtReprojectOptions()
    assert lib.pt_reproject_estimate(None, C.byref(opt)) == abi.PT_ERR_INVALID   # no device is needed to see that
    assert lib.pt_reproject_estimate(None, None) == abi.PT_ERR_INVALID


def test_the_contract_is_written_in_the_same_words_in_header_design_and_restatement():
    def statements(text):
        block = text[text.index("host, once: S = err_spp"):]
        block = block[:block.index("(a pixel that is `done` before the taps leaves A' = B' = all +0)")]
        lines = [re.sub(r"^[\s*]+", "", ln) for ln in block.splitlines()]
        return [re.sub(r"\s+", " ", ln).strip() for ln in lines if ln.strip()]

    header = statements(open(os.path.join(ROOT, "include", "ptrace.h")).read())
    design = statements(open(os.path.join(ROOT, "DESIGN.md")).read())
    ref = statements(REF.__doc__)
    assert len(ref) == 13
    assert header == ref and design == ref


def test_host_constants(shim):
    for S, caps in ((1, (32.0, 8.0)), (4, (32.0, 8.0)), (4, (7.0, 4.0)), (3, (16777215.0, 0.0)), (25, (32.0, 8.0))):
        out = np.zeros(4, np.float32)
        shim.reproject_estimate_constants(S, caps[0], caps[1], out.ctypes.data_as(C.POINTER(C.c_float)))
        ref = np.array(REF.host_constants(S, *caps), np.float32)
        assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), (S, caps)
        assert out[2] == caps[0] // S and out[3] == caps[1] // S


# ------------------------------------------------------------------------------------------------ the restatement's properties
def test_identity_camera_keeps_n_and_the_read_out(shim, view):
    """Eight passes of 4 spp everywhere, caps of 16 passes: every hit pixel keeps n = 8 (a power of two: g*n is exact, so
    cntE = 8 wsumE exactly whatever the weights) and k = 32.  The projection returns to the pixel's own centre up to the rounding
    of s and t, so a neighbour enters with a weight w <= ~96 x 8 x 2^-24 = 5e-5 (test_reproject_ref.py): the read-out's m moves
    by at most w x (colours below ~4) and se^2 by at most w x the largest se^2 of the frame, plus a few ulp of rounding.
    Observed: |dm| <= 1.8e-6, |d se^2| <= 3.4e-8 = 3.6e-6 of the largest se^2; bounds: w x 4 = 2e-4, and 2 w = 1e-4 of the largest
    se^2."""
    sph, p, pl, st, acc = view
    f = {"cur_ids": pl["ids"], "cur_pnt": pl["point"], "hist_ids": pl["ids"], "hist_pnt": pl["point"], "acc": acc}
    out, new, tallies = run(shim, f, st, 4, p, p, caps=(64.0, 64.0))
    hit = pl["ids"][..., 0] >= 0
    assert 0.5 < hit.mean() < 0.8
    assert np.all(st[..., 0, 3] == 8) and np.all(st[..., 1, 3] == 32)
    assert np.all(new[hit][:, 0, 3] == 8) and np.all(new[hit][:, 1, 3] == 32) and not new[~hit].any()
    se0, m0, _ = ER.pixel_error(st)
    se1, m1, known = ER.pixel_error(new)
    assert np.array_equal(known, hit)
    dm = np.abs(m1[hit] - m0[hit]).max()
    v0, v1 = se0[hit].astype(np.float64) ** 2, se1[hit].astype(np.float64) ** 2
    dv = np.abs(v1 - v0).max()
    print("identity camera: |dm| <= %.3g, |d se^2| <= %.3g = %.3g of the largest se^2" % (dm, dv, dv / v0.max()))
    assert dm <= 2e-4 and dv <= 1e-4 * v0.max()
    assert tallies["pixels_kept"] == int(hit.sum())


def test_caps_bind_per_material_class_in_passes(shim, hand):
    p, f, st, cls = hand
    diffuse = f["cur_ids"][..., 2] == abi.PT_DIFFUSE
    S = 4
    _, base, _ = run(shim, f, st, S, p, p, caps=(16777215.0, 16777215.0))
    assert_well_formed(base, S)
    n0 = base[..., 0, 3]
    assert (n0[diffuse] > 8).any() and (n0[~diffuse] > 3).any()
    # 35 / 4 -> 8 passes, 14 / 4 -> 3 passes: the cap counts whole passes
    _, new, _ = run(shim, f, st, S, p, p, caps=(35.0, 14.0))
    assert_well_formed(new, S)
    n1 = new[..., 0, 3]
    with np.errstate(invalid="ignore"):
        assert np.array_equal(n1[diffuse], np.where(n0[diffuse] >= 2, np.minimum(n0[diffuse], 8), 0))
        assert np.array_equal(n1[~diffuse], np.where(n0[~diffuse] >= 2, np.minimum(n0[~diffuse], 3), 0))
    # a cap that bites leaves the per-sample mean alone and widens the standard error: se'^2 = W / nE
    bites = diffuse & (n0 > 8) & np.isfinite(base).all(axis=(-1, -2)) & np.isfinite(new).all(axis=(-1, -2))
    assert bites.sum() > 20
    se_b, m_b, _ = ER.pixel_error(base)
    se_n, m_n, _ = ER.pixel_error(new)
    assert np.allclose(m_b[bites], m_n[bites], rtol=1e-6, atol=0) and np.all(se_n[bites] >= se_b[bites])
    # a class whose cap is below 2 passes carries no estimate (7 / 4 -> 1 pass); the accumulation still carries its samples
    for caps, gone in (((7.0, 8.0), diffuse), ((32.0, 7.0), ~diffuse), ((32.0, 0.0), ~diffuse)):
        out, new, _ = run(shim, f, st, S, p, p, caps=caps)
        assert not new[gone].any() and (new[..., 0, 3][~gone] >= 2).any()
    out, new, _ = run(shim, f, st, S, p, p, caps=(7.0, 7.0))
    assert not new.any() and (out[..., 3] > 0).any()


def test_a_state_that_knows_nothing_carries_nothing(shim, hand):
    p, f, st, cls = hand
    for n, k in ((1.0, 4.0), (0.0, 0.0), (8.0, 0.0), (8.0, -32.0), (-2.0, 8.0), (np.nan, 8.0), (8.0, np.nan)):
        s = st.copy()
        s[..., 0, 3], s[..., 1, 3] = n, k
        out, new, _ = run(shim, f, s, 4, p, p)
        assert not new.any(), (n, k)
        assert (out[..., 3] > 0).any()


def test_nothing_folded_since_the_last_clear_is_a_clear(hand):
    p, f, st, cls = hand
    out, new, tallies = REF.reproject_estimate(f["cur_ids"], f["cur_pnt"], f["hist_ids"], f["hist_pnt"], f["acc"], st, 0, p, p,
                                               CAPS[0], CAPS[1], TOL)
    base, base_tallies = RR.reproject(f["cur_ids"], f["cur_pnt"], f["hist_ids"], f["hist_pnt"], f["acc"], p, p, CAPS[0], CAPS[1], TOL)
    assert not new.any() and RR.same_floats(out, base) and tallies == base_tallies


def test_hostile_operands_in_the_state(shim, hand):
    """NaN, inf, negative n, k = 0, n = 1, huge M2: no index depends on the state (the bounds-checked program below shows it),
    texels that are not known (n < 2, k <= 0, NaN) are skipped as taps, non-finite values stay non-finite in a well-formed
    texel, and the estimate's sums do not depend on a.w > 0"""
    p, f, st, cls = hand
    assert all((cls == i).sum() >= 20 for i in range(len(REF.STATE_CLASSES)))
    S = 4
    out, new, _ = run(shim, f, st, S, p, p)
    assert_well_formed(new, S)   # n' whole and >= 2, k' = n' S — also where colours are NaN or inf
    fcls = f["cls"]
    for name in ("miss", "behind", "outside_x", "outside_y", "nan", "inf", "ninf", "huge", "huge_ahead", "other_index", "other_face"):
        m = fcls == RR.CLASSES.index(name)
        assert m.sum() >= 20 and not new[m].any(), name
    assert np.isnan(new[..., 0, :3]).any() and np.isinf(new[..., 0, :3]).any()
    assert np.isnan(new[..., 1, :3]).any() and np.isinf(new[..., 1, :3]).any() and (new[..., 1, :3] < 0).any()
    assert np.isinf(new[..., 1, :3][np.isfinite(st[..., 1, :3]).all(-1)]).any() or (new[..., 1, :3] > 1e37).any()   # huge M2 survives or overflows
    # tolerance 0: a "centre" pixel gathers from the one history texel that holds its own point and nothing else does (see
    # test_reproject_ref.py): an unknown texel there carries nothing, a known one is carried with its own count, capped
    _, new_c, _ = run(shim, f, st, S, p, p, tol=0.0)
    centre = fcls == RR.CLASSES.index("centre")
    with np.errstate(invalid="ignore"):
        unknown = ~((st[..., 0, 3] >= 2) & (st[..., 1, 3] > 0))
    assert (centre & unknown).sum() >= 3 and not new_c[centre & unknown].any() and not new_c[~centre].any()
    capP = np.where(f["cur_ids"][..., 2] == abi.PT_DIFFUSE, 8, 2)
    assert np.array_equal(new_c[..., 0, 3][centre & ~unknown], np.minimum(st[..., 0, 3], capP)[centre & ~unknown])
    # the estimate does not depend on a.w > 0: an empty accumulation keeps nothing, the state is carried all the same
    g = dict(f)
    g["acc"] = np.zeros_like(f["acc"])
    out0, new0, _ = run(shim, g, st, S, p, p)
    assert not out0.any() and RR.same_floats(new0, new)
    # n = inf in a tap: the blended count is inf, capped; k = inf in a tap: qq = 0, its mean and variance enter as zeros
    assert (new[..., 0, 3] == 8).any()


def test_two_band_ranks_with_a_partial_last_chunk(shim):
    """74x26 in bands of 4 rows over 2 ranks (the last chunk, rows 24 and 25, is partial and rank 0's): a band's state is the
    full-height state's wherever all four taps lie on rows it owns or outside the image; only taps that cross to the other
    band's rows make a difference"""
    sph, p = ER.estimate_scene(74, 26)
    f = RR.hand_frame(p, seed=11)
    st, _ = REF.hand_state(26, 74, seed=12)
    _, full, _ = run(shim, f, st, 4, p, p)
    agree = differ = 0
    for r in range(2):
        q = p.copy()
        q.band_rows, q.band_index, q.band_count = 4, r, 2
        ys = np.asarray(FR.owned_rows(q))
        assert len(ys) == (14 if r == 0 else 12)
        g = {k: v[ys] for k, v in f.items()}
        _, new, tallies = run(shim, g, st[ys], 4, p, q)
        assert tallies["pixels"] == len(ys) * 74
        live, y0 = RR.footprint_rows(g["cur_pnt"], p, q)
        own = np.zeros(27, bool)
        own[ys] = True
        foreign0 = (y0 >= 0) & ~own[np.clip(y0, 0, 26)]
        foreign1 = (y0 + 1 < 26) & ~own[np.clip(y0 + 1, 0, 26)]
        crosses = live & (foreign0 | foreign1)
        a, b = new.reshape(len(ys), 74, 8), full[ys].reshape(len(ys), 74, 8)
        same = ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all(-1)
        assert same[~crosses].all(), r
        agree += int(same[~crosses & (full[ys][..., 0, 3] > 0)].sum())
        differ += int((~same).sum())
    assert agree > 300 and differ > 20


# ------------------------------------------------------------------------------------------------ the sanitizer build
def test_per_pixel_header_under_address_and_undefined_behaviour_sanitizers(hand):
    """tests/reproject_estimate_main.cpp: a stand-alone program (its own main), built with -fsanitize=address,undefined and
    run as a child over the files written here: the 131x13 hand-made frame and state with every operand class at three settings,
    the same as two bands of four rows, and one-texel, one-column and 3x2 frames"""
    p, f, st, cls = hand
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "reproject_estimate_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", os.path.join(HERE, "reproject_estimate_main.cpp"), "-o", exe])
        files = []

        def add(f, st, S, prev, params, caps, tol):
            files.append(os.path.join(tmp, "frame%d.bin" % len(files)))
            REF.write_main_file(files[-1], f["cur_ids"], f["cur_pnt"], f["hist_ids"], f["hist_pnt"], f["acc"], st, S, prev, params,
                                caps[0], caps[1], tol)

        for S, caps, tol in ((4, (32.0, 8.0), 2.0), (1, (16777215.0, 0.0), 1000.0), (3, (7.0, 100.0), 0.5)):
            add(f, st, S, p, p, caps, tol)
        for r in range(2):
            q = p.copy()
            q.band_rows, q.band_index, q.band_count = 4, r, 2
            ys = abi.owned_rows(13, 4, r, 2)
            add({k: v[ys] for k, v in f.items()}, st[ys], 4, p, q, (32.0, 8.0), 2.0)
        for w, h in ((1, 1), (1, 9), (3, 2)):
            sph, q = ER.estimate_scene(w, h)
            add(RR.hand_frame(q, seed=w + h), REF.hand_state(h, w, seed=w)[0], 4, q, q, (32.0, 8.0), 4.0)
        out = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and "reproject estimate: ok (%d files)" % len(files) in out.stdout, out.stdout[-2000:]


# ------------------------------------------------------------------------------------------------ the quality condition
PASSES = 4   # per tick, of 1 spp each


@pytest.fixture(scope="module")
def flight(ora, shim):
    """the eight-frame flight with 1 spp x 4 passes per tick: per frame k >= 1 (fresh passes folded alone, carried state folded
    with them, the accumulation, the view)"""
    sph, p0 = ER.estimate_scene(W, H, spp=1)
    acc, st, planes, prev, frames = None, None, None, None, {}
    empty, zeros = ER.empty_state(H, W), np.zeros((H, W, 4), np.float32)
    for k in range(9):
        p = RR.flight_params(p0, k)
        pl = FR.planes(sph, p)
        passes = ER.oracle_passes(ora, sph, p, PASSES)
        fresh_st, fresh_acc = ER.fold(empty, zeros, passes)
        if k == 0:
            st, acc = fresh_st, fresh_acc
        else:
            f = {"cur_ids": pl["ids"], "cur_pnt": pl["point"], "hist_ids": planes["ids"], "hist_pnt": planes["point"], "acc": acc}
            carried_acc, carried_st, _ = run(shim, f, st, 1, prev, p)
            assert_well_formed(carried_st, 1)
            st, acc = ER.fold(carried_st, carried_acc, passes)
            frames[k] = (fresh_st, fresh_acc, st, acc, p)
        planes, prev = pl, p
    return sph, frames


def truth_of(ora, sph, p):
    q = p.copy()
    q.samples_per_pixel, q.time = 64, 777777.0   # samples of their own
    t = ora.render(sph, q, 16)[0]
    return (t[..., :3] / t[..., 3:]).astype(np.float64)


def sq(img, truth):
    return float(((img.astype(np.float64) - truth) ** 2).sum())


def calibration(st, truth):
    se, m, known = ER.pixel_error(st)
    return sq(m[known], truth[known]) / float((se[known].astype(np.float64) ** 2).sum())


@pytest.mark.parametrize("k", [4, 8])
def test_carried_and_filtered_beats_what_exists(ora, flight, k):
    """the quality condition (the figures stand in this module's docstring)"""
    sph, frames = flight
    fresh_st, fresh_acc, st, acc, p = frames[k]
    truth = truth_of(ora, sph, p)
    e_fresh = sq(fresh_acc[..., :3] / fresh_acc[..., 3:], truth)
    e_carried = sq(PF.filtered(st, 2, 1, 1.5)[..., :3], truth)
    e_reprojected = sq(acc[..., :3] / acc[..., 3:], truth)
    e_fresh_filtered = sq(PF.filtered(fresh_st, 2, 1, 1.5)[..., :3], truth)
    cal = calibration(st, truth)
    print("flight frame %d at %dx%d, over the fresh samples' squared error: carried + filter %.3f, (a) reprojected unfiltered %.3f, "
          "(b) fresh + filter %.3f; carried / better alternative %.2f; calibration %.2f"
          % (k, W, H, e_carried / e_fresh, e_reprojected / e_fresh, e_fresh_filtered / e_fresh,
             e_carried / min(e_reprojected, e_fresh_filtered), cal))
    assert np.isfinite(cal) and cal > 0
    assert e_carried < e_reprojected
    assert e_carried < e_fresh_filtered


def test_calibration_of_the_carried_estimate_at_the_first_frame(ora, flight):
    sph, frames = flight
    fresh_st, fresh_acc, st, acc, p = frames[1]
    cal = calibration(st, truth_of(ora, sph, p))
    print("flight frame 1: calibration of the carried estimate %.2f" % cal)
    assert np.isfinite(cal) and cal > 0
