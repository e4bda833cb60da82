"""Temporal reprojection on the CPU: the properties of the contract (include/ptrace.h pt_reproject) shown on its numpy
restatement tests/reproject_ref.py, the header the kernel runs per thread (csrc/pt_reproject.hpp, through
tests/reproject_plan_shim.cpp) held against that restatement bit for bit on every frame used here, and THE QUALITY CONDITION:
on an eight-frame flight, history + one fresh pass must have less than half the fresh pass's squared error.  CPU only.

Measured on the flight at 96x54 (default scene, depth 6, 4 spp per frame, tolerance 2 px, caps 32 / 8; truth: 16 x 64 spp),
squared error of history + fresh over squared error of the fresh pass alone:
    frame 4: 0.250        frame 8: 0.282        kept pixels 0.645 / 0.643 of the frame (nearly all of the rest is sky)
The sweep over tolerance 1 to 8 px and caps 8 to 64 gives 0.25 to 0.38 at these two frames (profiles/r19_reproject.txt).
"""
import tempfile

import numpy as np
import pytest

import error_ref as ER
import feature_ref as FR
import reproject_ref as RR
from ray_tracer_webgl_amd import abi

W, H = 96, 54
CAPS = (32.0, 8.0)
TOL = 2.0


@pytest.fixture(scope="module")
def shim():
    return RR.build_shim(tempfile.mkdtemp(prefix="reproject_ref_"))


@pytest.fixture(scope="module")
def view(ora):
    """the default scene at 96x54: its planes and one 4-spp pass"""
    sph, p = ER.estimate_scene(W, H)
    return sph, p, FR.planes(sph, p), ora.render(sph, p, 1)[0]


@pytest.fixture(scope="module")
def hand():
    sph, p = ER.estimate_scene(131, 13)
    return p, RR.hand_frame(p)


def run(shim, f, prev, params, caps=CAPS, tol=TOL):
    """the restatement's output and tallies; the shared C++ header must give the same bits"""
    args = (f["cur_ids"], f["cur_pnt"], f["hist_ids"], f["hist_pnt"], f["acc"], prev, params, caps[0], caps[1], tol)
    out, tallies = RR.reproject(*args)
    got = RR.shim_reproject(shim, *args)
    assert RR.same_floats(got, out), RR.first_difference(got, out)
    return out, tallies


def test_identity_camera_keeps_every_hit_pixel_with_its_count(shim, view):
    sph, p, pl, acc = view
    f = {"cur_ids": pl["ids"], "cur_pnt": pl["point"], "hist_ids": pl["ids"], "hist_pnt": pl["point"], "acc": acc}
    out, tallies = run(shim, f, p, p)
    hit = pl["ids"][..., 0] >= 0
    assert 0.5 < hit.mean() < 0.8
    assert tallies == {"pixels": W * H, "pixels_hit": int(hit.sum()), "pixels_kept": int(hit.sum()), "samples_kept": 4 * int(hit.sum())}
    assert np.all(out[hit][:, 3] == acc[hit][:, 3]) and np.all(out[~hit] == 0)
    # the projection returns to the pixel's own centre up to the rounding of s and t (a few ulp of a number near 1, times the
    # width): a neighbour enters with a weight of at most ~96 x 8 x 2^-24 = 5e-5, colours are below ~2
    change = np.abs(out[hit][:, :3] / 4 - acc[hit][:, :3] / 4).max()
    print("identity camera: largest colour change %.3g" % change)
    assert change <= 1e-4


def test_caps_bind_per_material_class(shim, hand):
    p, f = hand
    diffuse = f["cur_ids"][..., 2] == abi.PT_DIFFUSE
    base, _ = run(shim, f, p, p, caps=(16777215.0, 16777215.0))
    assert (base[..., 3][diffuse] > 32).any() and (base[..., 3][~diffuse] > 8).any()
    out, _ = run(shim, f, p, p, caps=(32.0, 8.0))
    assert np.array_equal(out[..., 3][diffuse], np.minimum(base[..., 3][diffuse], 32))
    assert np.array_equal(out[..., 3][~diffuse], np.minimum(base[..., 3][~diffuse], 8))
    assert np.all(out[..., 3] == np.floor(out[..., 3]))   # counts stay whole numbers
    for caps, gone in (((0.0, 8.0), diffuse), ((32.0, 0.0), ~diffuse)):   # cap 0 keeps nothing of that class
        out, _ = run(shim, f, p, p, caps=caps)
        assert np.all(out[gone] == 0) and (out[..., 3][~gone] > 0).any()
    out, tallies = run(shim, f, p, p, caps=(0.0, 0.0))
    assert not out.any() and tallies["pixels_kept"] == 0 and tallies["samples_kept"] == 0


def test_tolerance_and_ids(shim, hand):
    p, f = hand
    cls = f["cls"]
    # tolerance 0: only exact coincidences of history and current point pass d2 <= 0
    # (the "centre" class looks at the history texel's own point; every other pixel is a fraction of a pixel away)
    same = np.all(f["cur_pnt"].view(np.uint32) == f["hist_pnt"].view(np.uint32), axis=-1)
    assert np.array_equal(same, cls == RR.CLASSES.index("centre"))
    out, _ = run(shim, f, p, p, tol=0.0)
    kept = out[..., 3] > 0
    assert kept[same].all() and not kept[~same].any()
    # a tolerance of a thousand pixels: the depth no longer decides, the index and the side still do
    out, _ = run(shim, f, p, p, tol=1000.0)
    assert (out[..., 3][cls == RR.CLASSES.index("other_depth")] > 0).any()
    assert not out[cls == RR.CLASSES.index("other_index")].any()
    assert not out[cls == RR.CLASSES.index("other_face")].any()
    out2, _ = run(shim, f, p, p)
    assert not out2[cls == RR.CLASSES.index("other_depth")].any()


def test_hostile_points_give_zeros(shim, hand):
    p, f = hand
    out, tallies = run(shim, f, p, p)
    cls = f["cls"]
    for name in ("miss", "behind", "outside_x", "outside_y", "nan", "inf", "ninf", "huge", "huge_ahead"):
        m = cls == RR.CLASSES.index(name)
        assert m.sum() >= 20, name
        assert not out[m].any(), name
    # the rims keep what lies inside the frame; non-finite colour stays non-finite
    for name in ("left_rim", "right_rim", "bottom_rim", "top_rim", "plain"):
        assert (out[..., 3][cls == RR.CLASSES.index(name)] > 0).any(), name
    assert np.isnan(out[..., 0]).any() and np.isinf(out[..., 1]).any()
    assert tallies["pixels_hit"] == int((f["cur_ids"][..., 0] >= 0).sum())


def test_degenerate_history_cameras_are_refused():
    sph, p = ER.estimate_scene(W, H)
    assert RR.constants(p, 2.0) is not None
    for field in ("horizontal", "vertical"):
        q = p.copy()
        setattr(q, field, abi.f3(0.0, 0.0, 0.0))
        assert RR.constants(q, 2.0) is None
    q = p.copy()
    q.lower_left_corner = q.camera_origin     # e = 0
    assert RR.constants(q, 2.0) is None
    q = p.copy()
    q.horizontal = abi.f3(float("nan"), 0.0, 0.0)
    assert RR.constants(q, 2.0) is None
    assert RR.constants(p, -1.0) is None and RR.constants(p, float("inf")) is None


def test_bands_gather_from_their_own_rows(shim):
    """three bands of four rows at 74x26: a band's output is the full-height output's wherever all four taps lie on rows
    it owns or outside the image, and only taps that cross to another band's row make a difference"""
    sph, p = ER.estimate_scene(74, 26)
    f = RR.hand_frame(p, seed=11)
    full, _ = run(shim, f, p, p)
    agree = differ = 0
    for r in range(3):
        q = p.copy()
        q.band_rows, q.band_index, q.band_count = 4, r, 3
        ys = np.asarray(FR.owned_rows(q))
        g = {k: v[ys] for k, v in f.items()}
        out, tallies = run(shim, g, p, q)
        assert tallies["pixels"] == len(ys) * 74
        live, y0 = RR.footprint_rows(g["cur_pnt"], p, q)
        own = np.zeros(27, bool)     # (row 26 = above the image: no tap)
        own[ys] = True
        foreign0 = (y0 >= 0) & ~own[np.clip(y0, 0, 26)]
        foreign1 = (y0 + 1 < 26) & ~own[np.clip(y0 + 1, 0, 26)]
        crosses = live & (foreign0 | foreign1)
        same = ((out.view(np.uint32) == full[ys].view(np.uint32)) | (np.isnan(out) & np.isnan(full[ys]))).all(-1)
        assert same[~crosses].all(), r
        agree += int(same[~crosses & (full[ys][..., 3] > 0)].sum())
        differ += int((~same).sum())
    assert agree > 300 and differ > 20


@pytest.fixture(scope="module")
def flight(ora, shim):
    """the eight-frame flight: per frame k >= 1 (fresh pass, history + fresh pass, kept share)"""
    sph, p0 = ER.estimate_scene(W, H)
    acc, planes, prev, frames = None, None, None, {}
    for k in range(9):
        p = RR.flight_params(p0, k)
        pl = FR.planes(sph, p)
        fresh = ora.render(sph, p, 1)[0]
        if k == 0:
            acc = fresh
        else:
            f = {"cur_ids": pl["ids"], "cur_pnt": pl["point"], "hist_ids": planes["ids"], "hist_pnt": planes["point"], "acc": acc}
            carried, tallies = run(shim, f, prev, p)
            acc = carried + fresh
            frames[k] = (fresh, acc, tallies["pixels_kept"] / tallies["pixels"], p)
        planes, prev = pl, p
    return sph, frames


@pytest.mark.parametrize("k", [4, 8])
def test_history_plus_fresh_has_less_than_half_the_fresh_error(ora, flight, k):
    sph, frames = flight
    fresh, acc, kept, p = frames[k]
    q = p.copy()
    q.samples_per_pixel, q.time = 64, 777777.0   # samples of their own
    truth = ora.render(sph, q, 16)[0]
    truth = truth[..., :3] / truth[..., 3:]
    err_fresh = float((((fresh[..., :3] / fresh[..., 3:]) - truth).astype(np.float64) ** 2).sum())
    err_both = float((((acc[..., :3] / acc[..., 3:]) - truth).astype(np.float64) ** 2).sum())
    print("flight frame %d at %dx%d: history + fresh / fresh = %.3f, kept pixels %.3f" % (k, W, H, err_both / err_fresh, kept))
    assert np.all(acc[..., 3] >= 4) and np.all(acc[..., 3] == np.floor(acc[..., 3]))
    assert 0.55 < kept < 0.70
    assert err_both < 0.5 * err_fresh
