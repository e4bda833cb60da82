"""The variance-guided filtered read-out on the device (pt_resolve_filtered: pt_filter_kernel) against the plain numpy
restatement of its statements (tests/filter_ref.py, itself held to its properties by tests/test_filter_ref.py without a GPU).

Most states go in through load_error_state, so no trace launch is needed; floats are compared as bit patterns except where
both sides are NaN (error_ref.same_floats); no tolerance and no clock anywhere."""
import ctypes as C

import numpy as np
import pytest

import error_ref as E
import filter_ref as FR
from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd.tracer import PathTracer, PtError

pytestmark = pytest.mark.gpu

F = np.float32


def _context(w, h, band=None, spp=4, reserve=2, estimate=True):
    spheres, p = E.estimate_scene(w, h, spp=spp, band=band)
    t = PathTracer(p.width, p.height)
    t.set_spheres(spheres)
    t.set_params(p)
    t.reserve_passes(reserve)
    if estimate:
        t.error_estimate(True)
    return t, p


def _loaded(state, band=None, height=None):
    rows, width = state.shape[:2]
    t, _ = _context(width, rows if height is None else height, band=band)
    assert (t.local_rows, t.width) == (rows, width)
    t.load_error_state(state)
    return t


def _check(t, state, radius, kappa, gamma, what, band_rows=0):
    got = t.filtered_image(radius, kappa, gamma=gamma)
    ref = FR.filtered(state, radius, kappa, gamma=gamma, band_rows=band_rows)
    assert E.same_floats(got, ref), "%s, radius %d, kappa %g, gamma %d: %s" % (what, radius, kappa, gamma, E.first_difference(got, ref))
    return got


@pytest.fixture(scope="module")
def hand():
    state, _ = E.hand_state()
    t = _loaded(state)
    yield t, state
    t.close()


@pytest.fixture(scope="module")
def ordinary():
    state = FR.ordinary_state(E.HAND_W, E.HAND_H, seed=13)
    t = _loaded(state)
    yield t, state
    t.close()


@pytest.mark.parametrize("gamma", [0, 1])
@pytest.mark.parametrize("radius", range(0, abi.PT_FILTER_MAX_RADIUS + 1))
def test_hand_made_state_at_every_radius(hand, radius, gamma):
    """131x13: every operand class of n, k and M2, full and edge tiles of the kernel (32x8), a seam at x = 32, 64, 96 and 128
    and at y = 8."""
    t, state = hand
    got = _check(t, state, radius, 2.0, gamma, "hand-made state")
    _, m, cntd = FR.counted(state)
    assert np.all(got[..., 3][~cntd] == 0.0) and np.all(got[..., 3][cntd] >= 1.0)
    if radius == 0:
        with np.errstate(all="ignore"):
            assert E.same_floats(got[..., :3], np.sqrt(m) if gamma else m)
    if radius == 2:
        assert got[..., 3].min() == 0.0 and got[..., 3].max() == 25.0


@pytest.mark.parametrize("kappa,mean_taps", [(0.5, 1.0), (2.0, 1.4), (8.0, 18.7), (32.0, 66.0)])
def test_ordinary_state_from_everything_rejected_to_everything_accepted(ordinary, kappa, mean_taps):
    """mean uniform in [0.5, 8), M2 uniform in [0, 4), n 8, k 32 at 131x13, radius 4."""
    t, state = ordinary
    got = _check(t, state, 4, kappa, 0, "ordinary state")
    assert abs(float(got[..., 3].mean()) - mean_taps) <= 0.1 * mean_taps, float(got[..., 3].mean())
    if kappa == 32.0:
        assert got[..., 3].max() == 81.0
    if kappa == 0.5:
        assert got[..., 3].max() <= 2.0


@pytest.mark.parametrize("shape", [(3, 2), (1, 1), (33, 9), (61, 37)])
def test_shapes_below_a_tile_and_a_radius_and_just_past_one(shape):
    w, h = shape
    state = FR.ordinary_state(w, h, seed=w * 100 + h)
    state[..., 1, :3] *= F(40.0)                # wide enough that kappa 2 accepts a good share of the taps
    if w > 2:
        state[h // 2, w // 2, 0, 3] = 1.0       # ... and a short pixel inside
    t = _loaded(state)
    for radius in (0, 1, 2, 4):
        got = _check(t, state, radius, 2.0, 1, "%dx%d" % shape)
    assert got[..., 3].max() > 1.0 or w * h == 1
    t.close()


@pytest.mark.parametrize("index", [0, 1])
def test_band_context_filters_inside_its_chunks(index):
    """band_rows 3, band_count 2 on a height of 37: chunks of three image rows dealt in turn, the last chunk (image row 36) partial.
    Both band indices against the restatement with band_rows 3."""
    height, width = 37, 61
    rows = abi.local_rows(height, 3, index, 2)
    assert rows == (19, 18)[index]
    state = FR.ordinary_state(width, rows, seed=21 + index)
    state[..., 1, :3] *= F(40.0)
    t = _loaded(state, band=(3, index, 2), height=height)
    for radius, kappa in ((1, 2.0), (2, 2.0), (4, 8.0)):
        got = _check(t, state, radius, kappa, 0, "band %d of 2" % index, band_rows=3)
    assert got[..., 3].max() == 27.0        # three rows of nine taps: nothing crossed a chunk
    whole = FR.filtered(state, 4, 8.0)
    assert not E.same_floats(got, whole)
    t.close()


def test_device_pointer_gives_the_bytes_of_a_host_pointer(hand):
    """The device memory is a second context's error state, 32 bytes per pixel: the read-out fills its first half."""
    t, state = hand
    host = t.filtered_image(2, 2.0, gamma=True)
    other = _loaded(np.full_like(state, -1.0))
    ptr, nbytes = C.c_void_p(), C.c_size_t()
    assert other.lib.pt_error_ptr(other._ctx, C.byref(ptr), C.byref(nbytes)) == abi.PT_OK and nbytes.value == 2 * host.nbytes
    assert t.lib.pt_resolve_filtered(t._ctx, ptr, 2, 2.0, 1) == abi.PT_OK
    buf = other.error_state().reshape(-1)
    assert buf[:host.size].tobytes() == host.tobytes() and np.all(buf[host.size:] == -1.0)
    other.close()


def test_rendered_frame_and_the_call_leaves_accum_and_state_untouched():
    """64x36, 8 passes of 4 spp through pt_render_passes."""
    t, p = _context(64, 36, reserve=8)
    t.render_passes(8)
    state, accum = t.error_state(), t.accum()
    assert np.all(state[..., 0, 3] == 8.0) and np.all(state[..., 1, 3] == 32.0)
    for radius in (0, 2, 4):
        for gamma in (0, 1):
            got = _check(t, state, radius, 2.0, gamma, "rendered 64x36")
    assert got[..., 3].mean() > 4.0
    assert t.error_state().tobytes() == state.tobytes() and t.accum().tobytes() == accum.tobytes()
    # the estimate's own mean is the frame's: radius 0 against pt_resolve to rounding (mean * n / k against sum / k)
    plain = t.resolve(gamma=False)
    assert np.allclose(t.filtered_image(0, 2.0, gamma=False)[..., :3], plain[..., :3], rtol=1e-5, atol=1e-7)
    t.close()


def test_after_two_partial_rounds_of_adaptive_sampling():
    """Pixels of one frame hold different numbers of passes: every tap divides by its own pixel's count."""
    t, p = _context(64, 36, reserve=2)
    st, ad = t.render_adaptive(0.025, 2, 6)
    assert (ad.rounds, ad.partial_rounds) == (3, 2) and st.passes_min < st.passes_max
    state = t.error_state()
    assert len(np.unique(state[..., 0, 3])) >= 2
    for radius in (1, 2, 4):
        _check(t, state, radius, 2.0, 1, "adaptive 64x36")
    assert t.error_state().tobytes() == state.tobytes()
    t.close()


def test_error_paths():
    t, p = _context(64, 36, estimate=False)
    lib = t.lib
    out = np.full((p.height, p.width, 4), 7.0, np.float32)
    ptr = out.ctypes.data_as(C.c_void_p)
    assert lib.pt_resolve_filtered(t._ctx, ptr, 2, 2.0, 1) == abi.PT_ERR_NOT_READY
    assert b"estimate is off" in (lib.pt_last_error(t._ctx) or b"")
    with pytest.raises(PtError):
        t.filtered_image()
    t.error_estimate(True)
    assert lib.pt_resolve_filtered(t._ctx, None, 2, 2.0, 1) == abi.PT_ERR_INVALID
    assert lib.pt_resolve_filtered(t._ctx, ptr, abi.PT_FILTER_MAX_RADIUS + 1, 2.0, 1) == abi.PT_ERR_INVALID
    assert lib.pt_resolve_filtered(t._ctx, ptr, 0xffffffff, 2.0, 1) == abi.PT_ERR_INVALID
    for bad in (float("nan"), float("inf"), -float("inf"), -1.0):
        assert lib.pt_resolve_filtered(t._ctx, ptr, 2, bad, 1) == abi.PT_ERR_INVALID, bad
    assert np.all(out == 7.0)               # a refused call writes nothing
    # a fresh estimate: nothing known, every pixel passes through as 0 with no taps; kappa 0 and -0 are valid
    for kappa in (0.0, -0.0):
        assert lib.pt_resolve_filtered(t._ctx, ptr, abi.PT_FILTER_MAX_RADIUS, kappa, 1) == abi.PT_OK
        assert not out.any()
    t.close()
