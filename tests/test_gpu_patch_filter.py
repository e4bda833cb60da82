"""The patch-wise filtered read-out on the device (pt_resolve_filtered_patch: pt_filter_patch_kernel) against the plain numpy
restatement of its statements (tests/patch_filter_ref.py, itself held to its properties by tests/test_patch_filter_ref.py
without a GPU), and at patch 0 against pt_resolve_filtered on the device.

States go in through load_error_state as in tests/test_gpu_filter.py, so most cases need no trace launch; floats are compared
as bit patterns except where both sides are NaN (error_ref.same_floats); no tolerance and no clock anywhere."""
import ctypes as C

import numpy as np
import pytest

import error_ref as E
import filter_ref as FR
import patch_filter_ref as PR
from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd.tracer import PathTracer, PtError

pytestmark = pytest.mark.gpu

F = np.float32
KAPPA = abi.PT_FILTER_PATCH_KAPPA_DEFAULT


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


def _check(t, state, radius, patch, kappa, gamma, what, band_rows=0):
    got = t.patch_filtered_image(radius, patch, kappa, gamma=gamma)
    ref = PR.filtered(state, radius, patch, kappa, gamma=gamma, band_rows=band_rows)
    assert E.same_floats(got, ref), "%s, radius %d, patch %d, kappa %g, gamma %d: %s" % (
        what, radius, patch, kappa, gamma, E.first_difference(got, ref))
    return got


def _wide(state, factor=40.0):
    """Standard errors wide enough that a good share of the taps pass and the patch terms decide which."""
    state[..., 1, :3] *= F(factor)
    return state


@pytest.fixture(scope="module")
def hand():
    state, _ = E.hand_state()
    t = _loaded(state)
    yield t, state
    t.close()


@pytest.fixture(scope="module")
def ordinary():
    state = _wide(FR.ordinary_state(E.HAND_W, E.HAND_H, seed=13))
    t = _loaded(state)
    yield t, state
    t.close()


@pytest.mark.parametrize("gamma", [0, 1])
@pytest.mark.parametrize("patch", [0, 1])
def test_hand_made_state_at_every_radius(hand, patch, gamma):
    """131x13: every operand class of n, k and M2 as a centre, as a tap and as a patch term; full and edge tiles of the kernel."""
    t, state = hand
    _, m, cntd = FR.counted(state)
    for radius in range(0, abi.PT_FILTER_MAX_RADIUS + 1):
        got = _check(t, state, radius, patch, KAPPA, gamma, "hand-made state")
        assert np.all(got[..., 3][~cntd] == 0.0) and np.all(got[..., 3][cntd] >= 1.0)
        if radius == 0:
            with np.errstate(all="ignore"):
                assert E.same_floats(got[..., :3], np.sqrt(m) if gamma else m)


@pytest.mark.parametrize("kappa", [0.0, KAPPA, 1e4])
def test_kappa_from_everything_rejected_to_everything_accepted(ordinary, kappa):
    """131x13, radius 4, patch 1.  Kappa 0 accepts identical neighbourhoods only: none here; a huge kappa accepts every tap."""
    t, state = ordinary
    got = _check(t, state, 4, 1, kappa, 0, "ordinary state")
    taps = got[..., 3]
    if kappa == 0.0:
        assert np.all(taps == 1.0)
    elif kappa == 1e4:
        assert taps.max() == 81.0 and taps.min() == 25.0
    else:
        assert 1.0 < taps.mean() < 60.0 and len(np.unique(taps)) > 10
        assert not E.same_floats(got, t.patch_filtered_image(4, 0, kappa, gamma=False))   # the patch terms decided something


def test_kappa_zero_accepts_identical_neighbourhoods():
    st = E.empty_state(9, 45)
    st[..., 0, :3], st[..., 0, 3], st[..., 1, :3], st[..., 1, 3] = 2.0, 8.0, 1.0, 32.0
    t = _loaded(st)
    got = _check(t, st, 2, 1, 0.0, 1, "constant 45x9")
    assert got[..., 3].max() == 25.0 and got[..., 3].min() == 9.0
    t.close()


@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (31, 7), (33, 9), (45, 19), (74, 26)])
def test_shapes_below_a_tile_and_the_halo_and_just_past_them(shape):
    """Below and just above a 32x8 tile and the 5-texel halo; 74x26: several tiles with partial edges."""
    w, h = shape
    state = _wide(FR.ordinary_state(w, h, seed=w * 100 + h))
    if w > 2:
        state[h // 2, w // 2, 0, 3] = 1.0       # a short pixel inside: a dropped tap and dropped terms
        state[0, w - 1, 0, 0] = np.nan          # and a non-finite one in a corner
    t = _loaded(state)
    for radius in (0, 1, 4):
        for patch in (0, 1):
            got = _check(t, state, radius, patch, KAPPA, 1, "%dx%d" % shape)
    assert got[..., 3].max() > 1.0 or w * h == 1
    t.close()


@pytest.mark.parametrize("index", [0, 1])
def test_band_context_filters_inside_its_chunks(index):
    """band_rows 3, band_count 2 on a height of 37: chunks of three image rows dealt in turn, the last chunk (image row 36)
    partial.  Rows at a chunk border lose their patch terms there as well as their taps."""
    height, width = 37, 61
    rows = abi.local_rows(height, 3, index, 2)
    assert rows == (19, 18)[index]
    state = _wide(FR.ordinary_state(width, rows, seed=21 + index))
    t = _loaded(state, band=(3, index, 2), height=height)
    for radius, patch, kappa in ((1, 1, KAPPA), (2, 1, KAPPA), (4, 1, 3.0), (4, 0, KAPPA)):
        got = _check(t, state, radius, patch, kappa, 0, "band %d of 2" % index, band_rows=3)
        free = PR.filtered(state, radius, patch, kappa)
        assert not E.same_floats(got, free)
    got = _check(t, state, 4, 1, 1e4, 0, "band %d of 2" % index, band_rows=3)
    assert got[..., 3].max() == 27.0        # three rows of nine taps: nothing crossed a chunk
    # a row in the middle of a chunk has the band-free image's taps at radius 0 + patch 1 reach ... a border row does not
    got = _check(t, state, 1, 1, KAPPA, 0, "band %d of 2" % index, band_rows=3)
    alone = PR.filtered(state[3:6], 1, 1, KAPPA)
    assert E.same_floats(got[3:6], alone)   # chunk 1 as an image of its own: terms stop at the border too
    t.close()


def test_device_pointer_gives_the_bytes_of_a_host_pointer(ordinary):
    """The device memory is a second context's error state, 32 bytes per pixel: the read-out fills its first half."""
    t, state = ordinary
    host = t.patch_filtered_image(2, 1, KAPPA, gamma=True)
    other = _loaded(np.full_like(state, -1.0))
    ptr, nbytes = C.c_void_p(), C.c_size_t()
    assert other.lib.pt_error_ptr(other._ctx, C.byref(ptr), C.byref(nbytes)) == abi.PT_OK and nbytes.value == 2 * host.nbytes
    assert t.lib.pt_resolve_filtered_patch(t._ctx, ptr, 2, 1, KAPPA, 1) == abi.PT_OK
    buf = other.error_state().reshape(-1)
    assert buf[:host.size].tobytes() == host.tobytes() and np.all(buf[host.size:] == -1.0)
    other.close()


def test_patch_zero_is_pt_resolve_filtered_on_the_device(hand, ordinary):
    for t, state in (hand, ordinary):
        for radius in range(0, abi.PT_FILTER_MAX_RADIUS + 1):
            for kappa, gamma in ((2.0, True), (KAPPA, False)):
                old = t.filtered_image(radius, kappa, gamma=gamma)
                new = t.patch_filtered_image(radius, 0, kappa, gamma=gamma)
                assert E.same_floats(new, old), (radius, kappa, gamma, E.first_difference(new, old))


def _stats_tuple(t):
    st = t.stats()
    values = (getattr(st, name) for name, _ in st._fields_)
    return tuple(tuple(v) if isinstance(v, C.Array) else v for v in values)


def test_rendered_frame_and_the_call_moves_nothing_else_of_the_context():
    """160x88, 8 passes of 4 spp of the default scene through pt_render_passes."""
    t, p = _context(160, 88, reserve=8)
    t.render_passes(8)
    state, accum, stats = t.error_state(), t.accum(), _stats_tuple(t)
    assert np.all(state[..., 0, 3] == 8.0) and np.all(state[..., 1, 3] == 32.0)
    for radius, patch in ((2, 1), (4, 1), (2, 0)):
        for gamma in (0, 1):
            got = _check(t, state, radius, patch, KAPPA, gamma, "rendered 160x88")
    assert got[..., 3].mean() > 4.0
    assert t.error_state().tobytes() == state.tobytes() and t.accum().tobytes() == accum.tobytes()
    assert _stats_tuple(t) == stats
    t.close()


def test_after_two_partial_rounds_of_adaptive_sampling():
    """Pixels of one frame hold different numbers of passes: every term reads its own two pixels' counts."""
    t, p = _context(64, 36, reserve=2)
    st, ad = t.render_adaptive(0.025, 2, 6)
    assert (ad.rounds, ad.partial_rounds) == (3, 2) and st.passes_min < st.passes_max
    state = t.error_state()
    assert len(np.unique(state[..., 0, 3])) >= 2
    for radius in (1, 2, 4):
        _check(t, state, radius, 1, KAPPA, 1, "adaptive 64x36")
    assert t.error_state().tobytes() == state.tobytes()
    t.close()


def test_error_paths():
    t, p = _context(64, 36, estimate=False)
    lib = t.lib
    out = np.full((p.height, p.width, 4), 7.0, np.float32)
    ptr = out.ctypes.data_as(C.c_void_p)
    assert lib.pt_resolve_filtered_patch(t._ctx, ptr, 2, 1, KAPPA, 1) == abi.PT_ERR_NOT_READY
    assert b"pt_resolve_filtered_patch" in (lib.pt_last_error(t._ctx) or b"") and b"estimate is off" in lib.pt_last_error(t._ctx)
    with pytest.raises(PtError):
        t.patch_filtered_image()
    # the argument checks come before the state's, in the header's order
    assert lib.pt_resolve_filtered_patch(t._ctx, ptr, abi.PT_FILTER_MAX_RADIUS + 1, 1, KAPPA, 1) == abi.PT_ERR_INVALID
    assert lib.pt_resolve_filtered_patch(t._ctx, ptr, 2, abi.PT_FILTER_MAX_PATCH + 1, KAPPA, 1) == abi.PT_ERR_INVALID
    assert b"patch" in lib.pt_last_error(t._ctx)
    t.error_estimate(True)
    assert lib.pt_resolve_filtered_patch(t._ctx, None, 2, 1, KAPPA, 1) == abi.PT_ERR_INVALID
    assert lib.pt_resolve_filtered_patch(t._ctx, ptr, abi.PT_FILTER_MAX_RADIUS + 1, 1, KAPPA, 1) == abi.PT_ERR_INVALID
    assert lib.pt_resolve_filtered_patch(t._ctx, ptr, 0xffffffff, 1, KAPPA, 1) == abi.PT_ERR_INVALID
    assert lib.pt_resolve_filtered_patch(t._ctx, ptr, 2, abi.PT_FILTER_MAX_PATCH + 1, KAPPA, 1) == abi.PT_ERR_INVALID
    assert lib.pt_resolve_filtered_patch(t._ctx, ptr, 2, 0xffffffff, KAPPA, 1) == abi.PT_ERR_INVALID
    assert lib.pt_resolve_filtered_patch(t._ctx, ptr, abi.PT_FILTER_MAX_RADIUS + 1, abi.PT_FILTER_MAX_PATCH + 1, KAPPA, 1) == abi.PT_ERR_INVALID
    assert b"radius" in lib.pt_last_error(t._ctx)      # the radius is looked at first
    for bad in (float("nan"), float("inf"), -float("inf"), -1.0):
        assert lib.pt_resolve_filtered_patch(t._ctx, ptr, 2, 1, bad, 1) == abi.PT_ERR_INVALID, bad
    assert np.all(out == 7.0)               # a refused call writes nothing
    # a fresh estimate: nothing known, every pixel passes through as 0 with no taps; kappa 0 and -0 are valid
    for kappa in (0.0, -0.0):
        assert lib.pt_resolve_filtered_patch(t._ctx, ptr, abi.PT_FILTER_MAX_RADIUS, abi.PT_FILTER_MAX_PATCH, kappa, 1) == abi.PT_OK
        assert not out.any()
    t.close()
