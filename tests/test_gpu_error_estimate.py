"""The per-pixel error estimate on the device (PT_OPT_ERROR_ESTIMATE: pt_fold_error_kernel, pt_resolve_error_kernel,
pt_error_tiles_kernel, pt_error_stats, pt_render_until) against the plain numpy restatement of its statements
(tests/error_ref.py, itself held to its properties by tests/test_error_ref.py without a GPU).

The restatement is fed with pass sums obtained independently of the code under test: each pass rendered alone by the plain
path into a fresh context (first_pass = p, estimate off), and the oracle's passes.  Floats are compared as bit patterns
except where both sides are NaN, counts outright; no tolerance and no clock anywhere."""
import ctypes as C

import numpy as np
import pytest

import error_ref as E
import readout_ref as R
from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd.tracer import PathTracer, PtError

pytestmark = pytest.mark.gpu

MAX_PASSES = 5


def _context(spheres, p, reserve=MAX_PASSES, estimate=True, **kw):
    t = PathTracer(p.width, p.height, **kw)
    t.set_spheres(spheres)
    t.set_params(p)
    t.reserve_passes(reserve)
    if estimate:
        t.error_estimate(True)
    return t


def _render(t, p, first, n):
    q = p.copy()
    q.first_pass = p.first_pass + first
    t.set_params(q)
    t.render_passes(n)


def _solo_passes(spheres, p, n):
    """Each pass alone, by the plain path, in a context of its own."""
    out = []
    for k in range(n):
        t = _context(spheres, p, reserve=1, estimate=False)
        _render(t, p, k, 1)
        out.append(t.accum())
        t.close()
    return out


def _zeros(p):
    rows = abi.local_rows(p.height, p.band_rows, p.band_index, p.band_count)
    return E.empty_state(rows, p.width), np.zeros((rows, p.width, 4), np.float32)


def _check_read_outs(t, state, what):
    """pt_resolve_error, pt_error_tiles and pt_error_stats of the context against the restatement on `state`."""
    got = t.error_image()
    ref = E.resolve_error(state)
    assert E.same_floats(got, ref), "%s, pt_resolve_error: %s" % (what, E.first_difference(got, ref))
    got = t.error_tiles()
    ref, _ = E.tiles(state)
    assert E.same_floats(got, ref), "%s, pt_error_tiles: %s" % (what, E.first_difference(got, ref))
    assert E.same_floats(t.error_tiles(), got), "%s: pt_error_tiles differs from run to run" % what
    st = t.error_stats()
    assert E.same_stats(st, E.stats(state)) == "", (what, E.same_stats(st, E.stats(state)))
    assert st.passes_rendered == 0 and st.reached == 0
    return st


CASES = {
    "64x36": dict(w=64, h=36, spp=4),
    "61x37": dict(w=61, h=37, spp=4),
    "3x5": dict(w=3, h=5, spp=4),
    "1x1": dict(w=1, h=1, spp=4),
    "64x36 band 1 of 3": dict(w=64, h=36, spp=4, band=(8, 1, 3)),
    "64x36 2spp": dict(w=64, h=36, spp=2),
}


@pytest.mark.parametrize("name", list(CASES))
def test_raw_state_read_outs_and_accum_against_the_restatement(ora, name):
    """1, 2, 5 passes and 3 + 2 over two calls: the raw state is the restatement's fold of passes rendered one by one elsewhere,
    accum has the bytes of a context without the estimate, and every read-out is the restatement's on that state."""
    c = CASES[name]
    spheres, p = E.estimate_scene(c["w"], c["h"], spp=c["spp"], band=c.get("band"))
    solo = _solo_passes(spheres, p, MAX_PASSES)
    for k, s in enumerate(E.oracle_passes(ora, spheres, p, MAX_PASSES)):
        assert E.same_floats(solo[k], s), "%s: pass %d rendered alone differs from the oracle's: %s" % (name, k, E.first_difference(solo[k], s))
    on, off = _context(spheres, p), _context(spheres, p, estimate=False)
    st0, acc0 = _zeros(p)
    assert on.error_state().shape == st0.shape and not on.error_state().any()
    for calls in ((1,), (2,), (5,), (3, 2)):
        what = "%s, passes %s" % (name, "+".join(str(n) for n in calls))
        on.reset()
        off.reset()
        first = 0
        for n in calls:
            _render(on, p, first, n)
            _render(off, p, first, n)
            first += n
        ref_state, ref_acc = E.fold(st0, acc0, solo[:first])
        got = on.error_state()
        assert E.same_floats(got, ref_state), "%s, raw state: %s" % (what, E.first_difference(got, ref_state))
        assert np.all(got[..., 0, 3] == first) and np.all(got[..., 1, 3] == first * c["spp"])
        acc_on, acc_off = on.accum(), off.accum()
        assert acc_on.tobytes() == acc_off.tobytes(), "%s: accum differs with the estimate on" % what
        assert E.same_floats(acc_on, ref_acc), what
        st = _check_read_outs(on, ref_state, what)
        assert st.pixels == st0.shape[0] * st0.shape[1]
        assert (st.pixels_short == st.pixels) if first < 2 else (st.pixels_counted == st.pixels and st.passes_min == st.passes_max == first)
    on.close()
    off.close()


def test_a_captured_launch_replayed_three_times_is_three_direct_calls():
    """n and k live in the buffer: three replays of a captured pt_render_passes(2) leave the raw state and accum of three direct
    calls, n = 6."""
    import torch

    spheres, p = E.estimate_scene(spp=4)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = _context(spheres, p, reserve=2, use_torch=True)   # binds the side stream as its launch stream
        t.render_passes(2)                                    # warm-up outside the capture
        torch.cuda.current_stream().synchronize()
        t.reset()
        assert not t.error_state().any()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            t.render_passes(2)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    d = _context(spheres, p, reserve=2)
    for _ in range(3):
        d.render_passes(2)
    got, ref = t.error_state(), d.error_state()
    assert E.same_floats(got, ref), E.first_difference(got, ref)
    assert np.all(got[..., 0, 3] == 6.0) and np.all(got[..., 1, 3] == 24.0)
    assert t.accum_tensor.cpu().numpy().tobytes() == d.accum().tobytes()
    solo = _solo_passes(spheres, p, 2)
    ref_state, _ = E.fold(*_zeros(p), solo * 3)
    assert E.same_floats(got, ref_state), E.first_difference(got, ref_state)
    _check_read_outs(t, ref_state, "after three replays")
    t.close()
    d.close()


def test_read_outs_on_hand_made_states():
    """States written through pt_error_ptr: n in {0, 1, 2, 3, 2^24}, k in {0, -0, subnormal, inf, NaN}, M2 in {0, tiny, huge, inf,
    NaN, negative}, each class filling a full tile and an edge tile."""
    state, classes = E.hand_state()
    counts = E.hand_classes(state)
    for name, n in counts.items():
        assert n >= 8 * E.HAND_H, (name, n)   # every class is there, a column of tiles wide
    spheres, p = E.estimate_scene(E.HAND_W, E.HAND_H)
    t = _context(spheres, p)
    t.load_error_state(state)
    assert E.same_floats(t.error_state(), state), "the written state is not handed back as it was"
    st = _check_read_outs(t, state, "hand-made state")
    assert st.pixels_short == 2 * 8 * E.HAND_H and st.pixels_nonfinite == 7 * 8 * E.HAND_H
    assert st.pixels_counted + st.pixels_short + st.pixels_nonfinite == st.pixels
    rec = t.error_tiles()
    assert rec[0, :, 2].tolist() == [float(x) for x in [0, 0, 64, 64, 64] + [0, 0, 0, 64, 0] + [64, 64, 64, 0, 0, 0] + [24]]
    assert rec[1, -1, 2] == 15.0
    # a second, shuffled state: classes meet inside a tile
    rng = np.random.default_rng(9)
    flat = state.reshape(-1, 2, 4).copy()
    flat[:, 0, 3] = rng.permutation(flat[:, 0, 3])
    flat[:, 1, 3] = rng.permutation(flat[:, 1, 3])
    shuffled = flat.reshape(state.shape)
    t.load_error_state(shuffled)
    _check_read_outs(t, shuffled, "shuffled hand-made state")
    t.close()


def test_black_background_and_non_finite_radiance(ora):
    """A black background: pixels whose passes are all the same have M2 == 0 exactly.  readout_ref.extreme_scene: emissions of
    inf and NaN reach the state; such pixels are counted in pixels_nonfinite and every other sum stays finite."""
    spheres, p = E.estimate_scene(spp=2, black=True)
    t = _context(spheres, p)
    t.render_passes(4)
    ref_state, _ = E.fold(*_zeros(p), E.oracle_passes(ora, spheres, p, 4))
    got = t.error_state()
    assert E.same_floats(got, ref_state), E.first_difference(got, ref_state)
    assert int((got[..., 1, :3] == 0.0).all(axis=-1).sum()) >= 64, "no pixel with M2 == 0"
    _check_read_outs(t, ref_state, "black background")
    t.close()
    spheres, p = R.extreme_scene(2)
    t = _context(spheres, p)
    t.render_passes(4)
    ref_state, _ = E.fold(*_zeros(p), E.oracle_passes(ora, spheres, p, 4))
    got = t.error_state()
    assert E.same_floats(got, ref_state), E.first_difference(got, ref_state)
    st = _check_read_outs(t, ref_state, "extreme radiance")
    assert st.pixels_nonfinite >= 64 and st.pixels_counted >= 64 and st.pixels_short == 0
    assert int(np.isnan(got[..., 0, :3]).any(axis=-1).sum()) >= 16 and int((got[..., 1, :3] == 0.0).all(axis=-1).sum()) >= 64
    assert np.isfinite([st.sum_e2, st.sum_m2, st.rel_error, st.rms_error]).all()
    t.close()


def test_render_until_stops_where_the_restatement_says(ora):
    spheres, p = E.estimate_scene(spp=4)
    cap = 32
    passes = E.oracle_passes(ora, spheres, p, cap)
    want, reached, ref_state, ref_acc = E.predicted_stop(passes, 4, 0.03, cap)
    assert reached and 8 <= want < cap, (want, reached)
    t = _context(spheres, p, reserve=4)
    st = t.render_until(0.03, 4, cap)
    assert (st.passes_rendered, st.reached) == (want, 1)
    assert E.same_stats(st, E.stats(ref_state)) == "", E.same_stats(st, E.stats(ref_state))
    assert st.rel_error <= float(np.float32(0.03)) and st.pixels_short == 0
    assert E.same_floats(t.error_state(), ref_state)
    one = _context(spheres, p, reserve=want, estimate=False)
    one.render_passes(want)
    assert t.accum().tobytes() == one.accum().tobytes(), "not the frame of one pt_render_passes of %d passes" % want
    assert E.same_floats(one.accum(), ref_acc)
    one.close()
    # max_passes spent before an unreachable target: reached == 0, still PT_OK; a second call continues the same frame
    t.reset()
    t.set_params(p)
    st = t.render_until(1e-6, 4, 4)
    assert (st.passes_rendered, st.reached) == (4, 0)
    st = t.render_until(0.03, 4, cap - 4)
    assert (st.passes_rendered, st.reached) == (want - 4, 1)
    assert E.same_floats(t.error_state(), ref_state) and E.same_floats(t.accum(), ref_acc)
    assert t.params.first_pass == want
    # a launch shorter than passes_per_launch at the end: 4 + 2 of max 6
    t.reset()
    t.set_params(p)
    st = t.render_until(1e-6, 4, 6)
    assert (st.passes_rendered, st.reached) == (6, 0)
    assert E.same_floats(t.error_state(), E.fold(*_zeros(p), passes[:6])[0])
    t.close()


def _rc(t, fn, *args):
    return fn(t._ctx, *args), t.lib.pt_last_error(t._ctx) or b""


def test_error_paths():
    spheres, p = E.estimate_scene(spp=4)
    t = _context(spheres, p, estimate=False)
    lib = t.lib
    ptr, nbytes, st = C.c_void_p(), C.c_size_t(), abi.PtErrorStats()
    tx, ty = C.c_uint32(), C.c_uint32()
    out = np.zeros((p.height, p.width, 4), np.float32)
    assert lib.pt_error_ptr(t._ctx, C.byref(ptr), C.byref(nbytes)) == abi.PT_ERR_NOT_READY
    assert lib.pt_resolve_error(t._ctx, out.ctypes.data_as(C.c_void_p)) == abi.PT_ERR_NOT_READY
    assert lib.pt_error_tiles(t._ctx, None, C.byref(tx), C.byref(ty)) == abi.PT_ERR_NOT_READY
    assert lib.pt_error_stats(t._ctx, C.byref(st)) == abi.PT_ERR_NOT_READY
    rc, msg = _rc(t, lib.pt_render_until, 0.1, 1, 4, C.byref(st))
    assert rc == abi.PT_ERR_INVALID and b"estimate is off" in msg
    t.error_estimate(True)
    assert lib.pt_error_ptr(t._ctx, C.byref(ptr), C.byref(nbytes)) == abi.PT_OK and nbytes.value == p.width * p.height * 32
    assert lib.pt_error_tiles(t._ctx, None, C.byref(tx), C.byref(ty)) == abi.PT_OK and (tx.value, ty.value) == (8, 5)
    assert lib.pt_render_until(t._ctx, 0.1, MAX_PASSES + 1, 64, C.byref(st)) == abi.PT_ERR_CAPACITY
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.pt_render_until(t._ctx, bad, 1, 4, C.byref(st)) == abi.PT_ERR_INVALID, bad
    assert lib.pt_render_until(t._ctx, 0.1, 0, 4, C.byref(st)) == abi.PT_ERR_INVALID
    assert lib.pt_set_option(t._ctx, abi.PT_OPT_ERROR_ESTIMATE, 2) == abi.PT_ERR_INVALID
    assert not t.accum().any()   # nothing above rendered anything
    # another samples_per_pixel in the middle of an estimate
    t.render_passes(2)
    q = p.copy()
    q.samples_per_pixel = 2
    t.set_params(q)
    rc, msg = _rc(t, lib.pt_render_passes, 1)
    assert rc == abi.PT_ERR_INVALID and b"clear first" in msg
    assert np.all(t.error_state()[..., 0, 3] == 2.0) and np.all(t.accum()[..., 3] == 8.0)   # a refused call changes nothing
    t.reset()
    t.render_passes(1)   # after a clear the new count is taken
    assert np.all(t.error_state()[..., 1, 3] == 2.0)
    # off releases the state, on again starts from zero
    t.error_estimate(False)
    assert lib.pt_error_ptr(t._ctx, C.byref(ptr), C.byref(nbytes)) == abi.PT_ERR_NOT_READY
    t.error_estimate(True)
    assert not t.error_state().any()
    t.close()


def test_the_estimate_is_cleared_wherever_the_accumulation_is_cleared_or_replaced():
    spheres, p = E.estimate_scene(spp=4)
    t = _context(spheres, p)
    other = _context(spheres, p, estimate=False)

    def filled():
        t.set_params(p)
        t.render_passes(2)
        assert np.all(t.error_state()[..., 0, 3] == 2.0)

    def cleared(what, spp=3):
        assert not t.error_state().view(np.uint32).any(), "%s left the estimate in place" % what
        q = p.copy()
        q.samples_per_pixel = spp   # ... and the next fold may bring another sample count
        t.set_params(q)
        t.render_passes(1)
        assert np.all(t.error_state()[..., 1, 3] == float(spp)), what
        t.reset()

    filled()
    t.reset()
    cleared("pt_reset_accum")
    filled()
    t.tune(2)
    assert t.stats().render_launches == 0   # (it launched, and cleared the statistics with the rest)
    cleared("pt_tune")
    filled()
    checkpoint = t.accum()
    t.load_accum(checkpoint)
    assert t.accum().tobytes() == checkpoint.tobytes()
    cleared("pt_load_accum")
    filled()
    ptr, nbytes = C.c_void_p(), C.c_size_t()
    assert other.lib.pt_accum_ptr(other._ctx, C.byref(ptr), C.byref(nbytes)) == abi.PT_OK
    t._check(t.lib.pt_bind_accum(t._ctx, ptr, nbytes.value))
    cleared("pt_bind_accum")
    filled()
    t._check(t.lib.pt_bind_accum(t._ctx, None, 0))
    cleared("pt_bind_accum(NULL)")
    filled()
    q = p.copy()
    q.band_rows, q.band_index, q.band_count = 8, 1, 3
    t.set_params(q)
    assert t.error_state().shape[0] == abi.local_rows(p.height, 8, 1, 3) and not t.error_state().view(np.uint32).any()
    t.set_params(p)
    assert t.error_state().shape[0] == p.height
    cleared("pt_set_params with another row partition")
    filled()
    t._check(t.lib.pt_resize(t._ctx, 80, 48))
    t.width, t.height, t.local_rows = 80, 48, 48
    assert t.error_state().shape == (48, 80, 2, 4) and not t.error_state().view(np.uint32).any()
    sp2, p2 = E.estimate_scene(80, 48, spp=2)
    t.set_params(p2)
    t.render_passes(2)
    ref, _ = E.fold(*_zeros(p2), _solo_passes(sp2, p2, 2))
    assert E.same_floats(t.error_state(), ref)
    t.close()
    other.close()
