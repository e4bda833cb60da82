"""What each change of a context drops, at the ABI: the rows of csrc/pt_ctx_state.hpp's change table and the transitions of its
accumulation tallies, as a caller sees them (tests/test_ctx_state.py pins the table itself on the CPU).

Per row: one fresh 40 x 24 context — a regular scene of 37 spheres (it gets a grid), 1 spp, depth 4, two passes reserved, the
error estimate, the feature planes and reprojection on, two passes folded, the features rendered, the history kept —, the
change, then the probes the other modules use:
  the feature planes speak      pt_read_features answers PT_OK, else PT_ERR_NOT_READY
  the estimate holds its passes a pass at another samples_per_pixel is refused with PT_ERR_INVALID, else accepted
  the history is usable         (after pt_render_features for the uniforms in place) pt_reproject answers PT_OK, else
                                PT_ERR_NOT_READY and says "no history"
  the tallies                   PtStats.total_spp, samples and render_launches
The probes run in that order, the statistics first: the second sets uniforms and may render, the third uses the history up.
The adaptive tables' rows are tests/test_gpu_adaptive.py's; whether pt_tune launches is scheduling
(tests/test_gpu_context_sequences.py).  No tolerance and no clock anywhere."""
import ctypes as C

import numpy as np
import pytest

from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer

pytestmark = pytest.mark.gpu

W, H = 40, 24
PIX = W * H
OK, INVALID, NOT_READY = abi.PT_OK, abi.PT_ERR_INVALID, abi.PT_ERR_NOT_READY
NEAR = ((2.5, 1.5, 3.0), (0.0, 0.2, -0.5))   # look from, look at


def spheres():
    """a ground and 6 x 6 small spheres standing on it"""
    items = [scenes._sphere((0.0, -100.5, -1.0), 100.0, abi.PT_DIFFUSE, (0.5, 0.5, 0.5))]
    for k in range(36):
        kind = (abi.PT_DIFFUSE, abi.PT_METAL, abi.PT_GLASS)[k % 3]
        items.append(scenes._sphere(((k % 6 - 2.5) * 0.6, -0.3, (k // 6 - 2.5) * 0.6 - 1.0), 0.2, kind,
                                    (0.2 + 0.1 * (k % 7), 0.8 - 0.1 * (k % 5), 0.5), 0.1 * (k % 3), 1.5))
    return scenes._pack(items)


def params(w=W, h=H, view=NEAR, spp=1):
    p = scenes._base_params(spp, 4)
    scenes._look_at(scenes._lib(), p, w, h, view[0], view[1], 50.0, 0.0, 3.5)
    p.width, p.height = w, h
    p.time, p.time_step, p.first_pass = 100.0, abi.PT_TIME_STEP_DECORRELATED, 0
    return p


def view_where(t, far):
    """the camera moved along its line of sight — out until the grid in place no longer fits it (pt_grid_fit() == 1), or in until
    it does; host arithmetic on the uniforms, nothing is launched"""
    for s in ((1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0) if far else (1.0, 0.5, 0.25, 0.125)):
        view = (tuple(a + s * (f - a) for f, a in zip(*NEAR)), NEAR[1])
        t.set_params(params(view=view))
        if (t.grid_fit() == 1) == far:
            return view
    raise AssertionError("no camera distance %s the grid's near region" % ("leaves" if far else "lies inside"))


class Ctx:
    """the set-up of the module's docstring, the camera inside the region the grid was built for, or (`far`) outside it"""

    def __init__(self, far=False):
        self.t = PathTracer(W, H)
        try:
            self._set_up(far)
        except BaseException:
            self.t.close()   # (the caller's try / finally begins only once the set-up has succeeded)
            raise

    def _set_up(self, far):
        t = self.t
        t.set_geometry_path(abi.PT_GEOM_GRID)
        t.set_spheres(spheres())
        self.p = params(view=view_where(t, far))
        t.set_params(self.p)
        t.reserve_passes(2)
        t.error_estimate(True)
        t.feature_planes(True)
        t.reproject_option(True)
        st = t.stats()
        assert st.n_spheres == 37 and st.grid_entries > 0 and min(st.grid_cells) >= 1, "the scene has no grid"
        t.render_passes(2)
        t.render_features()
        t.keep_history()

    def msg(self):
        return self.t.lib.pt_last_error(self.t._ctx) or b""

    def probe(self, p=None):
        """(features speak, estimate holds its passes, history usable, total_spp, samples, launches); `p`: the uniforms the
        context should have by now (after a resize there are none until the probe's own pt_set_params)"""
        t, lib = self.t, self.t.lib
        st = t.stats()
        buf = np.empty(t.local_rows * t.width * 4, np.float32)
        rc = lib.pt_read_features(t._ctx, abi.PT_FEAT_ALBEDO, buf.ctypes.data_as(C.c_void_p))
        assert rc in (OK, NOT_READY), (rc, self.msg())
        feat = rc == OK
        q = (p or self.p).copy()
        q.samples_per_pixel = 2
        t.set_params(q)
        rc = lib.pt_render_passes(t._ctx, 1)
        assert rc in (OK, INVALID), (rc, self.msg())
        assert rc == OK or b"clear first" in self.msg()
        est = rc == INVALID
        t.render_features()   # (the uuid arrays are in place, or this refuses)
        opt = abi.PtReprojectOptions()
        rc = lib.pt_reproject(t._ctx, C.byref(opt))
        assert rc in (OK, NOT_READY), (rc, self.msg())
        assert rc == OK or b"no history" in self.msg()
        return feat, est, rc == OK, st.total_spp, st.samples, st.render_launches

    def close(self):
        self.t.close()


KEPT = (True, True, True, 2, 2 * PIX, 1)   # what the set-up leaves: everything speaks, two passes of one sample in one launch


def band(c):
    q = c.p.copy()
    q.band_rows, q.band_index, q.band_count = 4, 1, 3   # rows 4-7 and 16-19
    c.t.set_params(q)
    c.p = q


def same_rows(c):
    q = c.p.copy()
    q.time = 117.0
    q.band_rows, q.band_index, q.band_count = 5, 3, 0   # "every row" in other words: no repartition
    c.t.set_params(q)
    c.p = q


def resize(c):
    t = c.t
    assert t.lib.pt_resize(t._ctx, 33, 19) == OK   # partial tiles on both edges
    t.width, t.height, t.local_rows = 33, 19, 19
    assert t.lib.pt_render_passes(t._ctx, 1) == NOT_READY and t.lib.pt_render_features(t._ctx) == NOT_READY   # no uniforms
    c.p = params(33, 19)


def leave_the_grid(c):
    near0 = c.t.stats().grid_near_factor
    assert c.t.grid_fit() != 1
    c.t.refit_grid(True)   # only if the class in place is too small for the camera: it is not
    assert c.t.stats().grid_near_factor == near0


def refused_calls(c):
    t, lib = c.t, c.t.lib
    q = c.p.copy()
    q.width = W + 1
    assert lib.pt_set_params(t._ctx, C.byref(q)) == INVALID and b"pt_resize" in c.msg()
    a = np.zeros((H, W, 4), np.float32)
    assert lib.pt_load_accum(t._ctx, a.ctypes.data_as(C.c_void_p), a.nbytes - 16) == INVALID and b"row partition holds" in c.msg()
    opt = abi.PtReprojectOptions(cap_diffuse=0.5)
    assert lib.pt_reproject(t._ctx, C.byref(opt)) == INVALID and b"not a whole number" in c.msg()
    opt = abi.PtReprojectOptions(tolerance_px=-1.0)
    assert lib.pt_reproject_estimate(t._ctx, C.byref(opt)) == INVALID


#            change                                   features estimate history total_spp samples launches
ROWS = {
    "nothing": (lambda c: None, KEPT),
    "refused calls": (refused_calls, KEPT),
    "pt_set_spheres": (lambda c: c.t.set_spheres(spheres()), (False, True, False, 2, 2 * PIX, 1)),
    "pt_set_params, same rows": (same_rows, (False, True, True, 2, 2 * PIX, 1)),
    "pt_set_params, other rows": (band, (False, False, False, 0, 2 * PIX, 1)),   # samples and launches go on counting
    "pt_resize": (resize, (False, False, False, 0, 0, 0)),
    "pt_reset_accum": (lambda c: c.t.reset(), (True, False, True, 0, 0, 0)),
    "pt_refit_grid, nothing to rebuild": (leave_the_grid, KEPT),
    "pt_keep_history again": (lambda c: c.t.keep_history(), KEPT),
}


@pytest.mark.parametrize("name", list(ROWS))
def test_what_a_change_drops(name):
    change, want = ROWS[name]
    c = Ctx()
    try:
        change(c)
        assert c.probe() == want, name
    finally:
        c.close()


def test_a_refit_that_rebuilds_the_grid_drops_the_planes_alone():
    c = Ctx(far=True)
    try:
        t = c.t
        near0 = t.stats().grid_near_factor
        assert t.grid_fit() == 1
        t.refit_grid(False)
        st = t.stats()
        assert st.grid_near_factor != near0 and t.grid_fit() == 0, "the refit rebuilt the grid"
        assert c.probe() == (False, True, True, 2, 2 * PIX, 1)
        assert t.stats().grid_near_factor == st.grid_near_factor
    finally:
        c.close()


@pytest.mark.parametrize("carry", [False, True])
def test_a_reprojection_uses_the_history_up(carry):
    """pt_reproject clears the estimate, pt_reproject_estimate carries it; neither touches the planes or the host's tallies, and
    PtStats.total_spp is what the device holds at pixel 0 afterwards"""
    c = Ctx()
    try:
        t = c.t
        (t.reproject_estimate if carry else t.reproject)()
        want_spp = int(t.accum()[0, 0, 3])
        assert c.probe() == (True, carry, False, want_spp, 2 * PIX, 1)
        assert t.reproject_stats().pixels == PIX
    finally:
        c.close()


def test_binding_and_unbinding_an_accumulation_restart_the_count_and_nothing_else():
    c = Ctx()
    other = PathTracer(W, H)   # the caller's buffer: a second context's accumulation, five samples in every pixel
    try:
        t = c.t
        mine = np.zeros((H, W, 4), np.float32)
        mine[..., 3] = 5.0
        other.load_accum(mine)
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        assert other.lib.pt_accum_ptr(other._ctx, C.byref(ptr), C.byref(nbytes)) == OK and nbytes.value == mine.nbytes
        assert t.lib.pt_bind_accum(t._ctx, ptr, nbytes.value) == OK
        st = t.stats()
        assert (st.total_spp, st.samples, st.render_launches) == (5, 2 * PIX, 1)   # what the bound buffer holds
        assert t.lib.pt_bind_accum(t._ctx, None, 0) == OK
        assert not t.accum().any()   # the own buffer comes back empty
        assert c.probe() == (True, False, True, 0, 2 * PIX, 1)
    finally:
        c.close()
        other.close()


@pytest.mark.parametrize("w", [7, 0, 2 ** 24 - 1])
def test_a_loaded_checkpoint_sets_the_tallies(w):
    c = Ctx()
    try:
        a = c.t.accum()
        a[..., 3] = np.float32(w)
        c.t.load_accum(a)
        assert c.probe() == (True, False, True, w, w * PIX, 1)
    finally:
        c.close()
