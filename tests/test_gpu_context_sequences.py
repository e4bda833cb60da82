"""ONE long-lived context driven through chains of state changes, compared with the model of tests/context_model.py after every
step that says `check`, and with a FRESH context given only the final configuration at the end of every sequence.

Almost every other test builds a context, configures it once, renders and compares; a value left over from the configuration
before — a tile order or cost table sized for the old partition, a cached frame graph whose plan compares equal but should not,
a first_pass advanced by one entry point and not seen by another, an estimate or a buffer not cleared — shows only when calls
CROSS.  The sequences are constructed so that every ordered pair of configuration calls is followed by work and a check, and
every configuration call stands directly before and after pt_render_frames, pt_render_adaptive, pt_tune and a captured and
replayed pt_render_passes (tests/test_context_model.py counts that).  One test per leading operation: a failure names its
crossing, the assertion message the step.

After every check: accum() bit for bit, PtStats.segments and total_spp, canvas and both textures byte for byte, the estimate's
state bit for bit while it is on, the build of the last trace launch under roulette and overlay, PtStats.geometry_path under a
forced path.  At the end: both contexts cleared, the last work repeated on both, everything above again for both, and the
structure fields of PtStats equal (where neither pt_tune nor pt_refit_grid has refitted the grid since the scene was set; the
grid's build only under a forced path: PT_GEOM_AUTO settles lazily and the build follows whether the grid is in use).
Frames of 40 x 24, 33 x 19 and 64 x 36, at most 3 spp and 3 passes per call.  Tolerance: none.

FOUND BY THE CROSSING bind_accum -> set_band / resize -> bind_accum(NULL) (and, plainly, render -> bind_accum(NULL)):
pt_bind_accum(ctx, NULL) restarted the sample count and cleared the estimate but handed back the own buffer with whatever it
held when the caller's buffer took its place — an image of another frame, after a repartition of another set of rows, that
PtStats.total_spp and every read-out then took for the current one.  The own buffer now comes back cleared.
"""
import ctypes as C
import time

import numpy as np
import pytest

import context_model as M
import error_ref as E
from ray_tracer_webgl_amd import abi

pytestmark = pytest.mark.gpu

LAUNCHING = ("render", "render_passes", "render_until", "render_adaptive", "render_frame", "render_frames", "captured_passes")
_paths = {}


def expected_path(policy, scene, steered):
    """PtStats.geometry_path of a fresh context with that forced path on that scene (steered: roulette or overlay on)"""
    key = (policy, scene, steered)
    if key not in _paths:
        d = M.Driver(M.SIZES[0])
        try:
            d.t.set_geometry_path(policy)
            d.t.set_spheres(M.scene(scene))
            if steered:
                d.t.set_russian_roulette(1)
            d.t.set_params(M.base_params(*M.SIZES[0]))
            d.t.render()
            _paths[key] = int(d.t.stats().geometry_path)
        finally:
            d.close()
    return _paths[key]


def compare(d, m, where, launched):
    t = d.t
    got = t.accum()
    assert got.shape == m.accum.shape, (where, got.shape, m.accum.shape)
    assert E.same_floats(got, m.accum), "%s: accum: %s" % (where, E.first_difference(got, m.accum))
    st = t.stats()
    assert (st.segments, st.total_spp, st.local_rows) == (m.segments, m.total_spp, m.rows), (where, st.segments, m.segments, st.total_spp, m.total_spp)
    assert np.array_equal(t.read_canvas(), m.canvas), "%s: canvas" % where
    for k in range(2):
        assert np.array_equal(t.read_texture(k), m.tex[k]), "%s: texture %d" % (where, k)
    if m.err_on:
        est = t.error_state()
        assert E.same_floats(est, m.err), "%s: estimate: %s" % (where, E.first_difference(est, m.err))
    else:
        ptr = C.c_void_p()
        assert t.lib.pt_error_ptr(t._ctx, C.byref(ptr), None) == abi.PT_ERR_NOT_READY, where
    if launched:
        want = abi.BUILD_DEBUG_OVERLAY if m.overlay is not None else (abi.BUILD_ROULETTE if m.roulette else None)
        if want is not None:
            assert t.last_trace_build() == want, where
        if m.policy != abi.PT_GEOM_AUTO:
            assert st.geometry_path == expected_path(m.policy, m.scene, bool(m.roulette or m.overlay is not None)), where
    return got, st


def step(d, m, s):
    """one step on context and model: (model's return code, context's)"""
    name, v = s
    op = M.OPS[name]
    args = op.plan(m, v)
    if name == "tune":
        rc_ctx, cleared = op.ctx(d, args)
        rc_model = M._m_tune(m, args, cleared)
    else:
        rc_model = op.model(m, args)
        rc_ctx = op.ctx(d, args)
    return rc_model, rc_ctx


def fresh_for(m):
    """a new context given only the configuration the model holds"""
    d = M.Driver((m.w, m.h))
    t = d.t
    t.set_geometry_path(m.policy)
    t.set_carry_lanes(m.carry)
    t.set_refill_min(m.refill)
    t.set_count_work(m.count_work)
    t.set_grid_fit(bool(m.grid_fit))
    t.set_spheres(M.scene(m.scene))
    t.set_russian_roulette(m.roulette)
    if m.overlay is not None:
        t.set_debug_overlay(True, *m.overlay)
    t.set_params(m.params)
    t.reserve_passes(m.reserved)
    t.error_estimate(m.err_on)
    return d


def described(st, m):
    fields = [f for f in M.STAT_FIELDS if f != "grid_kernel_build" or m.policy != abi.PT_GEOM_AUTO]
    return tuple(tuple(int(v) for v in getattr(st, f)) if f == "grid_cells" else int(getattr(st, f)) for f in fields)


def run_sequence(name, k, ora):
    seq = M.SEQUENCES[name][k]
    refused = M.REFUSED if name == "refusals" else [None] * len(seq)
    m = M.start(M.OracleRenderer())
    d = M.Driver(M.SIZES[0])
    fresh = None
    try:
        launched = False
        for i, s in enumerate(seq):
            where = "%s[%d] step %d %s after %s" % (name, k, i, s, seq[max(0, i - 4):i])
            if s == M.CHECK:
                got, _ = compare(d, m, where, launched)
                if not m.uneven:
                    m.checkpoint = got   # (the context's own: a later load_accum gives it back)
                continue
            seg = m.segments
            rc_model, rc_ctx = step(d, m, s)
            assert rc_ctx == rc_model, "%s: returned %d, the model says %d (%s)" % (where, rc_ctx, rc_model, d.lib.pt_last_error(d.ctx))
            assert rc_model == (M.OK if refused[i] is None else refused[i]), where
            if rc_model == M.OK and M.OPS[s[0]].group != M.WORK:
                launched = False   # (a configuration call: the last launch no longer speaks for it)
            if rc_model == M.OK and s[0] in LAUNCHING and m.segments > seg:   # (render_adaptive may find nothing left to do)
                launched = True
        # a fresh context with the final configuration, both from a cleared state, the last work once more
        last = seq[-2]
        assert M.OPS[last[0]].group == M.WORK
        for s in (("reset", 0), ("clear_textures", 0)):
            assert step(d, m, s) == (M.OK, M.OK)
        fresh = fresh_for(m)
        args = M.OPS[last[0]].plan(m, last[1])
        rc = [M.OPS[last[0]].ctx(x, args) for x in (d, fresh)]
        rc_model = M.OPS[last[0]].model(m, args)
        assert rc == [rc_model, rc_model], (name, k, last, rc, rc_model)
        did = rc_model == M.OK and last[0] in LAUNCHING and m.segments > 0
        _, st_long = compare(d, m, "%s[%d] the long-lived context after a clear and %s" % (name, k, last), did)
        _, st_new = compare(fresh, m, "%s[%d] a fresh context after %s" % (name, k, last), did)
        if not m.tuned:
            assert described(st_long, m) == described(st_new, m), (name, k, described(st_long, m), described(st_new, m))
    finally:
        d.close()
        if fresh is not None:
            fresh.close()


@pytest.mark.parametrize("name", list(M.SEQUENCES))
def test_sequences_led_by(ora, name):
    t0 = time.time()
    for k in range(len(M.SEQUENCES[name])):
        run_sequence(name, k, ora)
    print("%s: %.2f s" % (name, time.time() - t0))


def test_unbinding_hands_back_an_empty_accumulation(ora):
    """The crossing that found it: bind_accum -> set_band -> bind_accum(NULL).  The own buffer used to come back holding the
    full-height image it held before the bind, read as the band's rows, with total_spp restarted on the host only."""
    import torch

    m = M.start(M.OracleRenderer())
    d = M.Driver(M.SIZES[0])
    try:
        for s in M.PROLOGUE[:-1] + [("render_passes", 1), M.CHECK, ("bind_accum", 0), ("set_band", 1), ("render", 0), M.CHECK,
                                    ("bind_accum", 1), M.CHECK, ("render", 0), M.CHECK]:
            if s == M.CHECK:
                compare(d, m, str(s), True)
            else:
                assert step(d, m, s) == (M.OK, M.OK), s
        assert d.t.stats().total_spp == m.params.samples_per_pixel
        torch.cuda.synchronize()
    finally:
        d.close()
