"""Adaptive sampling on the device (pt_render_adaptive, pt_adaptive_tiles: the partial round's tile table, trace launch and
masked fold) against the plain restatement of its loop and rule (tests/adaptive_ref.py on top of tests/error_ref.py, held to
their properties by tests/test_adaptive_ref.py without a GPU).

The method is tests/test_gpu_error_estimate.py's: the restatement is fed with pass sums obtained independently of the code
under test — each pass of the uninterrupted frame rendered alone by the plain path in a context of its own (first_pass = p,
estimate off), checked against the oracle's where the oracle is fast enough.  Floats are compared as bit patterns, counts
outright; no tolerance and no clock anywhere.

WHICH DEALING MODE A CASE RUNS.  There is no read-out of the launch plan; from csrc/pt_launch_plan.hpp: a launch of
`items = tiles x 64 x k` work items on 256-thread workgroups asks for ceil(items / 256) of them, far fewer than are resident at
these sizes, so it gets that many and a lane per item (a partial launch of an odd tile count: up to 1.3 lanes).  With
lanes = items, `items x spp < 448 x lanes` deals the launch out (statically, or grouped from `items x spp >= 16 x lanes` on) and
anything above goes through the shared head: 4 spp is dealt statically, 32 spp grouped, 512 spp through the shared queue.  A
partial launch of m tiles and k = 2 has items / lanes = m / (2 ceil(m / 2)): 1 for an even m, (2j + 1) / (2j + 2) for m = 2j + 1,
and 512 x items >= 448 x lanes needs that ratio to be at least 0.875 — so at 512 spp a partial launch of 1, 3 or 5 tiles falls
back to the grouped deal, and one of an even count or of 7 tiles and more goes through the shared head.  Scheduling never
changes a result: every case holds the same bits."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref as A
import error_ref as E
from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer, PtError

pytestmark = pytest.mark.gpu

TARGET, PER_ROUND, CAP = 0.025, 2, 40


def _context(spheres, p, reserve=PER_ROUND, estimate=True, path=None):
    t = PathTracer(p.width, p.height)
    t.set_spheres(spheres)
    t.set_params(p)
    t.reserve_passes(reserve)
    if path is not None:
        t.set_geometry_path(path)
    if estimate:
        t.error_estimate(True)
    return t


class _Solo:
    """The passes of one uninterrupted frame, each rendered alone by the plain path in a context of its own when first asked
    for, and compared with the oracle's (ora is None: too slow for this case)."""

    def __init__(self, spheres, p, ora):
        self.spheres, self.p, self.ora, self.got = spheres, p, ora, {}

    def _one(self, k):
        if k not in self.got:
            q = self.p.copy()
            q.first_pass = self.p.first_pass + k
            t = _context(self.spheres, q, reserve=1, estimate=False)
            t.render_passes(1)
            self.got[k] = t.accum()
            t.close()
            if self.ora is not None:
                ref = self.ora.render(self.spheres, q, 1)[0]
                assert E.same_floats(self.got[k], ref), "pass %d rendered alone differs from the oracle's: %s" % (
                    k, E.first_difference(self.got[k], ref))
        return self.got[k]

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._one(k) for k in range(i.start or 0, i.stop)]
        return self._one(i)


def _cover(w, h, spp):
    """The cover scene (484 spheres: a regular scene, it gets a hierarchy and a grid), depth 6, independent passes."""
    sc = scenes.config2(w, h, spp, 1, 6)
    p = sc.params.copy()
    p.time, p.time_step, p.first_pass = E.T0, abi.PT_TIME_STEP_DECORRELATED, 0
    return sc.spheres, p


_frames = {}


def _frame(ora, key, make, oracle=True):
    """(spheres, params, solo passes) of a case, shared by the tests that use it and left unchanged."""
    if key not in _frames:
        spheres, p = make()
        _frames[key] = (spheres, p, _Solo(spheres, p, ora if oracle else None))
    return _frames[key]


def _default(ora, w=64, h=36, spp=4, band=None, oracle=True):
    return _frame(ora, ("default", w, h, spp, band), lambda: E.estimate_scene(w, h, spp=spp, band=band), oracle)


def _check(t, st, ad, ref, what, last_partial=None, spp=4):
    """Everything a call leaves behind against adaptive_ref.predicted()'s `ref`, bit for bit.  last_partial: the flags of the
    most recent partial round on this context (None: there has been none, and pt_adaptive_tiles says so)."""
    got = t.error_state()
    assert E.same_floats(got, ref["state"]), "%s, raw state: %s" % (what, E.first_difference(got, ref["state"]))
    acc = t.accum()
    assert acc.tobytes() == ref["accum"].tobytes(), "%s, accum: %s" % (what, E.first_difference(acc, ref["accum"]))
    got, want = t.error_image(), E.resolve_error(ref["state"])
    assert E.same_floats(got, want), "%s, pt_resolve_error: %s" % (what, E.first_difference(got, want))
    got, want = t.error_tiles(), E.tiles(ref["state"])[0]
    assert E.same_floats(got, want), "%s, pt_error_tiles: %s" % (what, E.first_difference(got, want))
    if st is not None:
        assert E.same_stats(st, ref["stats"]) == "", (what, E.same_stats(st, ref["stats"]))
        assert (st.passes_rendered, st.reached) == (ref["stats"]["passes_rendered"], ref["stats"]["reached"]), what
        assert A.same_adaptive(ad, ref["adaptive"]) == "", (what, A.same_adaptive(ad, ref["adaptive"]))
    assert E.same_stats(t.error_stats(), ref["stats"]) == "", what
    counts = t.sample_counts()
    assert counts.tobytes() == ref["accum"][..., 3].tobytes(), what
    assert counts.tobytes() == (ref["state"][..., 0, 3] * np.float32(spp)).astype(np.float32).tobytes(), what
    assert t.params.first_pass == ref["next"], (what, t.params.first_pass, ref["next"])
    n_tiles = ref["adaptive"]["tiles"]
    if last_partial is None:
        assert t.lib.pt_adaptive_tiles(t._ctx, None, None, None, None) == abi.PT_ERR_NOT_READY, what
    else:
        base, order, n_active = t.adaptive_tiles()
        assert sorted(base.tolist()) == list(range(n_tiles)), "%s: base is not a permutation of the tiles" % what
        assert order.tolist() == A.partition(base, last_partial).tolist(), what
        assert n_active == int(last_partial.sum()) and set(order[:n_active].tolist()) == set(np.flatnonzero(last_partial).tolist())


def _last_partial(*refs):
    """The flags of the most recent partial round of the calls `refs` (in order), None if there was none."""
    flags = [r["active"] for ref in refs for r in ref["rounds"] if r["partial"]]
    return flags[-1] if flags else None


def _run(ora, name, frame, target=TARGET, per_round=PER_ROUND, cap=CAP, path=None, min_partial=3, spp=4):
    spheres, p, solo = frame
    ref = A.predicted(solo, per_round, target, cap)
    assert ref["adaptive"]["partial_rounds"] >= min_partial, (name, ref["adaptive"])
    t = _context(spheres, p, reserve=per_round, path=path)
    st, ad = t.render_adaptive(target, per_round, cap)
    _check(t, st, ad, ref, name, _last_partial(ref), spp=spp)
    return t, st, ad, ref


# ------------------------------------------------------------------------------------------------ the dealing modes
STATIC = {"64x36": dict(w=64, h=36), "61x37": dict(w=61, h=37), "64x36 band 1 of 3": dict(w=64, h=36, band=(8, 1, 3))}


@pytest.mark.parametrize("name", list(STATIC))
def test_static_deal_against_the_restatement(ora, name):
    """4 spp: every launch of these sizes is dealt statically.  61x37 has edge tiles in both directions, the band owns rows
    8-15 and 32-35 (an edge tile row of 4)."""
    c = STATIC[name]
    t, st, ad, ref = _run(ora, name, _default(ora, c["w"], c["h"], band=c.get("band")))
    assert st.reached == 1 and ad.partial_rounds >= 3 and ad.tiles_active <= 3 * ad.tiles // 4
    assert st.passes_min < st.passes_max == st.passes_rendered
    stats = t.stats()
    assert stats.samples == ad.samples and stats.render_launches == ad.rounds
    assert stats.total_spp == int(ref["accum"][0, 0, 3])   # pixel (0, 0)'s count
    t.close()


def test_static_deal_with_more_tiles_than_the_partition_kernel_has_threads(ora):
    """264x256: 33 x 32 = 1 056 tiles, so pt_partition_order_kernel's runs are per = ceil(1056 / 1024) = 2 positions long — 528
    of its 1024 threads own a run and 496 own none; every smaller case has one position per thread.  At most 12 passes: six
    rounds, five of them partial."""
    t, st, ad, ref = _run(ora, "264x256", _default(ora, w=264, h=256), cap=12)
    assert ad.tiles == 1056 and (ad.tiles + 1023) // 1024 == 2
    assert (ad.rounds, ad.partial_rounds) == (6, 5) and ad.tiles_active <= 3 * ad.tiles // 4
    assert st.passes_min < st.passes_max == st.passes_rendered == 12
    stats = t.stats()
    assert stats.samples == ad.samples and stats.render_launches == ad.rounds
    t.close()


def test_a_single_tile_equals_render_until(ora):
    """3x5: one tile, a partial round can never happen; state, accum and PtErrorStats have the bytes of pt_render_until."""
    spheres, p, solo = _default(ora, 3, 5)
    ref = A.predicted(solo, PER_ROUND, TARGET, 12)
    assert ref["adaptive"]["partial_rounds"] == 0 and ref["adaptive"]["tiles"] == 1
    t, u = _context(spheres, p), _context(spheres, p)
    st, ad = t.render_adaptive(TARGET, PER_ROUND, 12)
    su = u.render_until(TARGET, PER_ROUND, 12)
    _check(t, st, ad, ref, "3x5")
    assert bytes(st) == bytes(su)
    assert t.error_state().tobytes() == u.error_state().tobytes() and t.accum().tobytes() == u.accum().tobytes()
    assert (ad.rounds, ad.partial_rounds, ad.tiles, ad.tile_passes) == (st.passes_rendered // 2, 0, 1, st.passes_rendered)
    t.close()
    u.close()


def test_grouped_queue_against_the_restatement(ora):
    """61x37 at 32 spp: dealt through the grouped queue (the module's docstring).  Target 0.01: 2.5 times below the 4-spp cases'
    for passes of 8 times the samples, i.e. about as many looks."""
    t, st, ad, ref = _run(ora, "61x37 32 spp", _default(ora, 61, 37, spp=32), target=0.01, cap=16, spp=32)
    t.close()


def test_shared_queue_against_the_restatement(ora):
    """64x36 at 512 spp, 2 passes per round, at most 6 passes: the full launches and the partial launches of an even tile count
    or of at least 7 tiles go through the shared head (the module's docstring); that a partial round of that kind runs is asserted.  The target is chosen by the restatement on the solo passes — half the relative error of the first look —
    so that the rounds after the first are partial; that they are is asserted.  (No oracle pass here: 512 spp.)"""
    frame = _default(ora, 64, 36, spp=512, oracle=False)
    _, p, solo = frame
    first_look, _ = E.fold(E.empty_state(36, 64), np.zeros((36, 64, 4), np.float32), solo[0:2])
    target = float(np.float32(E.stats(first_look)["rel_error"] * 0.5))
    t, st, ad, ref = _run(ora, "64x36 512 spp", frame, target=target, cap=6, min_partial=1, spp=512)
    assert ad.partial_rounds >= 1 and ad.rounds == 3 and st.passes_rendered == 6
    shared = [int(r["active"].sum()) for r in ref["rounds"] if r["partial"] and r["k"] == 2]
    assert any(m % 2 == 0 or m >= 7 for m in shared), shared
    t.close()


# ------------------------------------------------------------------------------------------------ the geometry paths
PATHS = {
    "small list": (lambda ora: _default(ora, 61, 37), abi.PT_GEOM_SMALL, abi.PT_GEOM_SMALL, TARGET),
    "scalar list": (lambda ora: _default(ora, 61, 37), abi.PT_GEOM_SCALAR, abi.PT_GEOM_SCALAR, TARGET),
    "grid walk": (lambda ora: _frame(ora, "cover 61x37", lambda: _cover(61, 37, 4)), abi.PT_GEOM_GRID, abi.PT_GEOM_GRID, 0.04),
    "hierarchy walk": (lambda ora: _frame(ora, "cover 61x37", lambda: _cover(61, 37, 4)), abi.PT_GEOM_BVH, abi.PT_GEOM_BVH, 0.04),
}


@pytest.mark.parametrize("name", list(PATHS))
def test_geometry_paths_against_the_restatement(ora, name):
    """61x37, 4 spp: the default scene forced to the small-list kernel (what PT_GEOM_AUTO starts with on nine spheres) and to
    the scalar list walk; the cover scene (484 spheres, target 0.04) forced to the grid walk and to the hierarchy walk."""
    make, force, expect, target = PATHS[name]
    t, st, ad, ref = _run(ora, name, make(ora), target=target, cap=16, path=force)
    assert t.stats().geometry_path == expect, (name, t.stats().geometry_path)
    t.close()


# ------------------------------------------------------------------------------------------------ calls in sequence
def test_two_calls_of_six_equal_one_call_of_twelve(ora):
    spheres, p, solo = _default(ora, 61, 37)
    one = A.predicted(solo, PER_ROUND, 0.02, 12)
    assert one["stats"]["reached"] == 0 and one["adaptive"]["partial_rounds"] >= 3
    a = A.predicted(solo, PER_ROUND, 0.02, 6)
    b = A.predicted(solo, PER_ROUND, 0.02, 6, state=a["state"], accum=a["accum"], first=a["next"])
    t = _context(spheres, p)
    st, ad = t.render_adaptive(0.02, PER_ROUND, 6)
    _check(t, st, ad, a, "first call of 6", _last_partial(a))
    st, ad2 = t.render_adaptive(0.02, PER_ROUND, 6)
    _check(t, st, ad2, b, "second call of 6", _last_partial(a, b))
    # the second call starts from a look at the state the first left: its rounds are rounds 4 to 6 of the one call
    assert [r["active"].tolist() for r in a["rounds"] + b["rounds"]] == [r["active"].tolist() for r in one["rounds"]]
    assert b["rounds"][0]["first"] == 6 and b["rounds"][0]["partial"]
    u = _context(spheres, p)
    su, au = u.render_adaptive(0.02, PER_ROUND, 12)
    _check(u, su, au, one, "one call of 12", _last_partial(one))
    assert t.error_state().tobytes() == u.error_state().tobytes() and t.accum().tobytes() == u.accum().tobytes()
    assert E.same_stats(st, one["stats"]) == "" and (st.passes_rendered, su.passes_rendered, st.reached, su.reached) == (6, 12, 0, 0)
    for k in ("rounds", "partial_rounds", "tile_passes", "samples"):
        assert getattr(ad, k) + getattr(ad2, k) == getattr(au, k), k
    assert ad2.tiles_active == au.tiles_active
    assert t.adaptive_tiles()[1].tolist() == u.adaptive_tiles()[1].tolist()
    assert t.params.first_pass == u.params.first_pass == 12
    t.close()
    u.close()


def test_mixing_entry_points(ora):
    """An adaptive call, pt_render_passes(2), an adaptive call: the restatement's with an all-active round in the middle (the
    second call starts from a look at the state that round left).  The uniform launch after partial rounds reads the context's
    own cost order (the partition lives in a buffer of its own): the bits compared here do not depend on any tile order, so
    that property is held by test_a_partial_round_leaves_the_cost_order_as_it_found_it below, not by this test."""
    spheres, p, solo = _default(ora, 61, 37)
    a = A.predicted(solo, PER_ROUND, TARGET, 6)
    assert a["adaptive"]["partial_rounds"] >= 1
    mid_state, mid_acc = E.fold(a["state"], a["accum"], solo[6:8])
    b = A.predicted(solo, PER_ROUND, TARGET, 6, state=mid_state, accum=mid_acc, first=8)
    assert b["adaptive"]["partial_rounds"] >= 1
    t = _context(spheres, p)
    st, ad = t.render_adaptive(TARGET, PER_ROUND, 6)
    _check(t, st, ad, a, "first adaptive call", _last_partial(a))
    t.render_passes(2)
    q = t.params.copy()
    q.first_pass += 2
    t.set_params(q)
    assert E.same_floats(t.error_state(), mid_state) and t.accum().tobytes() == mid_acc.tobytes()
    st, ad = t.render_adaptive(TARGET, PER_ROUND, 6)
    _check(t, st, ad, b, "second adaptive call", _last_partial(a, b))
    t.close()


def test_a_partial_round_leaves_the_cost_order_as_it_found_it(ora):
    """The partition is written to a buffer of its own, never over the context's cost order.  Which tiles are active is set by
    hand here, so that it cannot follow the costs (on this scene the noisy tiles are also the expensive ones, and a partition
    of the cost order by the rule's own flags moves nothing): after one uniform launch, which reports costs, a state is loaded
    whose even-numbered tiles are far above any target (M2 = 100) and whose odd-numbered ones have M2 = 0.  The first call's
    round is partial: it brings the cost order up to date and partitions it — `base` is that order, `order` its partition,
    and they differ.  The second call's round is partial again with no cost reported in between (a partial launch reports
    none), so the order kernel does not run and `base` must be the first call's `base` entry for entry.  Had the first
    partition been written over the cost order, the second `base` would be the first `order`."""
    spheres, p, _ = _default(ora, 61, 37)
    t = _context(spheres, p)
    t.render_passes(2)
    even = np.arange(40) % 2 == 0
    state = E.empty_state(37, 61)
    state[..., 0, :3] = 1.0
    state[..., 0, 3] = 2.0
    state[..., 1, 3] = 8.0
    state[A.pixel_mask(even, 37, 61), 1, :3] = 100.0
    t.load_error_state(state)
    assert A.select(state, TARGET).tolist() == even.tolist()
    st, ad = t.render_adaptive(TARGET, PER_ROUND, 2)
    assert (ad.rounds, ad.partial_rounds, ad.tile_passes) == (1, 1, 40)
    base_a, order_a, n_a = t.adaptive_tiles()
    assert sorted(base_a.tolist()) == list(range(40)) and n_a == 20
    assert order_a.tolist() == A.partition(base_a, even).tolist() and order_a.tolist() != base_a.tolist()
    flags = A.select(t.error_state(), TARGET)
    assert flags.any() and not flags.all()
    st, ad = t.render_adaptive(TARGET, PER_ROUND, 2)
    assert (ad.rounds, ad.partial_rounds) == (1, 1)
    base_b, order_b, n_b = t.adaptive_tiles()
    assert base_b.tolist() == base_a.tolist(), "a partial round wrote the context's cost order"
    assert order_b.tolist() == A.partition(base_a, flags).tolist() and n_b == int(flags.sum())
    n = t.error_state()[..., 0, 3]
    assert np.all(n[A.pixel_mask(~even, 37, 61)] == 2.0) and np.all(n[A.pixel_mask(even & flags, 37, 61)] == 6.0)
    t.close()


def _snapshot(t):
    return {"accum": t.accum(), "state": t.error_state(), "canvas": t.read_canvas(), "tex0": t.read_texture(0), "tex1": t.read_texture(1)}


def _load_accum_raw(t, accum):
    """The accumulation as bytes, through its device pointer: pt_load_accum takes whole-pass checkpoints only, and after a partial
    round the pixels' sample counts differ."""
    from ray_tracer_webgl_amd.tracer import _H2D, _memcpy
    ptr, nbytes = C.c_void_p(), C.c_size_t()
    assert t.lib.pt_accum_ptr(t._ctx, C.byref(ptr), C.byref(nbytes)) == abi.PT_OK and nbytes.value == accum.nbytes
    t.synchronize()
    _memcpy(ptr, np.ascontiguousarray(accum).ctypes.data_as(C.c_void_p), accum.nbytes, _H2D)


def test_every_launch_kind_in_one_context(ora):
    """The five kinds of trace launch — uniform, single frame (with its cost-order probe), captured frame groups, partial round,
    a frame below four samples (which takes the probed order back) — one after the other in ONE context, whose tile-order state
    and cached plans each step hands to the next.  After every step the context holds, bit for bit, what a fresh context gives
    that starts from the same accumulation, estimate and textures and runs that step alone (a fresh context writes its canvas
    only in a frame step: elsewhere the one context's canvas must be the one it had).  Segment tallies add up: the probes'
    are taken back out.  After the partial round `base` is a permutation of the tiles and `order` its stable partition."""
    spheres, p, _ = _default(ora, 61, 37)
    even = np.arange(40) % 2 == 0
    loaded = E.empty_state(37, 61)          # the state of test_a_partial_round_leaves_the_cost_order_as_it_found_it
    loaded[..., 0, :3] = 1.0
    loaded[..., 0, 3] = 2.0
    loaded[..., 1, 3] = 8.0
    loaded[A.pixel_mask(even, 37, 61), 1, :3] = 100.0
    assert A.select(loaded, TARGET).tolist() == even.tolist()
    one_spp = p.copy()
    one_spp.samples_per_pixel = 1

    def adaptive(t):
        st, ad = t.render_adaptive(TARGET, PER_ROUND, 2)
        assert (ad.rounds, ad.partial_rounds, ad.tile_passes) == (1, 1, 40)
        base, order, n_active = t.adaptive_tiles()
        assert sorted(base.tolist()) == list(range(40)) and n_active == 20
        assert order.tolist() == A.partition(base, even).tolist()

    def frame_at_one_spp(t):
        back = t.params.copy()
        t.set_params(one_spp)
        t.render_frame(0)
        t.set_params(back)

    steps = [("render_passes(2)", lambda t: t.render_passes(2), False),
             ("a frame, which probes", lambda t: t.render_frame(0), True),
             ("a series of 5 frames", lambda t: t.render_frames(1, 100000, 5), True),
             ("load_error_state", lambda t: t.load_error_state(loaded), False),
             ("an adaptive call with a partial round", adaptive, False),
             ("a frame at 1 spp", frame_at_one_spp, True),
             ("render_passes(2) again", lambda t: t.render_passes(2), False)]
    t = _context(spheres, p)
    segments = 0
    for name, step, draws in steps:
        before, params = _snapshot(t), t.params.copy()
        step(t)
        after = _snapshot(t)
        u = _context(spheres, params)
        _load_accum_raw(u, before["accum"])
        u.load_error_state(before["state"])
        u.write_texture(0, before["tex0"])
        u.write_texture(1, before["tex1"])
        step(u)
        alone = _snapshot(u)
        for k in after:
            want = alone[k] if draws or k != "canvas" else before[k]
            assert after[k].tobytes() == want.tobytes(), "%s: %s differs from a fresh context's" % (name, k)
        assert t.params.first_pass == u.params.first_pass, name
        segments += u.stats().segments
        assert t.stats().segments == segments, name
        u.close()
    n = t.error_state()[..., 0, 3]
    assert np.all(n[A.pixel_mask(even, 37, 61)] == 6.0) and np.all(n[A.pixel_mask(~even, 37, 61)] == 4.0)
    t.close()


def test_nothing_to_skip(ora):
    """A target so loose that it is reached at the first look: one uniform round, the bytes of pt_render_until."""
    spheres, p, solo = _default(ora, 61, 37)
    ref = A.predicted(solo, PER_ROUND, 0.5, CAP)
    assert ref["adaptive"]["rounds"] == 1 and ref["stats"]["reached"] == 1
    t, u = _context(spheres, p), _context(spheres, p)
    st, ad = t.render_adaptive(0.5, PER_ROUND, CAP)
    su = u.render_until(0.5, PER_ROUND, CAP)
    _check(t, st, ad, ref, "loose target")
    assert bytes(st) == bytes(su) and (ad.rounds, ad.partial_rounds) == (1, 0)
    assert t.error_state().tobytes() == u.error_state().tobytes() and t.accum().tobytes() == u.accum().tobytes()
    t.close()
    u.close()


def test_idle_tiles_are_untouched_by_a_partial_round(ora):
    """One uniform round, then the same context again through one uniform and one partial round: the pixels of the tiles behind
    n_active in adaptive_tiles()' table keep their accum and state bytes, the others hold two passes more."""
    spheres, p, solo = _default(ora, 61, 37)
    t = _context(spheres, p)
    t.render_adaptive(TARGET, PER_ROUND, 2)
    before_s, before_a = t.error_state(), t.accum()
    assert t.lib.pt_adaptive_tiles(t._ctx, None, None, None, None) == abi.PT_ERR_NOT_READY
    t.reset()
    t.set_params(p)
    st, ad = t.render_adaptive(TARGET, PER_ROUND, 4)
    assert (ad.rounds, ad.partial_rounds) == (2, 1)
    after_s, after_a = t.error_state(), t.accum()
    base, order, n_active = t.adaptive_tiles()
    assert 0 < n_active < len(order)
    idle = np.zeros(len(order), bool)
    idle[order[n_active:]] = True
    m = A.pixel_mask(idle, 37, 61)
    assert m.any() and not m.all()
    assert after_s[m].tobytes() == before_s[m].tobytes() and after_a[m].tobytes() == before_a[m].tobytes()
    assert np.all(after_s[m][:, 0, 3] == 2.0) and np.all(after_s[~m][:, 0, 3] == 4.0)
    assert np.all(after_a[~m][:, 3] == before_a[~m][:, 3] + 8.0)
    t.close()


# ------------------------------------------------------------------------------------------------ error paths
def _rc(t, *args):
    st, ad = abi.PtErrorStats(), abi.PtAdaptiveStats()
    return t.lib.pt_render_adaptive(t._ctx, *args, C.byref(st), C.byref(ad)), t.lib.pt_last_error(t._ctx) or b""


def test_error_paths_leave_the_context_usable(ora):
    spheres, p, solo = _default(ora, 61, 37)
    t = _context(spheres, p, estimate=False)
    rc, msg = _rc(t, 0.1, 1, 4)
    assert rc == abi.PT_ERR_INVALID and b"estimate is off" in msg
    t.error_estimate(True)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert _rc(t, bad, 1, 4)[0] == abi.PT_ERR_INVALID, bad
    assert _rc(t, 0.1, 0, 4)[0] == abi.PT_ERR_INVALID and _rc(t, 0.1, 1, 0)[0] == abi.PT_ERR_INVALID
    assert _rc(t, 0.1, PER_ROUND + 1, 64)[0] == abi.PT_ERR_CAPACITY
    assert t.lib.pt_render_adaptive(t._ctx, 0.1, 1, 4, None, None) == abi.PT_ERR_INVALID
    assert t.lib.pt_adaptive_tiles(t._ctx, None, None, None, None) == abi.PT_ERR_NOT_READY
    assert not t.accum().any() and not t.error_state().any()   # nothing above rendered anything
    # another samples_per_pixel than the estimate holds
    t.render_passes(2)
    q = p.copy()
    q.samples_per_pixel = 2
    t.set_params(q)
    rc, msg = _rc(t, 0.1, 1, 4)
    assert rc == abi.PT_ERR_INVALID and b"clear first" in msg
    assert np.all(t.error_state()[..., 0, 3] == 2.0) and np.all(t.accum()[..., 3] == 8.0)
    # ... and the context still renders: the whole frame from a clear, against the restatement
    t.reset()
    t.set_params(p)
    ref = A.predicted(solo, PER_ROUND, TARGET, CAP)
    st, ad = t.render_adaptive(TARGET, PER_ROUND, CAP)
    _check(t, st, ad, ref, "after the refused calls", _last_partial(ref))
    # a new scene takes the tables back
    n, na = C.c_uint32(), C.c_uint32()
    assert t.lib.pt_adaptive_tiles(t._ctx, None, None, C.byref(n), C.byref(na)) == abi.PT_OK and n.value == 40
    t.set_spheres(spheres)
    assert t.lib.pt_adaptive_tiles(t._ctx, None, None, C.byref(n), C.byref(na)) == abi.PT_ERR_NOT_READY
    with pytest.raises(PtError):
        t.adaptive_tiles()
    # ... and so do another row partition and a resize, while new uniforms for the same rows leave them (csrc/pt_ctx_state.hpp)
    def tables():
        return t.lib.pt_adaptive_tiles(t._ctx, None, None, C.byref(n), C.byref(na))

    for change in ("band", "resize"):
        t.reset()
        t.set_params(p)
        t.render_adaptive(TARGET, PER_ROUND, CAP)
        assert tables() == abi.PT_OK and n.value == 40
        q = t.params.copy()
        q.time += 1.0
        t.set_params(q)
        assert tables() == abi.PT_OK
        if change == "band":
            q.band_rows, q.band_index, q.band_count = 8, 1, 3
            t.set_params(q)
        else:
            assert t.lib.pt_resize(t._ctx, 33, 19) == abi.PT_OK
        assert tables() == abi.PT_ERR_NOT_READY, change
    t.close()
