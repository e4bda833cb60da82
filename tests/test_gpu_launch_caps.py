"""The pixel and tile kernels around the trace kernels PAST THEIR LAUNCH CAPS, at the smallest shapes that get there, against the
restatements the small-shape tests use (tests/readout_ref.py, error_ref.py, adaptive_ref.py) and the oracle's passes.

Every kernel that folds passes, keeps the error estimate, reads pictures out or blends frames strides a capped grid over its
pixels or tiles (csrc/pt_api.hip):

    pixel_grid(n) = grid_for(n, 256, 2048)   workgroups of 256 threads, at most 2048 of them: 2048 x 256 = 524 288 threads, so
                                             up to 524 288 pixels the grid-stride loop makes one trip, above that several —
                                             pt_fold_error_kernel, pt_resolve_error_kernel, pt_resolve_kernel,
                                             pt_resolve_rgba8_kernel, pt_blend_rgba8_kernel, pt_frame_blend_kernel,
                                             pt_frames_blend_kernel, pt_accumulate_kernel
    tile_grid(n)  = grid_for(n, 4, 4096)     a wave64 per tile, four per workgroup, at most 4096 workgroups: 16 384 waves, so the
                                             `j += waves` loop starts its second trip at 16 385 tiles —
                                             pt_error_tiles_kernel, pt_fold_error_tiles_kernel

No other test of these kernels is larger than 160x88 (1280x702 has 898 560 pixels, 1920x1080 has 2 073 600 and 32 400 tiles).

    A = 1024x513   525 312 pixels = 524 288 + one row: the last image row is the second trip of every pixel kernel
    B = 1025x1021  129 x 128 = 16 512 tiles: the last 128 are the second trip of the tile kernels; the right edge tiles are one
                   pixel wide, the bottom ones five rows high; 1 046 525 pixels
    (C = 264x256, 33 x 32 = 1 056 tiles — two positions per thread of the partition kernel — is a case of
    tests/test_gpu_adaptive.py; the table kernels at every size: tests/test_gpu_tile_tables.py)

Floats are compared as bit patterns except where both sides are NaN, bytes and counts outright; no tolerance anywhere."""
import numpy as np
import pytest

import adaptive_ref as A
import error_ref as E
import readout_ref as R
import test_gpu_adaptive as TA
import test_gpu_error_estimate as TE
import test_gpu_readout_edges as TR

pytestmark = pytest.mark.gpu

PIXEL_CAP = 2048 * 256   # pixel_grid: workgroups x threads
TILE_CAP = 4096 * 4      # tile_grid: workgroups x waves
A_W, A_H = 1024, 513
B_W, B_H = 1025, 1021


def test_the_shapes_are_the_smallest_that_pass_their_caps():
    assert A_W * (A_H - 1) == PIXEL_CAP and A_W * A_H == 525312
    ty, tx = A.tile_shape(A_H, A_W)
    assert ty * tx == 8320 <= TILE_CAP
    ty, tx = A.tile_shape(B_H, B_W)
    assert (tx, ty) == (129, 128) and tx * ty == 16512 > TILE_CAP and B_W * B_H == 1046525
    assert (tx - 1) * ty <= TILE_CAP and tx * (ty - 1) <= TILE_CAP   # a tile column or a tile row fewer stays below the cap
    assert B_W - 8 * (tx - 1) == 1 and B_H - 8 * (ty - 1) == 5


def _spread_hand_state(w, h):
    """error_ref.hand_state at this size — every operand class of n, k and M2 in a column of tiles, ordinary pixels elsewhere —
    with every row of tiles shifted 13 tiles further right than the one above (wrapping), so the classes cross the whole
    image, the last row and the second trip included; a narrower last column of tiles takes the sixteen classes in turn, one
    per row of tiles."""
    hand, classes = E.hand_state(w, h)
    st = hand.copy()
    for ty in range((h + 7) // 8):
        rows = slice(8 * ty, 8 * ty + 8)
        st[rows] = np.roll(hand[rows], 8 * 13 * ty, axis=1)
        if w % 8:
            col = classes[ty % len(classes)][2]
            st[rows, 8 * (w // 8):] = hand[rows, 8 * col:8 * col + w % 8]
    return st


def _every_class(state, what):
    classes = E.hand_classes(state)
    assert all(v > 0 for v in classes.values()), (what, classes)


# ------------------------------------------------------------------------------------------------ A: read-out
def test_shape_a_resolve_kernels_on_a_loaded_buffer():
    """pt_load_accum, then pt_resolve and pt_resolve_rgba8 with gamma 0 and 1: a random draw of the edge colours under a count
    per pixel (pt_load_accum wants the same whole count in the first and the last pixel: small_accum keeps 3 there)."""
    t, _ = TR._context(A_W, A_H)
    acc = R.small_accum(A_H, A_W, 21)
    counts = R.count_classes(acc[-1:])
    assert all(v > 0 for v in counts.values()), counts   # the second trip's row holds every count of the cycle
    TR._check_read_outs(t, acc, "1024x513")
    t.close()


def test_shape_a_blend_rgba8_under_every_rule():
    """pt_blend_rgba8 under every rule of readout_ref.BLEND_RULES on a buffer whose counts vary from pixel to pixel, against a
    texture with every byte value in every channel."""
    t, p = TR._context(A_W, A_H)
    acc = R.blend_accum(A_H, A_W, seed=46)
    prev = R.seed_texture(A_H, A_W, 47, every_byte=True)
    t.load_accum(acc)
    for rc, avg, wt in R.BLEND_RULES:
        q = p.copy()
        q.render_count, q.should_average, q.last_frame_weight = rc, avg, wt
        t.set_params(q)
        TR._same_bytes(t.blend_rgba8(prev), R.blend_rgba8(acc, prev, rc, avg, wt), "1024x513, rule %r" % ((rc, avg, wt),))
    t.close()


# ------------------------------------------------------------------------------------------------ A: fold
def test_shape_a_fold_and_accumulate_kernels_against_the_oracle_passes(ora):
    """pt_render_passes(3) at 1 spp.  Estimate on (pt_fold_error_kernel): accum and raw state are error_ref.fold of the
    oracle's three passes.  Estimate off (pt_accumulate_kernel): accum is the oracle's sum.  pt_resolve_error
    (pt_resolve_error_kernel) is the restatement's read-out, of that state and of a loaded hand-made state with every operand
    class of error_ref.hand_state across the whole image."""
    spheres, p = E.estimate_scene(A_W, A_H, spp=1)
    passes = E.oracle_passes(ora, spheres, p, 3)
    ref_state, ref_acc = E.fold(E.empty_state(A_H, A_W), np.zeros((A_H, A_W, 4), np.float32), passes)
    total = ora.render(spheres, p, 3)[0]
    assert E.same_floats(ref_acc, total), "the fold's adds are not the oracle's sum: %s" % E.first_difference(ref_acc, total)
    on, off = TE._context(spheres, p, reserve=3), TE._context(spheres, p, reserve=3, estimate=False)
    on.render_passes(3)
    off.render_passes(3)
    got = off.accum()
    assert E.same_floats(got, total), "estimate off, accum: %s" % E.first_difference(got, total)
    got = on.accum()
    assert E.same_floats(got, ref_acc), "estimate on, accum: %s" % E.first_difference(got, ref_acc)
    got = on.error_state()
    assert E.same_floats(got, ref_state), "raw state: %s" % E.first_difference(got, ref_state)
    assert np.all(got[..., 0, 3] == 3.0) and np.all(got[..., 1, 3] == 3.0)
    got, want = on.error_image(), E.resolve_error(ref_state)
    assert E.same_floats(got, want), "pt_resolve_error of the folded state: %s" % E.first_difference(got, want)
    hand = _spread_hand_state(A_W, A_H)
    _every_class(hand[-1:], "the last row")
    on.load_error_state(hand)
    got, want = on.error_image(), E.resolve_error(hand)
    assert E.same_floats(got, want), "pt_resolve_error of the hand-made state: %s" % E.first_difference(got, want)
    on.close()
    off.close()


# ------------------------------------------------------------------------------------------------ A: frames
@pytest.fixture(scope="module")
def frame_set(ora):
    """Two contexts at 1024x513 (one replays groups of frames, one is stepped tick by tick) and the oracle's pass of each of
    the 23 frames (it depends on the clock alone)."""
    spheres, p = R.frame_scene(w=A_W, h=A_H)
    pair = TR._FramePair(spheres, p)
    yield pair, R.oracle_passes(ora, spheres, p, 23)
    pair.close()


@pytest.mark.parametrize("name", ["n23", "no_averaging"])
def test_shape_a_frames_grouped_and_tick_by_tick(frame_set, name):
    """pt_render_frames (n23: groups of 16 and 4 through pt_frames_blend_kernel, then three single frames through
    pt_frame_blend_kernel) against pt_render_frame tick by tick and against the restatement's chain of the oracle's passes:
    canvas and both textures, averaging and not."""
    pair, passes = frame_set
    s = next(s for s in R.FRAME_SERIES if s["name"] == name)
    assert pair.rows == A_H and s["band"] is None
    seeds = [R.seed_texture(A_H, A_W, 50), R.seed_texture(A_H, A_W, 51)]
    TR._check_series(pair, passes, s, seeds)


# ------------------------------------------------------------------------------------------------ B: tile records
def test_shape_b_tile_records_of_a_hand_made_state():
    """A loaded hand-made state, nothing rendered: pt_error_tiles (pt_error_tiles_kernel) is error_ref.tiles, pt_error_stats is
    error_ref.stats, pt_resolve_error the restatement's read-out — 16 512 tiles, the last 128 in the kernel's second trip."""
    spheres, p = E.estimate_scene(B_W, B_H, spp=1)
    t = TE._context(spheres, p, reserve=1)
    hand = _spread_hand_state(B_W, B_H)
    _every_class(hand[-5:], "the bottom row of tiles")       # tiles 16 384 ... 16 511: the second trip
    _every_class(hand[:, -1:], "the one-pixel column of tiles")
    t.load_error_state(hand)
    st = TE._check_read_outs(t, hand, "1025x1021")
    assert st.pixels == B_W * B_H and 0 < st.pixels_counted < st.pixels and st.pixels_short > 0 and st.pixels_nonfinite > 0
    t.close()


# ------------------------------------------------------------------------------------------------ B: a partial round
def test_shape_b_partial_round_of_more_than_16384_active_tiles(ora):
    """One round of pt_render_adaptive, one pass at 1 spp, on a loaded state in which 100 tiles (neither the first nor the
    last) hold n = 2, M2 = 0 — standard error 0: never selected — and every other pixel n = 1: short, always selected.  The
    round is partial with 16 412 active tiles, so pt_fold_error_tiles_kernel makes a second trip.  The accumulation agrees
    with the state (w = n spp, rgb = mean w); both go in through their device pointers (pt_load_accum would clear the state
    and wants one count in the first and the last pixel)."""
    frame = TA._frame(ora, ("caps B",), lambda: E.estimate_scene(B_W, B_H, spp=1))
    spheres, p, solo = frame
    n_tiles = 16512
    rng = np.random.default_rng(31)
    idle = np.zeros(n_tiles, bool)
    idle[rng.choice(np.arange(1, n_tiles - 1), 100, replace=False)] = True
    m = A.pixel_mask(idle, B_H, B_W)
    state = E.empty_state(B_H, B_W)
    state[..., 0, :3] = rng.uniform(0.05, 1.5, (B_H, B_W, 3)).astype(np.float32)
    state[..., 0, 3] = np.where(m, 2.0, 1.0)
    state[..., 1, 3] = np.where(m, 2.0, 1.0)     # k = n spp
    accum = np.empty((B_H, B_W, 4), np.float32)
    accum[..., 3] = state[..., 0, 3]             # w = n spp
    accum[..., :3] = state[..., 0, :3] * accum[..., 3:]
    # what the restatement says, before a look at the device
    flags = A.select(state, TA.TARGET)
    n_active = int(flags.sum())
    assert flags.tolist() == (~idle).tolist() and n_active == n_tiles - 100 == 16412 > TILE_CAP
    ref = A.predicted(solo, 1, TA.TARGET, 1, state=state, accum=accum)
    ad = ref["adaptive"]
    assert ref["rounds"][0]["active"].tolist() == flags.tolist() and ref["rounds"][0]["partial"]
    assert (ad["rounds"], ad["partial_rounds"], ad["tile_passes"]) == (1, 1, n_active) and ref["stats"]["reached"] == 0
    assert ad["samples"] == int((~m).sum()) and ref["next"] == 1
    t = TA._context(spheres, p, reserve=1)
    TA._load_accum_raw(t, accum)
    t.load_error_state(state)
    st, got_ad = t.render_adaptive(TA.TARGET, 1, 1)
    TA._check(t, st, got_ad, ref, "1025x1021, one partial round", TA._last_partial(ref), spp=1)
    after_s, after_a = t.error_state(), t.accum()
    assert after_s[m].tobytes() == state[m].tobytes() and after_a[m].tobytes() == accum[m].tobytes(), "an idle tile was written"
    assert np.all(after_s[..., 0, 3] == 2.0) and np.all(after_a[..., 3] == 2.0)
    base, order, got_active = t.adaptive_tiles()
    assert got_active == n_active and set(order[n_active:].tolist()) == set(np.flatnonzero(idle).tolist())
    t.close()
