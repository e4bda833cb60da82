"""The host's state of the work queue's tile order (csrc/pt_tile_order.hpp) on the CPU, through tests/tile_order_shim.cpp.

The order only schedules: images never depend on it, so no rendering test can see a slip in these rules — an order kernel that
runs when it need not, or a probe that is skipped, shows only as a slower bench line, a stale order as a wrong `base` from
pt_adaptive_tiles.  Here every transition is pinned: the sequences the entry points produce, each with a re-seed in the middle,
and a seeded random walk against a restatement of the table (Model below).  CPU only."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import pytest

SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tile_order_shim.cpp")
RESEED, UNIFORM, FRAMES, PARTIAL, NEW_SCENE = range(5)
SAME_AS_BASE = {7}   # tile_order_shim.cpp view_params: view 7 differs from view 0 only in fields that are not part of the view


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(tempfile.mkdtemp(prefix="tile_order_"), "libtile_order_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", SHIM, "-o", so])
    lib = C.CDLL(so)
    lib.tile_order_run.restype = C.c_int
    lib.tile_order_run.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_uint32)]
    return lib


def reseed():
    return (RESEED, 0, 0, 0, 0)


def new_scene():
    return (NEW_SCENE, 0, 0, 0, 0)


def uniform(feedback, captured=False):
    return (UNIFORM, int(feedback), int(captured), 0, 0)


def frames(spp, view=0, n=1, captured=False):
    return (FRAMES, spp, view, n, int(captured))


def partial():
    return (PARTIAL, 0, 0, 0, 0)


def run(lib, events):
    """Per event (order kernel runs, costs zeroed, probe runs, valid, pending, probed, frames_since_probe), on a fresh state."""
    flat = (C.c_int * (5 * len(events)))(*[x for e in events for x in e])
    out = (C.c_uint32 * (7 * len(events)))()
    assert lib.tile_order_run(flat, len(events), out) == 0
    return [tuple(out[7 * i:7 * i + 7]) for i in range(len(events))]


def actions(lib, events):
    """Per event the letters of what is enqueued: k order kernel, z costs zeroed, p probe."""
    return ["".join(c for c, on in zip("kzp", r[:3]) if on) for r in run(lib, events)]


class Model:
    """The table, restated: what each event enqueues and the state it leaves."""

    def __init__(self):
        self.valid = self.pending = self.probed = False
        self.view, self.gen, self.scene, self.since = None, 0, 0, 0

    def step(self, ev):
        kind, a, b, c, d = ev
        k = z = p = False
        if kind == RESEED:
            self.valid = self.probed = self.pending = False
        elif kind == NEW_SCENE:
            self.scene += 1
        elif kind == UNIFORM:                      # a = cost feedback, b = captured
            k = bool(a) or not self.valid
            if k and not b:
                self.valid, self.pending = True, False
            if a and not b:
                self.pending = True
        elif kind == PARTIAL:
            k = self.pending or not self.valid
        elif kind == FRAMES:                       # a = spp, b = view, c = frames, d = captured
            view = 0 if b in SAME_AS_BASE else b
            if a < 4:
                if self.probed:
                    self.probed = self.valid = self.pending = False
                    z = True
                k = not self.valid
            else:
                fresh = self.probed and self.valid and self.gen == self.scene and (self.view == view or self.since < 64)
                self.since = (self.since + c) & 0xffffffff
                if not fresh:
                    k = not self.valid
                    p = not d
        if k and kind in (PARTIAL, FRAMES):        # the capture status is not consulted
            self.valid, self.pending = True, False
        if p:
            self.probed, self.pending, self.view, self.gen, self.since = True, False, view, self.scene, 0
        return (int(k), int(z), int(p), int(self.valid), int(self.pending), int(self.probed), self.since)


def model(events):
    m = Model()
    return [m.step(e) for e in events]


# ------------------------------------------------------------------------------------------------ pinned sequences
def test_a_fresh_context_runs_the_order_kernel_once(shim):
    assert actions(shim, [uniform(False), uniform(False), uniform(False)]) == ["k", "", ""]
    assert run(shim, [uniform(False)])[0][3:6] == (1, 0, 0)
    # with feedback it runs before every launch, and costs stay pending after each
    got = run(shim, [uniform(True), uniform(True), uniform(False)])
    assert [g[:6] for g in got] == [(1, 0, 0, 1, 1, 0), (1, 0, 0, 1, 1, 0), (0, 0, 0, 1, 1, 0)]


def test_a_partial_round_consumes_pending_costs_once(shim):
    """tests/test_gpu_adaptive.py test_a_partial_round_leaves_the_cost_order_as_it_found_it, seen from the host"""
    ev = [uniform(True), partial(), partial()]
    assert actions(shim, ev) == ["k", "k", ""]
    assert [g[3:5] for g in run(shim, ev)] == [(1, 1), (1, 0), (1, 0)]
    # without feedback nothing is pending: the partial round keeps the order it finds
    assert actions(shim, [uniform(False), partial()]) == ["k", ""]
    # a partial round on a fresh state has to make an order first
    assert actions(shim, [partial(), partial()]) == ["k", ""]


def test_a_captured_order_kernel_does_not_count_as_run(shim):
    ev = [uniform(False, captured=True), uniform(False), uniform(False)]
    assert actions(shim, ev) == ["k", "k", ""]
    assert [g[3:5] for g in run(shim, ev)] == [(0, 0), (1, 0), (1, 0)]
    # a captured launch with feedback leaves nothing pending either
    ev = [uniform(False), uniform(True, captured=True), partial()]
    assert actions(shim, ev) == ["k", "k", ""]
    # ... but a frame's or a partial round's order kernel counts whatever the capture status (frames: as the code always had it)
    assert actions(shim, [frames(1, captured=True), frames(1), uniform(False)]) == ["k", "", ""]


def test_frames_of_four_samples_probe_per_view_and_scene(shim):
    ev = [frames(4, 0, 5), frames(4, 0, 5), frames(4, 0, 100),      # a probe, then none at the same view however many frames
          frames(4, 1, 10),                                          # 110 frames since the probe and another view: a probe
          frames(4, 2, 30), frames(4, 2, 30), frames(4, 2, 3), frames(4, 2, 1),  # yet another view, but 0, 30, 60, 63 frames since: none
          new_scene(), frames(4, 2, 1),                              # at once after a new scene
          frames(4, 3, 100, captured=True), frames(4, 3, 1, captured=True), frames(4, 3, 1)]  # none while capturing
    assert actions(shim, ev) == ["kp", "", "", "p", "", "", "", "", "", "p", "", "", "p"]
    got = run(shim, ev)
    assert [g[6] for g in got] == [0, 5, 105, 0, 30, 60, 63, 64, 64, 0, 100, 101, 0]
    assert all(g[3:6] == (1, 0, 1) for g in got)
    # a change in any field of the view counts (64 frames after the probe), a change in other fields does not
    for view in range(1, 9):
        want = ["kp", "", "" if view in SAME_AS_BASE else "p"]
        assert actions(shim, [frames(4, 0, 1), frames(4, 0, 64), frames(4, view, 1)]) == want, view
    # a probe consumes pending costs; a uniform launch with feedback afterwards leaves the probed order in place
    ev = [uniform(True), frames(8), uniform(True), frames(8), partial()]
    assert actions(shim, ev) == ["k", "p", "k", "", "k"]
    assert [g[3:6] for g in run(shim, ev)] == [(1, 1, 0), (1, 0, 1), (1, 1, 1), (1, 1, 1), (1, 0, 1)]


def test_frames_below_four_samples_restore_the_identity_order_once(shim):
    ev = [frames(4), frames(1), frames(1), frames(2), frames(3, 1, 100)]
    assert actions(shim, ev) == ["kp", "kz", "", "", ""]
    assert [g[3:6] for g in run(shim, ev)] == [(1, 0, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0)]
    # without a probed series there is nothing to restore, whatever a uniform launch reported
    assert actions(shim, [uniform(True), frames(1), frames(1)]) == ["k", "", ""]
    assert actions(shim, [frames(1), frames(1)]) == ["k", ""]
    # ... and the next series of four samples probes again
    assert actions(shim, [frames(4), frames(1), frames(4)]) == ["kp", "kz", "p"]


SEQUENCES = {
    "uniform": [uniform(False), uniform(False), uniform(True), uniform(False)],
    "partial": [uniform(True), partial(), partial(), uniform(True), partial()],
    "captured": [uniform(False, True), uniform(False), uniform(True, True), uniform(False)],
    "frames 4 spp": [frames(4, 0, 5), frames(4, 0, 5), frames(4, 1, 60), frames(4, 1, 1), new_scene(), frames(4, 1, 1),
                     frames(4, 2, 99, True), frames(4, 2, 1)],
    "frames 1 spp": [frames(4), frames(1), frames(1), frames(4), frames(2)],
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_a_reseed_in_the_middle(shim, name):
    """After a re-seed the device holds the identity order and zero costs: whatever comes next makes an order of its own, frames
    of four samples probe again, frames below four have nothing to restore.  Every position, against the restatement."""
    seq = SEQUENCES[name]
    assert run(shim, seq) == model(seq)
    for cut in range(len(seq) + 1):
        ev = seq[:cut] + [reseed()] + seq[cut:]
        got = run(shim, ev)
        assert got == model(ev), (name, cut)
        assert got[cut][:6] == (0, 0, 0, 0, 0, 0), (name, cut)
        nxt = next((i for i in range(cut + 1, len(ev)) if ev[i][0] in (UNIFORM, FRAMES, PARTIAL)), None)
        if nxt is None:
            continue
        k, z, p = got[nxt][:3]
        assert k == 1 and z == 0, (name, cut)
        if ev[nxt][0] == FRAMES:
            assert p == (1 if ev[nxt][1] >= 4 and not ev[nxt][4] else 0), (name, cut)


def test_a_seeded_random_walk_against_the_restatement(shim):
    rng = random.Random(20240612)
    for walk in range(8):
        ev = []
        for _ in range(600):
            r = rng.random()
            if r < 0.04:
                ev.append(reseed())
            elif r < 0.08:
                ev.append(new_scene())
            elif r < 0.38:
                ev.append(uniform(rng.random() < 0.5, rng.random() < 0.2))
            elif r < 0.55:
                ev.append(partial())
            else:
                ev.append(frames(rng.choice([1, 2, 3, 4, 8, 25]), rng.choice([0, 0, 0, 1, 5, 7, 8]), rng.choice([1, 1, 5, 16, 64, 200]),
                                 rng.random() < 0.15))
        got, want = run(shim, ev), model(ev)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (walk, i, ev[max(0, i - 5):i + 1], g, w)
        seen = {(e[0], g[:3]) for e, g in zip(ev, got)}
        # not vacuous: every kind of answer occurred
        for need in ((UNIFORM, (1, 0, 0)), (UNIFORM, (0, 0, 0)), (PARTIAL, (1, 0, 0)), (PARTIAL, (0, 0, 0)), (FRAMES, (1, 1, 0)),
                     (FRAMES, (0, 0, 1)), (FRAMES, (1, 0, 1)), (FRAMES, (0, 0, 0)), (FRAMES, (1, 0, 0))):
            assert need in seen, (walk, need)
