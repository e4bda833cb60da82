"""The geometry-path autotuner and the grid's class and build policy (csrc/pt_geom_plan.hpp) on the CPU, through
tests/geom_plan_shim.cpp.

All of it schedules: the images are the same bits whatever it decides, so no rendering test can see a slip in it (a wrong
path, class or build would only show as a slower bench line).  Here every decision is pinned: the paths a scene lists, the
PT_GEOM_AUTO launch sequence, settling, the fallbacks of a forced path, the class a view needs and the fit state, what a walk
kernel stages, pt_tune's search over the classes against scripted timings, and pt_refit_grid's decision.  The expected values
were recorded from the code as it stood inline in pt_api.hip before it moved into the header.  CPU only."""
import ctypes as C
import math
import os
import random
import subprocess
import tempfile

import pytest

from test_gpu_grid_classes import need_factor as lensless_need
from test_grid import CLASSES

SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "geom_plan_shim.cpp")
AUTO, LDS, SCALAR, BVH, GRID, SMALL = 0, 1, 2, 3, 4, 5  # include/ptrace.h PT_GEOM_*
D, U, I64 = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
IP = C.POINTER(C.c_int)


def load(so):
    lib = C.CDLL(so)
    scene = [C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint32]
    sigs = {
        "gp_list_paths": (C.c_int, scene + [IP, IP]),
        "gp_autotune": (None, scene + [C.c_int, C.c_int, IP, C.c_int, D, D, IP, IP, IP]),
        "gp_grid_use": (None, scene + [C.c_int, C.c_int, IP]),
        "gp_need_factor": (C.c_double, [D, D, D, C.c_double, D, C.c_double]),
        "gp_fit_state": (C.c_int, [C.c_int, C.c_double, C.c_double]),
        "gp_refit_factor": (C.c_double, [C.c_int, C.c_int, C.c_double]),
        "gp_grid_staging": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int, I64]),
        "gp_hierarchy_staging": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint64, I64]),
        "gp_walk_lds_room": (C.c_uint64, []),
        "gp_classes": (C.c_int, [D]),
        "gp_timed_passes": (C.c_uint32, [C.c_double, C.c_uint32]),
        "gp_tune": (C.c_int, [C.c_double, C.c_double, C.c_int, C.c_uint32, C.c_uint32, IP, U, I64, D, D, D, D, D, D]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(tempfile.mkdtemp(prefix="geom_plan_"), "libgeom_plan_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", SHIM, "-o", so])
    return load(so)


def arr(ctype, values):
    return (ctype * len(values))(*values)


# ---- the ways to read the list ----

# (n_spheres, have_bvh, have_grid, max entries in a cell, always-tested spheres) of the scenes, from the library's host builders
# (pt_build_bvh / pt_build_grid): 9 spheres (State::default, config 4) get neither, configs 2 / 3 and 5 even grids
SCENES = {
    "default_9": (9, 0, 0, 0, 0),
    "config2_484": (484, 1, 1, 6, 4),
    "config5_10001": (10001, 1, 1, 15, 1),
    "struct_16": (16, 1, 1, 3, 0),
    "struct_17": (17, 1, 1, 3, 0),
    "struct_64": (64, 1, 1, 4, 0),
    "struct_65": (65, 1, 1, 4, 0),
    "plain_16": (16, 0, 0, 0, 0),
    "plain_17": (17, 0, 0, 0, 0),
    "irregular_10232": (10232, 0, 0, 0, 0),  # (a non-finite sphere: no structure) the longest list the LDS holds
    "irregular_10233": (10233, 0, 0, 0, 0),
    "uneven_cell_17": (5000, 1, 1, 17, 0),
    "uneven_always_9": (5000, 1, 1, 10, 9),
    "even_edge_16_8": (5000, 1, 1, 16, 8),
    "bvh_only_200": (200, 1, 0, 0, 0),
    "uneven_small_16": (16, 1, 1, 17, 0),
}

PATHS = {
    "default_9": ((SMALL, LDS, SCALAR), 0),
    "config2_484": ((GRID,), GRID),
    "config5_10001": ((GRID,), GRID),
    "struct_16": ((SMALL, LDS, SCALAR, GRID), 0),
    "struct_17": ((LDS, SCALAR, GRID), 0),
    "struct_64": ((LDS, SCALAR, GRID), 0),
    "struct_65": ((GRID,), GRID),
    "plain_16": ((SMALL, LDS, SCALAR), 0),
    "plain_17": ((LDS, SCALAR), 0),
    "irregular_10232": ((LDS, SCALAR), 0),
    "irregular_10233": ((SCALAR,), SCALAR),
    "uneven_cell_17": ((BVH, GRID), 0),
    "uneven_always_9": ((BVH, GRID), 0),
    "even_edge_16_8": ((GRID,), GRID),
    "bvh_only_200": ((BVH,), BVH),
    "uneven_small_16": ((SMALL, LDS, SCALAR, BVH), 0),  # four paths at most: the grid is left out
}


def list_paths(lib, scene):
    out, tuned = (C.c_int * 4)(), C.c_int()
    n = lib.gp_list_paths(*scene, out, C.byref(tuned))
    return tuple(out[:n]), tuned.value


@pytest.mark.parametrize("name", sorted(PATHS))
def test_path_list(shim, name):
    assert list_paths(shim, SCENES[name]) == PATHS[name]


LAUNCH, TRIAL_LAUNCH, EVENTS_DONE, TUNE_RESET = 0, 1, 2, 3


def autotune(lib, scene, ops, policy=AUTO, roulette=False, samples=(1.0,) * 4, ms=(1.0,) * 4):
    n = len(ops)
    paths, trials, out3 = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * 3)()
    lib.gp_autotune(*scene, policy, 1 if roulette else 0, arr(C.c_int, ops), n, arr(C.c_double, samples), arr(C.c_double, ms),
                    paths, trials, out3)
    launches = [(paths[i], trials[i]) for i in range(n) if ops[i] <= TRIAL_LAUNCH]
    return launches, tuple(out3)


def test_auto_sequence_with_trials(shim):
    # the cold launch (not measured), one launch per trial, the first path while the trials are in flight, then the settled path
    ops = [TRIAL_LAUNCH] * 5 + [EVENTS_DONE, TRIAL_LAUNCH, TRIAL_LAUNCH]
    launches, end = autotune(shim, SCENES["default_9"], ops, ms=(3.0, 1.0, 2.0, 0.0))
    assert launches == [(SMALL, -1), (SMALL, 0), (LDS, 1), (SCALAR, 2), (SMALL, -1), (LDS, -1), (LDS, -1)]
    assert end == (LDS, 4, 3)


def test_auto_sequence_without_trials(shim):
    # launches that may not measure (graph-captured frames) take the first path and leave the sequence where it was
    ops = [LAUNCH, LAUNCH, TRIAL_LAUNCH, LAUNCH, TRIAL_LAUNCH, LAUNCH, TRIAL_LAUNCH, TRIAL_LAUNCH, LAUNCH, EVENTS_DONE, LAUNCH]
    launches, end = autotune(shim, SCENES["struct_17"], ops, ms=(2.0, 1.0, 3.0, 0.0))
    assert launches == [(LDS, -1), (LDS, -1), (LDS, -1), (LDS, -1), (LDS, 0), (LDS, -1), (SCALAR, 1), (GRID, 2), (LDS, -1),
                        (SCALAR, -1)]
    assert end == (SCALAR, 4, 3)


def test_auto_single_path_never_measures(shim):
    launches, end = autotune(shim, SCENES["config2_484"], [TRIAL_LAUNCH] * 3 + [LAUNCH])
    assert launches == [(GRID, -1)] * 4
    assert end == (GRID, 0, 1)


def test_pt_tune_reset_measures_again(shim):
    # pt_tune: reset, one cold launch and one per trial, then settle
    ops = [TRIAL_LAUNCH] * 4 + [EVENTS_DONE, TUNE_RESET] + [TRIAL_LAUNCH] * 4 + [EVENTS_DONE, LAUNCH]
    launches, end = autotune(shim, SCENES["uneven_cell_17"], ops, ms=(5.0, 4.0, 0.0, 0.0))
    assert launches == [(BVH, -1), (BVH, 0), (GRID, 1), (BVH, -1), (BVH, -1), (BVH, 0), (GRID, 1), (BVH, -1), (GRID, -1)]
    assert end == (GRID, 3, 2)


@pytest.mark.parametrize("samples,ms,want", [
    ((1.0, 1.0, 1.0), (3.0, 2.0, 1.0), SCALAR),
    ((1.0, 1.0, 1.0), (1.0, 1.0, 1.0), SMALL),    # a tie: the first path wins
    ((1.0, 2.0, 1.0), (2.0, 4.0, 3.0), SMALL),    # per sample: 2 / 2 / 3, the first of equals
    ((1.0, 4.0, 1.0), (2.0, 4.0, 3.0), LDS),      # 2 / 1 / 3
    ((0.0, 1.0, 1.0), (0.5, 1.0, 1.0), SMALL),    # no samples counts as one
    ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), SMALL),
], ids=["fastest_last", "tie", "tie_per_sample", "per_sample", "no_samples", "all_zero"])
def test_settle(shim, samples, ms, want):
    ops = [TRIAL_LAUNCH] * 4 + [EVENTS_DONE, LAUNCH]
    launches, end = autotune(shim, SCENES["default_9"], ops, samples=samples + (1.0,), ms=ms + (0.0,))
    assert launches[-1] == (want, -1) and end[0] == want


# a forced path the scene cannot use falls back to the nearest one it can; the roulette builds have no LDS list walk
FALLBACKS = [
    ("grid_without_grid_to_bvh", "bvh_only_200", GRID, False, BVH),
    ("grid_without_structure_to_scalar", "default_9", GRID, False, SCALAR),
    ("bvh_without_bvh_to_scalar", "default_9", BVH, False, SCALAR),
    ("small_over_16_to_scalar", "plain_17", SMALL, False, SCALAR),
    ("small_at_16", "plain_16", SMALL, False, SMALL),
    ("lds_over_10232_to_scalar", "irregular_10233", LDS, False, SCALAR),
    ("lds_at_10232", "irregular_10232", LDS, False, LDS),
    ("lds_roulette_to_scalar", "default_9", LDS, True, SCALAR),
    ("small_roulette", "default_9", SMALL, True, SMALL),
    ("grid_roulette", "config2_484", GRID, True, GRID),
    ("bvh_forced", "config2_484", BVH, False, BVH),
    ("scalar_forced", "config5_10001", SCALAR, False, SCALAR),
]


@pytest.mark.parametrize("name,scene,policy,roulette,want", FALLBACKS, ids=[f[0] for f in FALLBACKS])
def test_forced_path_fallbacks(shim, name, scene, policy, roulette, want):
    launches, end = autotune(shim, SCENES[scene], [TRIAL_LAUNCH, LAUNCH, TRIAL_LAUNCH], policy=policy, roulette=roulette)
    assert launches == [(want, -1)] * 3
    assert end[1] == 0  # (a forced path never measures)


def test_auto_roulette_takes_scalar_for_the_lds_trial(shim):
    launches, _ = autotune(shim, SCENES["default_9"], [TRIAL_LAUNCH] * 4, roulette=True)
    assert launches == [(SMALL, -1), (SMALL, 0), (SCALAR, 1), (SCALAR, 2)]


def grid_use(lib, scene, policy, tuned):
    out = (C.c_int * 2)()
    lib.gp_grid_use(*scene, policy, tuned, out)
    return tuple(out)


def test_grid_in_use_and_tried(shim):
    # (in use: the next launch may walk the grid; tried: pt_tune may time it — also after PT_GEOM_AUTO settled elsewhere)
    g17 = SCENES["uneven_cell_17"]
    assert grid_use(shim, g17, AUTO, 0) == (1, 1)
    assert grid_use(shim, g17, AUTO, GRID) == (1, 1)
    assert grid_use(shim, g17, AUTO, BVH) == (0, 1)
    assert grid_use(shim, g17, GRID, 0) == (1, 1)
    assert grid_use(shim, g17, BVH, 0) == (0, 0)
    assert grid_use(shim, g17, SCALAR, GRID) == (0, 0)
    assert grid_use(shim, SCENES["uneven_small_16"], AUTO, 0) == (1, 0)  # the grid is not among the four paths listed
    assert grid_use(shim, SCENES["bvh_only_200"], GRID, 0) == (0, 1)
    assert grid_use(shim, SCENES["bvh_only_200"], AUTO, 0) == (0, 0)


# ---- classes, need and fit ----

def test_class_table(shim):
    out = (C.c_double * 16)()
    n = shim.gp_classes(out)
    assert tuple(out[:n]) == CLASSES


def need(lib, origin, u=(1.0, 0.0, 0.0), v=(0.0, 1.0, 0.0), lens=0.0, c0=(0.0, 0.0, 0.0), s0=1.0):
    return lib.gp_need_factor(arr(C.c_double, origin), arr(C.c_double, u), arr(C.c_double, v), lens, arr(C.c_double, c0), s0)


def rho_for(factor, s0=1.0):
    """the camera distance at which the need formula reaches `factor` exactly"""
    return (factor / 1.01 * s0 - s0) * 0.9999


@pytest.mark.parametrize("k", range(len(CLASSES)))
def test_need_at_every_class_boundary(shim, k):
    f = CLASSES[k]
    rho = rho_for(f)
    assert need(shim, (0.0, 0.0, rho * (1 - 1e-4))) == f
    above = CLASSES[k + 1] if k + 1 < len(CLASSES) else CLASSES[-1]
    assert need(shim, (0.0, 0.0, rho * (1 + 1e-4))) == above
    if k == 0:
        assert need(shim, (0.0, 0.0, 0.0)) == CLASSES[0]


def test_need_with_a_lens_beyond_the_classes_and_not_finite(shim):
    # the lens reaches |lens| (|u| + |v|) per axis beyond the camera
    assert need(shim, (0.0, 0.0, 1.9), lens=0.0) == 3.0
    assert need(shim, (0.0, 0.0, 1.9), u=(0.3, 0.0, 0.0), v=(0.0, 0.3, 0.0), lens=1.0) == 4.0
    assert need(shim, (0.0, 0.0, 1.9), u=(0.3, 0.4, 0.0), v=(0.0, 0.3, 0.2), lens=1.0) == 5.5
    assert need(shim, (0.0, 0.0, 1.9), u=(0.3, 0.4, 0.0), v=(0.0, 0.3, 0.2), lens=-1.0) == 5.5
    assert need(shim, (10.0, 20.0, 30.0), c0=(10.0, 20.0, 28.0), s0=2.0) == 2.5
    assert need(shim, (10.0, 20.0, 30.0), c0=(10.0, 20.0, 26.0), s0=2.0) == 4.0
    assert need(shim, (0.0, 0.0, 1000.0)) == 16.0
    assert need(shim, (0.0, 0.0, float("inf"))) == 0.0
    assert need(shim, (float("nan"), 0.0, 0.0)) == 0.0
    assert need(shim, (0.0, 0.0, 1.0), u=(float("inf"), 0.0, 0.0), lens=1.0) == 0.0


def test_need_matches_the_lensless_formula(shim):
    rng = random.Random(7)
    for _ in range(2000):
        s0 = rng.choice([0.5, 1.0, 15.264130592346191, 70.82652282714844])
        rho = s0 * rng.uniform(0.0, 20.0)
        d = [rng.gauss(0, 1) for _ in range(3)]
        norm = math.sqrt(sum(x * x for x in d))
        o = [float(C.c_float(rho * x / norm).value) for x in d]
        rho32 = math.sqrt(sum(x * x for x in o))
        assert need(shim, o, s0=float(C.c_float(s0).value)) == lensless_need(rho32, float(C.c_float(s0).value))


# (in use, need, have) -> state: 0 fits, 1 too small, 2 looser than max(need, 3)
FIT = [
    (0, 4.0, 3.0, 0), (0, 3.0, 8.0, 0), (1, 0.0, 3.0, 0),
    (1, 4.0, 3.0, 1), (1, 4.0, 4.0, 0), (1, 4.0, 5.5, 2),
    (1, 2.5, 2.5, 0), (1, 2.5, 3.0, 0), (1, 2.5, 4.0, 2),
    (1, 3.0, 2.5, 1), (1, 3.0, 3.0, 0), (1, 3.0, 4.0, 2),
    (1, 16.0, 12.0, 1), (1, 16.0, 16.0, 0),
    (1, 4.0, 4.0 - 5e-7, 0), (1, 4.0, 4.0 - 2e-6, 1), (1, 4.0, 4.0 + 5e-7, 0), (1, 4.0, 4.0 + 2e-6, 2),
    (1, 3.0, 3.4, 2),  # (a PT_GRID_DNEAR grid: a factor outside the table)
    # the wider class pt_tune measured faster reads as looser than needed
    (1, 4.0, 8.0, 2),
]


@pytest.mark.parametrize("in_use,need_f,have,want", FIT)
def test_fit_state(shim, in_use, need_f, have, want):
    assert shim.gp_fit_state(in_use, need_f, have) == want


# (policy, fit state, need) -> the class pt_refit_grid rebuilds for (0: none)
REFIT = [
    (0, 0, 4.0, 0.0), (0, 1, 4.0, 4.0), (0, 1, 2.5, 3.0), (0, 2, 2.5, 3.0), (0, 2, 4.0, 4.0),
    (1, 0, 4.0, 0.0), (1, 1, 4.0, 4.0), (1, 1, 2.5, 3.0), (1, 2, 2.5, 0.0), (1, 2, 4.0, 0.0),
    # a refit undoes the wider class pt_tune measured faster, back to max(need, 3)
    (0, 2, 5.5, 5.5),
]


@pytest.mark.parametrize("policy,state,need_f,want", REFIT)
def test_refit_decision(shim, policy, state, need_f, want):
    assert shim.gp_refit_factor(policy, state, need_f) == want


# ---- what a walk kernel stages ----

def test_walk_lds_room(shim):
    assert shim.gp_walk_lds_room() == (((10232 + 7) & ~7) + 4) * 16 - 15 * 4 * 1024


def grid_staging(lib, n_cells, n_entries, cells_build=0, fit=0, room=None):
    b = C.c_uint64()
    kind = lib.gp_grid_staging(n_cells, n_entries, lib.gp_walk_lds_room() if room is None else room, cells_build, fit, C.byref(b))
    return kind, b.value


def cells_bytes(n):
    return (n + 3) // 4 * 16


@pytest.mark.parametrize("cells_build", [0, 1])
@pytest.mark.parametrize("fit", [0, 1, 2])
def test_grid_staging(shim, cells_build, fit):
    room = shim.gp_walk_lds_room()
    c2, c5 = 16 * 1 * 16, 30 * 6 * 30  # configs 2 and 5
    staged_all = cells_build == 0 and fit != 1
    want2 = (1, cells_bytes(c2) + 798 * 16) if staged_all else (2, cells_bytes(c2))
    assert grid_staging(shim, c2, 798, cells_build, fit) == want2
    assert grid_staging(shim, c5, 19482, cells_build, fit) == (2, cells_bytes(c5))  # the entries do not fit
    fits_exactly = (room - cells_bytes(c2)) // 16
    assert grid_staging(shim, c2, fits_exactly, cells_build, fit)[0] == (1 if staged_all else 2)
    assert grid_staging(shim, c2, fits_exactly + 1, cells_build, fit)[0] == 2
    big = room // 16 * 4 + 4  # cell records alone beyond the room
    assert grid_staging(shim, big, 10, cells_build, fit) == (3, 0)
    assert grid_staging(shim, big - 4, 0, cells_build, fit)[0] == (1 if staged_all else 2)


def test_hierarchy_staging(shim):
    b = C.c_uint64()
    room = shim.gp_walk_lds_room()
    # config 2's hierarchy: everything; config 5's: the nodes; nodes beyond the room: nothing
    assert shim.gp_hierarchy_staging(255, 516, room, C.byref(b)) == 0 and b.value == (256 * 2 + 516) * 16
    assert shim.gp_hierarchy_staging(5243, 10492, room, C.byref(b)) == 1 and b.value == 5244 * 16
    assert shim.gp_hierarchy_staging(room // 16, 0, room, C.byref(b)) == 2 and b.value == 0
    assert shim.gp_hierarchy_staging(room // 16 - 1, 0, room, C.byref(b)) == 1 and b.value == room
    n = room // 32 - 1
    assert shim.gp_hierarchy_staging(n, 0, room, C.byref(b)) == 0 and b.value == room


# ---- pt_tune's search over the classes ----

@pytest.mark.parametrize("yard_ms,n_passes,want", [
    (-1.0, 16, 4), (-1.0, 2, 2), (0.0, 16, 4), (0.0, 3, 3), (1.0, 16, 4), (1.0, 2, 2), (10.0, 16, 1), (2.2, 16, 2),
    (1.9, 16, 3), (4.0, 16, 1), (1.0, 1, 1),
])
def test_timed_passes(shim, yard_ms, n_passes, want):
    assert shim.gp_timed_passes(yard_ms, n_passes) == want


def tune(lib, need_f, script, have=3.0, fit_mode=0, n_passes=16, reserved=16):
    """pt_tune's grid part against a scripted device: script = {class: (builds, entries, cells, cold_ms, ms, cells_ms, far)},
    classes not named build a small grid timed at 10 ms with no far rays.  Returns the events ('rebuild', class) /
    ('launch', passes, cells build) and (the class at the end, the cells build kept, launched)."""
    rows = [script.get(f, (1, 100, 64, 10.0, 10.0, 10.0, 0.0)) for f in CLASSES]
    col = lambda k, t: arr(t, [r[k] for r in rows])
    log, out3 = (C.c_double * 300)(), (C.c_double * 3)()
    n = lib.gp_tune(need_f, have, fit_mode, n_passes, reserved, col(0, C.c_int), col(1, C.c_uint32), col(2, C.c_uint64),
                    col(3, C.c_double), col(4, C.c_double), col(5, C.c_double), col(6, C.c_double), log, out3)
    events = [("rebuild", log[3 * i + 1]) if log[3 * i] == 1 else ("launch", int(log[3 * i + 1]), int(log[3 * i + 2]))
              for i in range(n)]
    return events, (out3[0], int(out3[1]), int(out3[2]))


def probe(ms, far=0.0, builds=1, entries=100, cells=64, cold_ms=1.0, cells_ms=None):
    return (builds, entries, cells, cold_ms, ms, ms if cells_ms is None else cells_ms, far)


R, L = "rebuild", "launch"


def test_search_negligible_far_share_times_one_class(shim):
    events, end = tune(shim, 4.0, {4.0: probe(5.0, far=1e-5)})
    assert events == [(R, 4.0), (L, 1, 0), (L, 4, 0)]
    assert end == (4.0, 0, 1)


def test_search_need_25_times_25_and_3(shim):
    events, end = tune(shim, 2.5, {2.5: probe(5.0, cold_ms=2.0), 3.0: probe(4.0)})
    assert events == [(R, 2.5), (L, 1, 0), (L, 2, 0), (R, 3.0), (L, 2, 0)]
    assert end == (3.0, 0, 1)
    events, end = tune(shim, 2.5, {2.5: probe(4.0, cold_ms=2.0), 3.0: probe(4.0)})  # a tie: the first timed stays
    assert events == [(R, 2.5), (L, 1, 0), (L, 2, 0), (R, 3.0), (L, 2, 0), (R, 2.5)]
    assert end == (2.5, 0, 1)


def test_search_widens_twice_while_wider_wins(shim):
    script = {3.0: probe(9.0, far=1e-3, cold_ms=0.5), 4.0: probe(7.0, far=1e-3), 5.5: probe(6.0, far=1e-3), 8.0: probe(1.0)}
    events, end = tune(shim, 3.0, script, have=2.5)
    assert events == [(R, 3.0), (L, 1, 0), (L, 4, 0), (R, 4.0), (L, 4, 0), (R, 5.5), (L, 4, 0)]
    assert end == (5.5, 0, 1)


def test_search_stops_when_wider_loses(shim):
    script = {3.0: probe(6.0, far=1e-3, cold_ms=1.5), 4.0: probe(7.0, far=1e-3), 5.5: probe(1.0)}
    events, end = tune(shim, 3.0, script)
    assert events == [(L, 1, 0), (L, 3, 0), (R, 4.0), (L, 3, 0), (R, 3.0)]
    assert end == (3.0, 0, 1)


def test_search_far_share_edge(shim):
    events, _ = tune(shim, 3.0, {3.0: probe(6.0, far=2e-5), 4.0: probe(1.0)})
    assert events == [(L, 1, 0), (L, 4, 0), (R, 4.0), (L, 4, 0)]
    events, _ = tune(shim, 3.0, {3.0: probe(6.0, far=1.99e-5), 4.0: probe(1.0)})
    assert events == [(L, 1, 0), (L, 4, 0)]


def test_search_skips_a_class_without_a_grid(shim):
    # the class the camera needs builds no grid: no yardstick, the default class timed warm
    events, end = tune(shim, 2.5, {2.5: probe(1.0, builds=0), 3.0: probe(5.0)})
    assert events == [(L, 4, 0)]
    assert end == (3.0, 0, 1)
    # a wider class without a grid ends the widening
    script = {3.0: probe(6.0, far=1e-3), 4.0: probe(1.0, builds=0), 5.5: probe(1.0)}
    events, end = tune(shim, 3.0, script)
    assert events == [(L, 1, 0), (L, 4, 0)]
    assert end == (3.0, 0, 1)
    # nothing builds (no grid for the class is no error, and the grid in place stays)
    nothing = {f: probe(1.0, builds=0) for f in CLASSES}
    assert tune(shim, 5.5, nothing, have=3.0) == ([], (3.0, 0, 0))


def test_search_from_16_has_no_wider_class(shim):
    events, end = tune(shim, 16.0, {16.0: probe(5.0, far=0.5, cold_ms=3.0)})
    assert events == [(R, 16.0), (L, 1, 0), (L, 2, 0)]
    assert end == (16.0, 0, 1)
    events, end = tune(shim, 8.0, {8.0: probe(5.0, far=0.5), 12.0: probe(4.0, far=0.5), 16.0: probe(3.0, far=0.5)})
    assert events == [(R, 8.0), (L, 1, 0), (L, 4, 0), (R, 12.0), (L, 4, 0), (R, 16.0), (L, 4, 0)]
    assert end == (16.0, 0, 1)


@pytest.mark.parametrize("yard,want", [(0.0, 4), (1.0, 4), (10.0, 1)])
def test_search_yardstick(shim, yard, want):
    events, _ = tune(shim, 4.0, {4.0: probe(5.0, cold_ms=yard)}, have=4.0)
    assert events == [(L, 1, 0), (L, want, 0)]
    events, _ = tune(shim, 4.0, {4.0: probe(5.0, cold_ms=yard)}, have=4.0, n_passes=2, reserved=2)
    assert events == [(L, 1, 0), (L, min(want, 2), 0)]


def test_unmeasured_branch(shim):
    assert tune(shim, 4.0, {}, fit_mode=1) == ([(R, 4.0)], (4.0, 0, 0))
    assert tune(shim, 3.0, {}, fit_mode=1) == ([], (3.0, 0, 0))
    # more passes than are reserved falls back to the unmeasured class, even 2.5
    assert tune(shim, 2.5, {}, n_passes=8, reserved=4) == ([(R, 2.5)], (2.5, 0, 0))
    assert tune(shim, 2.5, {}, n_passes=4, reserved=4)[0][0] == (R, 2.5)


ENTRIES_16K = 16384 // 16


@pytest.mark.parametrize("entries,cells_ms,want_timed,want_kept", [
    (ENTRIES_16K, 1.0, False, 0),         # 16 KB of entries: not timed
    (ENTRIES_16K + 1, 1.0, True, 1),
    (ENTRIES_16K + 1, 0.98 * 5.0, True, 1),  # at least 2 % faster: kept
    (ENTRIES_16K + 1, 4.91, True, 0),
    (ENTRIES_16K + 1, 6.0, True, 0),
    (6000, 1.0, True, 1),
    (6400, 1.0, False, 0),                # entries beyond the LDS: build 2 anyway
])
def test_cells_build_gate(shim, entries, cells_ms, want_timed, want_kept):
    events, end = tune(shim, 4.0, {4.0: probe(5.0, entries=entries, cells_ms=cells_ms, cold_ms=1.0)}, have=4.0)
    timed = [(L, 1, 0), (L, 4, 0)]
    assert events == timed + ([(L, 1, 1), (L, 4, 1)] if want_timed else [])
    assert end == (4.0, want_kept, 1)


def test_cells_build_times_the_kept_class(shim):
    script = {2.5: probe(5.0, entries=1500, cold_ms=2.0), 3.0: probe(4.0, entries=1200, cells_ms=3.0)}
    events, end = tune(shim, 2.5, script)
    assert events == [(R, 2.5), (L, 1, 0), (L, 2, 0), (R, 3.0), (L, 2, 0), (L, 1, 1), (L, 2, 1)]
    assert end == (3.0, 1, 1)
