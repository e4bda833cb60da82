"""What a context knows about its derived products (csrc/pt_ctx_state.hpp) on the CPU, through tests/ctx_state_shim.cpp: the
change table from every combination of the flags, the accumulation tallies' transitions with the numbers written out, and the
effective row partition; then the stand-alone program tests/ctx_state_main.cpp under the address and undefined-behaviour
sanitizers, run as a child.  The expected rows are stated here, not read from the header.  CPU only; nothing sanitized is loaded
into this process."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from ray_tracer_webgl_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
FEAT, HIST, ADAPT, UUID, CELLS, SPHERES, PARAMS = (1 << k for k in range(7))   # the shim's numbering of the flags
ALL = 127
# change (in the order of the header's enum) -> (flags it drops, flags it establishes, does scene_gen move on)
TABLE = (
    ("SCENE_DROPPED", SPHERES | UUID | FEAT | HIST, 0, False),
    ("SCENE_INSTALLED", CELLS | ADAPT, SPHERES, True),
    ("UNIFORMS_SAME_ROWS", FEAT, PARAMS, False),
    ("ROWS_ASKED", FEAT | HIST, 0, False),
    ("UNIFORMS_OTHER_ROWS", FEAT | HIST | ADAPT, PARAMS, False),
    ("RESIZED", PARAMS | FEAT | HIST | ADAPT, 0, False),
    ("GRID_REBUILT", UUID | FEAT, 0, False),
    ("TILE_COUNT_CHANGED", ADAPT, 0, False),
    ("PARTIAL_ROUND_BEGINS", ADAPT, 0, False),
    ("PARTIAL_ROUND_DONE", 0, ADAPT, False),
    ("REPROJECTED", HIST, 0, False),
    ("UUIDS_UPLOADED", 0, UUID, False),
    ("CELLS_BUILD_UNMEASURED", CELLS, 0, False),
    ("CELLS_BUILD_CHOSEN", 0, CELLS, False),
)
EMPTIED, REPARTITIONED, OWN_FRESH, REBOUND, LOADED, UNIFORM, FRAMES, PARTIAL = range(8)


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(tempfile.mkdtemp(prefix="ctx_state_"), "libctx_state_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", os.path.join(HERE, "ctx_state_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    u32, u64 = C.c_uint32, C.c_uint64
    lib.ctx_changed.restype = None
    lib.ctx_changed.argtypes = [C.c_int, u32, C.POINTER(u64)]
    lib.tally_apply.argtypes = [C.POINTER(u64), C.c_int, u64, u64, u64, u64]
    lib.partition_get.argtypes = [u32, u32, u32, C.POINTER(u32)]
    lib.partition_equal.argtypes = [u32] * 6
    return lib


def test_every_change_drops_exactly_its_row_from_every_combination_of_the_flags(shim):
    assert shim.ctx_change_count() == len(TABLE)
    out = (C.c_uint64 * 3)()
    visited = 0
    for change, (name, drops, makes, gen) in enumerate(TABLE):
        assert not drops & makes, name
        for bits in range(ALL + 1):
            shim.ctx_changed(change, bits, out)
            assert out[0] == (bits & ~drops) | makes, (name, bin(bits), bin(out[0]))   # every other flag keeps its value
            assert out[1] == (42 if gen else 41) and out[2] == 1, (name, bits, out[1], out[2])   # est.spp, hist.ran, the options: never
            visited += 1
    assert visited == 14 * 128


def test_the_rows_of_one_call_together(shim):
    """what the calls that report two changes leave: an accepted pt_set_spheres (every flag of the old scene gone, the uuid arrays
    back when something wants them), a refused one, and a repartition refused by its allocation"""
    out = (C.c_uint64 * 3)()

    def after(bits, *names):
        for n in names:
            shim.ctx_changed([t[0] for t in TABLE].index(n), bits, out)
            bits = out[0]
        return bits

    assert after(ALL, "SCENE_DROPPED", "SCENE_INSTALLED") == SPHERES | PARAMS
    assert after(ALL, "SCENE_DROPPED", "UUIDS_UPLOADED", "SCENE_INSTALLED") == SPHERES | PARAMS | UUID
    assert after(ALL, "SCENE_DROPPED", "SCENE_DROPPED") == PARAMS | ADAPT | CELLS   # refused: no scene, the tables and the build as found
    assert after(ALL, "ROWS_ASKED") == ALL & ~(FEAT | HIST)   # the fit refused: the old rows and uniforms stay
    assert after(ALL, "ROWS_ASKED", "TILE_COUNT_CHANGED", "UNIFORMS_OTHER_ROWS") == ALL & ~(FEAT | HIST | ADAPT)
    assert after(ALL, "GRID_REBUILT", "UUIDS_UPLOADED") == ALL & ~FEAT
    assert after(ALL, "PARTIAL_ROUND_BEGINS", "PARTIAL_ROUND_DONE") == ALL


def tally(shim, state, op, a=0, b=0, c=0, d=0):
    s = (C.c_uint64 * 4)(*state)
    nothing = shim.tally_apply(s, op, a, b, c, d)
    assert nothing == (1 if s[0] == 0 and s[1] == 0 else 0)
    return tuple(s)


def test_each_transition_of_the_tallies_from_a_state_where_every_field_is_set(shim):
    S = (12, 1, 7, 46080)   # total_spp, captured, launches, samples: three launches' worth at 40 x 24 ... and then some
    pix = 960
    assert tally(shim, S, EMPTIED) == (0, 0, 0, 0)
    assert tally(shim, S, REPARTITIONED) == (0, 0, 7, 46080)      # samples and launches go on counting
    assert tally(shim, S, OWN_FRESH) == (0, 1, 7, 46080)          # total_spp alone
    assert tally(shim, S, REBOUND) == (0, 1, 7, 46080)            # likewise: `captured` stays
    assert tally(shim, S, LOADED, 5, pix) == (5, 0, 7, 4800)      # samples are SET, launches are not part of a checkpoint
    assert tally(shim, S, LOADED, 0, pix) == (0, 0, 7, 0)
    assert tally(shim, S, LOADED, 2 ** 24 - 1, pix) == (16777215, 0, 7, 16777215 * 960)
    assert tally(shim, S, LOADED, 2 ** 24 - 1, 2 ** 30) == (16777215, 0, 7, 16777215 << 30)   # 64-bit arithmetic
    assert tally(shim, S, UNIFORM, 0, pix, 3, 4) == (24, 1, 8, 46080 + 960 * 12)
    assert tally(shim, S, UNIFORM, 1, pix, 3, 4) == S             # a captured launch: the tallies untouched
    assert tally(shim, (12, 0, 7, 46080), UNIFORM, 1, pix, 3, 4) == (12, 1, 7, 46080)   # ... and `captured` set
    assert tally(shim, S, FRAMES, 1, pix, 4) == (12, 1, 8, 46080 + 3840)     # frames never touch total_spp
    assert tally(shim, S, FRAMES, 70, pix, 2) == (12, 1, 77, 46080 + 70 * 1920)
    assert tally(shim, S, PARTIAL, 200, 2, 4) == (12, 1, 8, 46080 + 1600)    # nor does a partial round
    assert tally(shim, (0, 0, 0, 0), UNIFORM, 0, 2 ** 31, 8, 64) == (512, 0, 1, 2 ** 40)
    # "nothing rendered yet": no direct launch and no captured one (tally() checks it after every transition above)
    assert shim.tally_apply((C.c_uint64 * 4)(0, 0, 3, 99), OWN_FRESH, 0, 0, 0, 0) == 1
    assert shim.tally_apply((C.c_uint64 * 4)(0, 1, 0, 0), REBOUND, 0, 0, 0, 0) == 0


def test_a_pt_reset_accum_then_the_calls_of_a_session(shim):
    s = tally(shim, (9, 1, 9, 9), EMPTIED)
    for op, args in ((UNIFORM, (0, 960, 2, 1)), (FRAMES, (3, 960, 1)), (PARTIAL, (128, 2, 1)), (REPARTITIONED, ()), (UNIFORM, (0, 320, 1, 1)),
                     (REBOUND, ()), (LOADED, (6, 320)), (UNIFORM, (1, 320, 1, 1)), (OWN_FRESH, ())):
        s = tally(shim, s, op, *args)
    assert s == (0, 1, 6, 1920)


EVERY_ROW = ((8, 0, 1), (0, 0, 0), (0, 3, 5), (8, 0, 0))
BANDS = ((4, 1, 3), (4, 2, 3), (4, 1, 2), (3, 1, 3), (1, 0, 2), (8, 5, 6))


def test_the_effective_partition(shim):
    out = (C.c_uint32 * 3)()
    for raw in EVERY_ROW:
        assert shim.partition_get(*raw, out) == 1 and tuple(out) == (0, 0, 1), raw   # one representation
        assert all(shim.partition_equal(*raw, *other) == 1 for other in EVERY_ROW), raw
        assert all(shim.partition_equal(*raw, *b) == 0 for b in BANDS), raw
    for a in BANDS:
        assert shim.partition_get(*a, out) == 0 and tuple(out) == a
        for b in BANDS:
            assert shim.partition_equal(*a, *b) == (1 if a == b else 0), (a, b)
    assert shim.partition_equal(4, 1, 3, 4, 2, 3) == 0
    # the normalised value names the rows the raw fields name: abi.local_rows / owned_rows are the rule's statement in Python
    for raw in EVERY_ROW + BANDS:
        shim.partition_get(*raw, out)
        for h in (1, 19, 24):
            assert abi.local_rows(h, *tuple(out)) == abi.local_rows(h, *raw), (raw, h)
            assert abi.owned_rows(h, *tuple(out)).tolist() == abi.owned_rows(h, *raw).tolist(), (raw, h)
            if raw in EVERY_ROW:
                assert abi.local_rows(h, *raw) == h


def test_the_same_walks_under_address_and_undefined_behaviour_sanitizers():
    """tests/ctx_state_main.cpp: a stand-alone program (its own main) over the same header and stand-in context, built with
    -fsanitize=address,undefined and run as a child."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "ctx_state_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(HERE, "ctx_state_main.cpp"), "-o", exe])
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and "ctx_state: ok" in out.stdout, out.stdout[-2000:]
