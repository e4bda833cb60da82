"""The wave-level dealing of work items and the look-ahead refill (csrc/pt_deal.hpp) on the CPU, through tests/deal_shim.cpp.

The dealing only schedules: which lane runs an item, and when, never changes a bit of the image, so a rendering test sees a
slip in it only as a missing or doubled pixel at some launch shape, or as a wave that never ends.  Here whole waves are run on
the CPU with the functions the kernels call — the ballot's rank against the pool, the reservation in each queue mode, the
promote / starving / wants-an-item predicates — over random item lengths (1-segment items included), items dropped at the
image's edge, all three queue modes and several waves that reach the queue's counters in different orders.  Asserted by the
simulation itself, at every step: no item number beyond the queue, no full next slot overwritten, no lane that holds a next
item without working on an item, every wave leaves with nothing in its hands on a dry queue; and by the tests: every item of
[0, n_items) decoded exactly once, within a step bound.  Then the single functions against their definitions, and the same
launches as a stand-alone program under the address and undefined-behaviour sanitizers.  CPU only."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SHARED, STATIC, GROUPED = 0, 1, 2  # PtKernelArgs.queue_static
MODES = {"shared": SHARED, "static": STATIC, "grouped": GROUPED}
ERRORS = {1: "an item number beyond the queue", 2: "a full next slot was overwritten", 3: "a lane held a next item and did not work",
          4: "the launch did not end within the step bound", 5: "a wave left with work in its hands or before the queue was dry",
          6: "a wave left reserved items behind", 7: "bad arguments"}


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(tempfile.mkdtemp(prefix="deal_"), "libdeal_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", os.path.join(HERE, "deal_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.deal_simulate.restype = C.c_int
    lib.deal_simulate.argtypes = [C.c_uint32] * 9 + [C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib.deal_rank_of.restype = C.c_uint32
    lib.deal_rank_of.argtypes = [C.c_uint64, C.c_uint32]
    lib.deal_taken.restype = C.c_uint32
    lib.deal_taken.argtypes = [C.c_uint64, C.c_uint32]
    lib.deal_grouped_base.restype = C.c_uint64
    lib.deal_grouped_base.argtypes = [C.c_uint32] * 4
    lib.deal_static_base.restype = C.c_uint64
    lib.deal_static_base.argtypes = [C.c_uint32] * 4
    lib.deal_reservation_end.restype = C.c_uint32
    lib.deal_reservation_end.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
    lib.deal_predicates.restype = C.c_int
    lib.deal_predicates.argtypes = [C.c_int] * 4
    lib.deal_plan_refill_ahead.restype = C.c_uint32
    lib.deal_plan_refill_ahead.argtypes = [C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_uint32]
    return lib


def simulate(lib, n_items, chunk, n_waves, mode, groups=0, seed=1, max_len=46, drop_percent=0, ahead=1):
    """runs one launch to its end; returns (per-item decode counts, statistics)"""
    decoded = (C.c_uint32 * max(n_items, 1))()
    stats = (C.c_uint64 * 6)()
    # every wave step moves a live lane one step on, so the steps of all waves are at most items x max_len, plus a step per
    # reservation that deals nothing and the waves' last steps; a wave takes three turns in four
    bound = 64 + 8 * (n_items * max_len + n_items // chunk + n_waves + 1)
    rc = lib.deal_simulate(n_items, chunk, n_waves, mode, groups, seed, max_len, drop_percent, ahead, bound, decoded, stats)
    assert rc == 0, "%d items, reservations of %d, %d waves, mode %d: %s" % (n_items, chunk, n_waves, mode, ERRORS.get(rc, rc))
    return list(decoded)[:n_items], dict(zip(("wave_steps", "decode_trips", "decode_lanes", "promotions", "reservations", "rounds"), stats))


def groups_for(mode, n_waves):
    """the launch plan's rule (csrc/pt_launch_plan.hpp): the largest power of two not above the wave count"""
    if mode != GROUPED:
        return 0
    g = 1
    while 2 * g <= n_waves:
        g *= 2
    return g


@pytest.mark.parametrize("mode", sorted(MODES), ids=sorted(MODES))
@pytest.mark.parametrize("chunk", [32, 64, 512])
@pytest.mark.parametrize("ahead", [1, 0], ids=["ahead", "direct"])
def test_every_item_is_decoded_exactly_once_and_every_wave_ends(shim, mode, chunk, ahead):
    """n_items 0, 1, 63, 64, 65 and the reservation size and its neighbours; one wave, a few, and more waves than reservations;
    items of exactly one step, of 1 to 3 steps with a fifth of them dropped at the image's edge, and of 1 to 46 steps; slots
    filled ahead, and lanes served directly (the launch plan's switch)"""
    for n_items in sorted({0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1}):
        for n_waves in (1, 3, 8):
            for max_len, drop in ((1, 0), (3, 20), (46, 0)):
                decoded, st = simulate(shim, n_items, chunk, n_waves, MODES[mode], groups_for(MODES[mode], n_waves),
                                       seed=chunk * 17 + n_items + max_len, max_len=max_len, drop_percent=drop, ahead=ahead)
                what = (mode, chunk, n_items, n_waves, max_len, drop, ahead)
                assert decoded == [1] * n_items, what
                assert st["decode_lanes"] == n_items, what
                assert st["promotions"] == n_items if drop == 0 else st["promotions"] <= n_items, what
                if max_len == 1 and drop == 0:  # every item is one wave step of one lane
                    assert st["wave_steps"] >= -(-n_items // (64 * n_waves)), what


@pytest.mark.parametrize("mode", sorted(MODES), ids=sorted(MODES))
def test_long_launches_with_drops(shim, mode):
    """thousands of items over a dozen waves: many reservations per wave, pools that end inside a ballot, slots that stay full
    over many steps"""
    rng = random.Random(20250 + MODES[mode])
    for _ in range(6):
        n_waves = rng.choice([2, 5, 12, 16])
        chunk = rng.choice([32, 64, 128, 512])
        n_items = rng.randrange(1000, 30000)
        max_len = rng.choice([1, 2, 7, 46])
        decoded, st = simulate(shim, n_items, chunk, n_waves, MODES[mode], groups_for(MODES[mode], n_waves), seed=rng.randrange(1 << 30),
                               max_len=max_len, drop_percent=rng.choice([0, 3, 50]), ahead=rng.choice([1, 1, 0]))
        assert decoded == [1] * n_items, (mode, n_items, chunk, n_waves, max_len)
        assert st["decode_lanes"] == n_items and st["decode_trips"] >= -(-n_items // 64)


def test_the_decode_serves_many_lanes_at_a_time(shim):
    """what the look-ahead is for, at the shape where it is certain: items of exactly one step on one wave.  Every lane uses up
    its item in every step, so whenever the decode runs every next slot is empty, and with reservations that are a multiple of
    64 and a queue of a multiple of 64 items every trip serves the whole wave — the bound is 64 lanes per trip, asserted with
    a margin of a quarter for the launch's last reservation.  (The refill it replaces served the lanes that had just run
    out; how many lanes a trip serves on a real launch is read from the measuring twins' region tallies.)"""
    decoded, st = simulate(shim, 64 * 200, 512, 1, SHARED, max_len=1)
    assert decoded == [1] * (64 * 200)
    assert st["decode_lanes"] / st["decode_trips"] >= 0.75 * 64, st


def test_lanes_served_directly_hold_nothing_back(shim):
    """the launch plan's switch off: the decode serves only lanes without an item, so an item is promoted in the step it is
    decoded in and no lane ever holds one beside the one it works on — with items of 46 steps on one wave a decode trip then
    serves few lanes (the lanes that ran out in that very step), where filling ahead serves many"""
    n = 64 * 40
    _, direct = simulate(shim, n, 512, 1, SHARED, max_len=46, ahead=0)
    _, ahead = simulate(shim, n, 512, 1, SHARED, max_len=46, ahead=1)
    assert direct["decode_lanes"] == ahead["decode_lanes"] == n
    assert direct["decode_trips"] > 2 * ahead["decode_trips"], (direct, ahead)


def test_the_launch_plan_fills_ahead_except_for_few_long_items(shim):
    """csrc/pt_launch_plan.hpp refill_ahead, on whole plans: the shapes that were measured.  Grid-walk launches are 512 threads x 3
    per CU, small-list launches 256 x 7, on 256 CUs; items = tiles x 64 x passes."""
    c2, c4, ref = 240 * 135 * 64, 128 * 128 * 64, 160 * 88 * 64
    cases = [(c2 * 64, 16, 64, 512, 3, 1, 484, 1),     # config 2, 64 passes of 16 spp: 337 items per lane
             (c2 * 64 // 8, 16, 64, 512, 3, 1, 484, 1),   # one rank's band of eight (about): 42 per lane
             (c2 * 4, 64, 4, 512, 3, 1, 10000, 0),     # config 5, 4 passes of 64 spp: 21 per lane of 64-spp items
             (c4 * 8, 64, 8, 256, 7, 0, 9, 0),         # config 4, 8 passes of 64 spp: 18 per lane
             (ref * 16, 25, 16, 256, 7, 0, 9, 1),      # the reference's scene, 16 passes of 25 spp
             (ref, 1, 1, 256, 7, 0, 9, 1),             # its single 1-spp frame
             (64, 2, 1, 512, 3, 1, 484, 1),            # one tile
             (84 * 64, 64, 1, 512, 3, 1, 484, 0)]      # 96 x 54, one pass of 64 spp: one item per lane
    for items, spp, passes, block, per_cu, walk, n_spheres, want in cases:
        assert shim.deal_plan_refill_ahead(items, spp, passes, block, per_cu, 256, walk, n_spheres) == want, (items, spp, passes)


def test_single_functions(shim):
    rng = random.Random(77)
    for _ in range(2000):
        mask = rng.getrandbits(64) & rng.getrandbits(64) if rng.random() < 0.5 else rng.getrandbits(64)
        lane = rng.randrange(64)
        assert shim.deal_rank_of(mask, lane) == bin(mask & ((1 << lane) - 1)).count("1")
        avail = rng.choice([0, 1, 5, 63, 64, 65, 512])
        assert shim.deal_taken(mask, avail) == min(bin(mask).count("1"), avail)
    assert shim.deal_rank_of((1 << 64) - 1, 63) == 63 and shim.deal_rank_of(0, 63) == 0 and shim.deal_rank_of((1 << 64) - 1, 0) == 0
    for r, groups, group, chunk in ((0, 256, 0, 64), (3, 256, 255, 64), (70000, 256, 17, 1024), (0xFFFFFFFF, 256, 255, 4096)):
        assert shim.deal_grouped_base(r, groups, group, chunk) == (r * groups + group) * chunk  # (64-bit: no wrap)
    for rnd, n_waves, wave, chunk in ((0, 6144, 0, 64), (5, 7168, 7167, 64), (0xFFFFFFFF, 7168, 7167, 4096)):
        assert shim.deal_static_base(rnd, n_waves, wave, chunk) == (rnd * n_waves + wave) * chunk
    assert shim.deal_reservation_end(0, 64, 65) == 64 and shim.deal_reservation_end(64, 64, 65) == 65
    assert shim.deal_reservation_end(0xFFFFFF00, 4096, 0xFFFFFFFF) == 0xFFFFFFFF
    # predicates: bit 0 wants an item, bit 1 starving, bit 2 promotes
    for alive in (0, 1):
        for empty in (0, 1):
            for dry in (0, 1):
                for ahead in (0, 1):
                    want = ((1 if empty and not dry and (ahead or not alive) else 0) | (2 if not alive and empty and not dry else 0) |
                            (4 if not alive and not empty else 0))
                    assert shim.deal_predicates(alive, empty, dry, ahead) == want, (alive, empty, dry, ahead)
                    assert not (want & 2) or (want & 1)  # a starving lane always wants an item: the decode it triggers serves it


def test_stand_alone_program_under_the_sanitizers():
    """tests/deal_main.cpp: a stand-alone program (its own main) over the same launches, built with
    -fsanitize=address,undefined and run as a child; nothing sanitized is loaded into this process"""
    with tempfile.TemporaryDirectory(prefix="deal_main_") as d:
        exe = os.path.join(d, "deal_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(HERE, "deal_main.cpp"), "-o", exe])
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:]
        assert "deal: ok" in out.stdout
