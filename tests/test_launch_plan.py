"""The trace launch's queue and grid policy (csrc/pt_launch_plan.hpp) on the CPU, through tests/launch_plan_shim.cpp.

The policy only schedules: the images are the same bits whatever it decides, so no rendering test can see a slip in it (a
reservation size or a dealing threshold would only show as a slower bench line).  Here every decision is pinned for the
launch shapes the project measures, on 256 CUs with the workgroup sizes and residency the committed kernel traces show
(profiles/r06_final_summary.txt: grid kernels 512 threads x 3 per CU, small and scalar list kernels 256 x 7, the LDS list
kernel 256 x 6).  The expected values were recorded from the arithmetic as it stood inline in pt_api.hip before it moved
into the header.  Then invariants over a seeded sweep, and where the dev knobs land.  CPU only."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import pytest

SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "launch_plan_shim.cpp")
KNOBS = ["coop_max", "per_cu", "queue_chunk", "grid_percent", "queue_static", "cost_feedback", "fewer_x10_1", "fewer_x10_2",
         "queue_grouped"]
FIELDS = ("queue_chunk", "queue_static", "queue_groups", "grid", "n_waves", "cost_feedback", "coop_max_live")
QUEUE_GROUPS_MAX = 256  # pt_kernel_args.h PT_QUEUE_GROUPS_MAX


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(tempfile.mkdtemp(prefix="launch_plan_"), "liblaunch_plan_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", SHIM, "-o", so])
    lib = C.CDLL(so)
    lib.launch_plan.restype = C.c_int
    lib.launch_plan.argtypes = [C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_uint32,
                                C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]
    lib.launch_list_block_threads.restype = C.c_uint32
    lib.launch_list_block_threads.argtypes = [C.c_uint64]
    return lib


def plan(lib, items, spp, passes, block, per_cu, walk, n_spheres=0, num_cus=256, knobs=None):
    mask, vals = 0, (C.c_int * len(KNOBS))()
    for k, v in (knobs or {}).items():
        mask |= 1 << KNOBS.index(k)
        vals[KNOBS.index(k)] = v
    out = (C.c_uint32 * 7)()
    assert lib.launch_plan(items, spp, passes, block, per_cu, num_cus, 1 if walk else 0, n_spheres, mask, vals, out) == 0
    return tuple(out)


# tiles of 8 x 8 pixels: config 2 / 5 at 1920x1080, config 3 at 3840x2160, config 4 at 1024x1024, the reference at 1280x702
C2, C3, C4, REF = 240 * 135, 480 * 270, 128 * 128, 160 * 88
# (name, launch, (queue_chunk, queue_static, queue_groups, grid, n_waves, cost_feedback, coop_max_live)); items = tiles x 64 x
# passes.  config 3 / 5: tools/config_sweep.py's launches; pt_tune's timing launches on config 2; rank 0 of an 8-rank config 2
# run owns 136 rows of 4-row bands (17 tile rows); the reference's frames through the small-list kernel (9 spheres), its
# groups of one-sample frames as one launch of a pass per frame, and the cost-order probe (one pass at the frame's spp).
PINNED = [
    ('config2_frame_64x16', {'items': 132710400, 'spp': 16, 'passes': 64, 'block': 512, 'per_cu': 3, 'walk': True}, (512, 0, 0, 768, 6144, 1, 0)),
    ('config2_frame_64x16_lds_list', {'items': 132710400, 'spp': 16, 'passes': 64, 'block': 256, 'per_cu': 6, 'walk': False, 'n_spheres': 484}, (512, 0, 0, 1536, 6144, 1, 12)),
    ('config2_frame_64x16_scalar_list', {'items': 132710400, 'spp': 16, 'passes': 64, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 484}, (512, 0, 0, 1792, 7168, 1, 12)),
    ('config3_sweep_8x64', {'items': 66355200, 'spp': 64, 'passes': 8, 'block': 512, 'per_cu': 3, 'walk': True}, (128, 0, 0, 768, 6144, 1, 0)),
    ('config5_sweep_4x64', {'items': 8294400, 'spp': 64, 'passes': 4, 'block': 512, 'per_cu': 3, 'walk': True}, (64, 0, 0, 768, 6144, 1, 0)),
    ('config4_small_64x16', {'items': 67108864, 'spp': 16, 'passes': 64, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, (128, 0, 0, 1792, 7168, 1, 6)),
    ('config2_tune_1x16', {'items': 2073600, 'spp': 16, 'passes': 1, 'block': 512, 'per_cu': 3, 'walk': True}, (64, 2, 256, 768, 6144, 1, 0)),
    ('config2_tune_2x16', {'items': 4147200, 'spp': 16, 'passes': 2, 'block': 512, 'per_cu': 3, 'walk': True}, (64, 2, 256, 768, 6144, 1, 0)),
    ('config2_tune_4x16', {'items': 8294400, 'spp': 16, 'passes': 4, 'block': 512, 'per_cu': 3, 'walk': True}, (64, 2, 256, 768, 6144, 1, 0)),
    ('config2_rank0_of_8_64x16', {'items': 16711680, 'spp': 16, 'passes': 64, 'block': 512, 'per_cu': 3, 'walk': True}, (128, 0, 0, 768, 6144, 1, 0)),
    ('reference_frame_1spp', {'items': 901120, 'spp': 1, 'passes': 1, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, (64, 1, 0, 768, 3072, 0, 6)),
    ('reference_frame_2spp', {'items': 901120, 'spp': 2, 'passes': 1, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, (64, 1, 0, 1024, 4096, 0, 6)),
    ('reference_frame_4spp', {'items': 901120, 'spp': 4, 'passes': 1, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, (64, 1, 0, 1792, 7168, 0, 6)),
    ('reference_frame_25spp', {'items': 901120, 'spp': 25, 'passes': 1, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, (64, 2, 256, 1792, 7168, 1, 6)),
    ('reference_group_64x1spp', {'items': 57671680, 'spp': 1, 'passes': 64, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, (64, 2, 256, 1792, 7168, 0, 6)),
    ('reference_group_16x1spp', {'items': 14417920, 'spp': 1, 'passes': 16, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, (64, 2, 256, 1792, 7168, 0, 6)),
    ('reference_group_4x1spp', {'items': 3604480, 'spp': 1, 'passes': 4, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, (64, 1, 0, 1792, 7168, 0, 6)),
    ('reference_cost_probe_8spp', {'items': 901120, 'spp': 8, 'passes': 1, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, (64, 1, 0, 1792, 7168, 1, 6)),
]


@pytest.mark.parametrize("name,launch,want", PINNED, ids=[p[0] for p in PINNED])
def test_pinned_decisions(shim, name, launch, want):
    assert dict(zip(FIELDS, plan(shim, **launch))) == dict(zip(FIELDS, want))


def test_list_kernels_workgroup_size(shim):
    # 256 threads while the list's LDS copy leaves room for several workgroups, 1024 above 40 KiB
    for lds, want in ((0, 256), (208, 256), (40 * 1024, 256), (40 * 1024 + 16, 1024), (163776, 1024)):
        assert shim.launch_list_block_threads(lds) == want


def sweep(seed=1234, n=4000):
    rng = random.Random(seed)
    for _ in range(n):
        tiles = rng.choice([1, 17, 240 * 17, REF, C2, C4, C3, rng.randint(1, 200000)])
        passes = rng.choice([1, 2, 3, 4, 8, 16, 64, 256])
        yield dict(items=tiles * 64 * passes, spp=rng.choice([1, 2, 3, 4, 8, 16, 25, 64, 1000]), passes=passes,
                   block=rng.choice([256, 512, 1024]), per_cu=rng.randint(0, 8), walk=rng.random() < 0.5,
                   n_spheres=rng.randint(0, 20000), num_cus=rng.choice([1, 8, 32, 80, 256, 304]))


def check_invariants(lib):
    for launch in sweep():
        chunk, deal, groups, grid, n_waves, cost_feedback, coop = plan(lib, **launch)
        assert grid >= 1, launch
        assert grid <= launch["num_cus"] * max(launch["per_cu"], 1), launch  # never more workgroups than are resident
        assert n_waves == grid * launch["block"] // 64, launch
        assert deal in (0, 1, 2), launch
        if deal:  # a static deal (grouped or not) reserves one tile's 64 items
            assert chunk == 64, launch
        else:
            assert 32 <= chunk <= 1024, launch
        if deal == 2:
            assert groups & (groups - 1) == 0 and 1 <= groups <= min(launch["num_cus"], QUEUE_GROUPS_MAX, n_waves), launch
        else:
            assert groups == 0, launch
        assert cost_feedback in (0, 1) and (coop == 0 if launch["walk"] else coop <= 16), launch


def test_invariants_over_a_seeded_sweep(shim):
    check_invariants(shim)


# overrides of the dev build (pt_api.hip read_launch_knobs), each where the arithmetic always applied it: PT_QUEUE_CHUNK
# before the static deal's 64 overwrites it, PT_GRID_PERCENT before n_waves and the dealing rule see the grid,
# PT_COST_FEEDBACK before a statically dealt one-sample launch drops it, out-of-range values ignored
KNOB_CASES = [
    ('chunk_over_shared', {'items': 132710400, 'spp': 16, 'passes': 64, 'block': 512, 'per_cu': 3, 'walk': True}, {'queue_chunk': 300}, (300, 0, 0, 768, 6144, 1, 0)),
    ('chunk_under_static', {'items': 901120, 'spp': 4, 'passes': 1, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, {'queue_chunk': 300}, (64, 1, 0, 1792, 7168, 0, 6)),
    ('chunk_out_of_range', {'items': 132710400, 'spp': 16, 'passes': 64, 'block': 512, 'per_cu': 3, 'walk': True}, {'queue_chunk': 5000}, (512, 0, 0, 768, 6144, 1, 0)),
    ('grid_percent_50', {'items': 132710400, 'spp': 16, 'passes': 64, 'block': 512, 'per_cu': 3, 'walk': True}, {'grid_percent': 50}, (512, 0, 0, 384, 3072, 1, 0)),
    ('grid_percent_50_static', {'items': 14417920, 'spp': 1, 'passes': 16, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, {'grid_percent': 50}, (64, 2, 256, 896, 3584, 0, 6)),
    ('grid_percent_0', {'items': 132710400, 'spp': 16, 'passes': 64, 'block': 512, 'per_cu': 3, 'walk': True}, {'grid_percent': 0}, (512, 0, 0, 1, 8, 1, 0)),
    ('grouped_off', {'items': 57671680, 'spp': 1, 'passes': 64, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, {'queue_grouped': 0}, (64, 1, 0, 1792, 7168, 0, 6)),
    ('grouped_on', {'items': 901120, 'spp': 1, 'passes': 1, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, {'queue_grouped': 1}, (64, 2, 256, 768, 3072, 0, 6)),
    ('static_off', {'items': 901120, 'spp': 1, 'passes': 1, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, {'queue_static': 0}, (1024, 0, 0, 1792, 7168, 0, 6)),
    ('static_on', {'items': 132710400, 'spp': 16, 'passes': 64, 'block': 512, 'per_cu': 3, 'walk': True}, {'queue_static': 1}, (64, 2, 256, 768, 6144, 1, 0)),
    ('cost_feedback_on_static_1spp', {'items': 3604480, 'spp': 1, 'passes': 4, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, {'cost_feedback': 1}, (64, 1, 0, 1792, 7168, 0, 6)),
    ('cost_feedback_on_1pass', {'items': 2073600, 'spp': 4, 'passes': 1, 'block': 512, 'per_cu': 3, 'walk': True}, {'queue_static': 0, 'cost_feedback': 1}, (512, 0, 0, 768, 6144, 1, 0)),
    ('cost_feedback_off', {'items': 132710400, 'spp': 16, 'passes': 64, 'block': 512, 'per_cu': 3, 'walk': True}, {'cost_feedback': 0}, (512, 0, 0, 768, 6144, 0, 0)),
    ('per_cu_2', {'items': 132710400, 'spp': 16, 'passes': 64, 'block': 512, 'per_cu': 3, 'walk': True}, {'per_cu': 2}, (512, 0, 0, 512, 4096, 1, 0)),
    ('per_cu_out_of_range', {'items': 132710400, 'spp': 16, 'passes': 64, 'block': 512, 'per_cu': 3, 'walk': True}, {'per_cu': 40}, (512, 0, 0, 768, 6144, 1, 0)),
    ('fewer_x10_1', {'items': 901120, 'spp': 1, 'passes': 1, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, {'fewer_x10_1': 60}, (64, 1, 0, 512, 2048, 0, 6)),
    ('fewer_x10_2', {'items': 901120, 'spp': 2, 'passes': 1, 'block': 256, 'per_cu': 7, 'walk': False, 'n_spheres': 9}, {'fewer_x10_2': 50, 'fewer_x10_1': 90}, (64, 1, 0, 768, 3072, 0, 6)),
    ('coop_max_list', {'items': 132710400, 'spp': 16, 'passes': 64, 'block': 256, 'per_cu': 6, 'walk': False, 'n_spheres': 484}, {'coop_max': 3}, (512, 0, 0, 1536, 6144, 1, 3)),
    ('coop_max_walk', {'items': 132710400, 'spp': 16, 'passes': 64, 'block': 512, 'per_cu': 3, 'walk': True}, {'coop_max': 3}, (512, 0, 0, 768, 6144, 1, 0)),
]


@pytest.mark.parametrize("name,launch,knobs,want", KNOB_CASES, ids=[k[0] for k in KNOB_CASES])
def test_knob_placement(shim, name, launch, knobs, want):
    assert dict(zip(FIELDS, plan(shim, knobs=knobs, **launch))) == dict(zip(FIELDS, want))
