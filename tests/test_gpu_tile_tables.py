"""The work queue's two tile-table kernels on caller data: pt_tile_order_kernel and pt_partition_order_kernel, launched as the
product launches them (one workgroup of 1024 threads) through the developer entry points pt_debug_tile_order and
pt_debug_partition_order (include/ptrace_dev.h), against tests/tile_tables_ref.py (held to its properties by
tests/test_tile_tables_ref.py without a GPU).

In the product the order kernel's output can only be seen as `base` of pt_adaptive_tiles and the costs it sorted cannot be read;
no scene the suite renders has more than a few hundred tiles.  Here a thread owns several tiles: above 1024 tiles the order
kernel's loops make a second trip (`i += 1024`) and the partition kernel's runs are per = ceil(n / 1024) positions long, the last
one short when n % per != 0.  1280x702 has 14 080 tiles, 1920x1080 32 400, the 4K frame 129 600.

Everything is compared exactly.  The entry points fill their outputs with 0xFF bytes first, so an entry a kernel never wrote
reads 0xFFFFFFFF and is no tile."""
import numpy as np
import pytest

import error_ref as E
import tile_tables_ref as T
from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd._lib import _u32p
from ray_tracer_webgl_amd.tracer import PathTracer

pytestmark = pytest.mark.gpu

U = np.uint32


def _ptr(a):
    return a.ctypes.data_as(_u32p)


def tile_order(t, cost):
    """(order, cost as the kernel left it) of pt_tile_order_kernel on `cost`."""
    cost = np.ascontiguousarray(cost, dtype=U)
    order, cost_out = np.empty(len(cost), U), np.empty(len(cost), U)
    t._check(t.lib.pt_debug_tile_order(t._ctx, _ptr(cost), len(cost), _ptr(order), _ptr(cost_out)))
    return order, cost_out


def partition_order(t, order, flags):
    """(part, base) of pt_partition_order_kernel on the table `order` and the per-tile `flags`."""
    order, flags = np.ascontiguousarray(order, dtype=U), np.ascontiguousarray(flags, dtype=U)
    part, base = np.empty(len(order), U), np.empty(len(order), U)
    t._check(t.lib.pt_debug_partition_order(t._ctx, _ptr(order), _ptr(flags), len(order), _ptr(part), _ptr(base)))
    return part, base


@pytest.fixture(scope="module")
def ctx():
    """One context for every case: 64x36 with the scene and uniforms the last test renders."""
    spheres, p = E.estimate_scene(64, 36, spp=4)
    t = PathTracer(p.width, p.height)
    t.set_spheres(spheres)
    t.set_params(p)
    yield t, spheres, p
    t.close()


@pytest.mark.parametrize("n", T.SIZES)
def test_tile_order_kernel_against_the_contract(ctx, n):
    """Every cost class of tile_tables_ref.cost_classes: the order is a permutation, its buckets do not decrease (heaviest tiles
    first), each bucket's slice holds that bucket's tiles, the costs are cleared; all costs zero give the identity."""
    t = ctx[0]
    for name, cost in T.cost_classes(n):
        before = cost.copy()
        order, cost_out = tile_order(t, cost)
        assert cost.tobytes() == before.tobytes()
        fault = T.order_fault(cost, order, cost_out)
        assert fault == "", "%d tiles, %s: %s" % (n, name, fault)


@pytest.mark.parametrize("n", T.SIZES)
def test_partition_order_kernel_against_the_restatement(ctx, n):
    """Every flag class of tile_tables_ref.flag_classes on the identity and on a random permutation as `order`:
    part == partition(order, flags) and base == order, entry for entry."""
    t = ctx[0]
    rng = np.random.default_rng(7000 + n)
    for kind, order in (("identity", np.arange(n, dtype=U)), ("permutation", rng.permutation(n).astype(U))):
        for name, flags in T.flag_classes(order):
            part, base = partition_order(t, order, flags)
            what = "%d tiles, %s, %s" % (n, kind, name)
            fault = T.table_fault(base, order, what + ", base") or T.table_fault(part, T.partition(order, flags), what + ", part")
            assert fault == "", fault


def test_the_order_kernel_feeds_the_partition_kernel(ctx):
    """The product's sequence at 1920x1080's tile count: the order of random costs, partitioned by random flags."""
    t = ctx[0]
    n = 32400
    rng = np.random.default_rng(11)
    cost = rng.integers(0, 401, n).astype(U)
    order, cost_out = tile_order(t, cost)
    assert T.order_fault(cost, order, cost_out) == ""
    flags = (rng.random(n) < 0.5).astype(U)
    part, base = partition_order(t, order, flags)
    fault = T.table_fault(base, order, "base") or T.table_fault(part, T.partition(order, flags), "part")
    assert fault == "", fault


def test_entry_points_refuse_nothing_to_do_and_disturb_nothing(ctx, ora):
    """n == 0 and NULL pointers are PT_ERR_INVALID.  After all of the above — and one more call of each entry point here — an
    ordinary pt_render_passes(1) on the same context equals the oracle's pass: the calls touched neither the context's order
    and costs nor its launch state."""
    t, spheres, p = ctx
    a = np.arange(8, dtype=U)
    assert t.lib.pt_debug_tile_order(t._ctx, _ptr(a), 0, _ptr(a), _ptr(a)) == abi.PT_ERR_INVALID
    assert t.lib.pt_debug_partition_order(t._ctx, _ptr(a), _ptr(a), 0, _ptr(a), _ptr(a)) == abi.PT_ERR_INVALID
    for k in range(3):
        args = [_ptr(a), 8, _ptr(a), _ptr(a)]
        args[(0, 2, 3)[k]] = None
        assert t.lib.pt_debug_tile_order(t._ctx, *args) == abi.PT_ERR_INVALID
    for k in range(4):
        args = [_ptr(a), _ptr(a), 8, _ptr(a), _ptr(a)]
        args[(0, 1, 3, 4)[k]] = None
        assert t.lib.pt_debug_partition_order(t._ctx, *args) == abi.PT_ERR_INVALID
    assert a.tolist() == list(range(8))
    cost = np.random.default_rng(12).integers(0, 401, 2049).astype(U)
    order, cost_out = tile_order(t, cost)
    assert T.order_fault(cost, order, cost_out) == ""
    part, base = partition_order(t, order, cost & 1)
    assert part.tolist() == T.partition(order, cost & 1).tolist() and base.tolist() == order.tolist()
    t.render_passes(1)
    ref, seg = ora.render(spheres, p, 1)
    got = t.accum()
    assert E.same_floats(got, ref), E.first_difference(got, ref)
    assert t.stats().segments == seg
