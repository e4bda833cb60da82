"""The tile-table kernels' restatement (tests/tile_tables_ref.py) without a GPU.

  (1) The surface: pt_debug_tile_order and pt_debug_partition_order are exported, declared in include/ptrace_dev.h (not in the
      versioned header) and in _lib.DEV_SIGNATURES with the header's argument counts; both refuse a missing context.
  (2) buckets(): monotone in the cost, hand-computed lists, the maxima 1, 2^24 + 1 and 2^32 - 1, and the fact that the heaviest
      tile need not land in bucket 0.
  (3) order_fault() accepts every order a counting sort may produce and names what is wrong with one it may not.
  (4) last_run() and the shared inputs.
"""
import os
import re

import numpy as np

import adaptive_ref as A
import tile_tables_ref as T
from ray_tracer_webgl_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pt_debug_tile_order", "pt_debug_partition_order")
U = np.uint32


# ------------------------------------------------------------------------------------------------ (1) the surface
def test_the_two_entry_points_are_exported_and_declared_as_developer_diagnostics(lib):
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", path)).read(), flags=re.S)
    dev, public = strip("ptrace_dev.h"), strip("ptrace.h")
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in public and name not in _lib.SIGNATURES and name not in _lib.ADDED_WITHIN_ABI_5, name
        h = re.search(r"\b%s\s*\(([^)]*)\)" % name, dev)
        assert h, name
        assert len([a for a in h.group(1).split(",") if a.strip()]) == len(_lib.DEV_SIGNATURES[name][1]), name
        fn = getattr(lib, name)
        assert fn.restype is _lib.DEV_SIGNATURES[name][0] and list(fn.argtypes) == _lib.DEV_SIGNATURES[name][1]
    assert lib.pt_abi_version() == 5 == abi.PT_ABI_VERSION
    a = np.zeros(4, U)
    p = a.ctypes.data_as(_lib._u32p)
    assert lib.pt_debug_tile_order(None, p, 4, p, p) == abi.PT_ERR_INVALID
    assert lib.pt_debug_partition_order(None, p, p, 4, p, p) == abi.PT_ERR_INVALID


# ------------------------------------------------------------------------------------------------ (2) buckets
def test_buckets_by_hand():
    """max 4: scale = 255.75, the products 0, 255.75, 511.5, 767.25, 1023 truncate to 0, 255, 511, 767, 1023.
    max 3: scale = 341, products 1023, 682, 341, 0.  max 1: scale = 1023."""
    assert T.buckets([0, 1, 2, 3, 4]).tolist() == [1023, 768, 512, 256, 0]
    assert T.buckets([3, 2, 1, 0]).tolist() == [0, 341, 682, 1023]
    assert T.buckets([0, 1, 1, 0]).tolist() == [1023, 0, 0, 1023]
    assert T.buckets([9]).tolist() == [0] and T.buckets([1]).tolist() == [0]
    assert T.buckets([0, 0, 0]).tolist() == [0, 0, 0] and T.buckets([0]).tolist() == [0]
    assert T.buckets([7] * 5).tolist() == [0] * 5
    assert T.buckets(np.zeros(0, U)).shape == (0,)
    assert T.buckets([1, 2]).dtype == U


def test_buckets_at_the_maxima_1_2_24_plus_1_and_2_32_minus_1():
    """2^24 + 1 is no float32: it rounds (to even) to 2^24, scale = 1023 / 2^24 exactly.  16 777 215 * scale = 1023 - 1023 / 2^24,
    whose nearest float32 is 1023 - 2^-14: bucket 1.  2^32 - 1 rounds to 2^32, scale = 1023 / 2^32; a cost of 2^32 - 129 rounds
    to 2^32 - 256 and its product again to 1023 - 2^-14."""
    assert T.buckets([1, 0]).tolist() == [0, 1023]
    assert T.buckets([16777217, 16777216, 16777215, 8388608, 1, 0]).tolist() == [0, 0, 1, 512, 1023, 1023]
    assert T.buckets([0xFFFFFFFF, 0xFFFFFFFF - 127, 0xFFFFFFFF - 128, 1 << 31, 1 << 22, 400, 1, 0]).tolist() == [0, 0, 1, 512, 1023, 1023, 1023, 1023]
    # ... each of them alone is the maximum and heads the table
    for mx in (1, (1 << 24) + 1, (1 << 32) - 1):
        assert T.buckets([mx]).tolist() == [0]


def test_the_heaviest_tile_need_not_land_in_bucket_0():
    """f32(max) * (1023 / f32(max)) rounds below 1023 for 678 of the maxima 1..4999: the heaviest tile is then alone at the head
    of bucket 1 and bucket 0 is empty.  Nothing may assert bucket 0 for it; what holds is that no tile lies in a lower bucket."""
    first = np.array([T.buckets([m])[0] for m in range(1, 5000)])
    assert set(first.tolist()) == {0, 1} and int((first == 1).sum()) == 678
    rng = np.random.default_rng(3)
    for mx in (3, 41, 400, 4999, 70001, (1 << 24) + 1, (1 << 32) - 1):
        c = rng.integers(0, mx + 1, 500, dtype=np.uint64).astype(U)
        c[7] = mx
        b = T.buckets(c)
        assert b[7] == b.min() and b.max() <= 1023


def test_buckets_are_monotone_in_the_cost():
    """a >= b implies bucket(a) <= bucket(b), whatever the maximum: a float32 conversion, a product with a positive scale and a
    truncation are each monotone."""
    rng = np.random.default_rng(4)
    for mx in (1, 2, 3, 400, 1023, 1024, 1025, 4999, 123457, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 31) + 12345, (1 << 32) - 1):
        c = np.unique(np.concatenate([rng.integers(0, mx + 1, 4000, dtype=np.uint64), [0, mx, mx // 2, max(mx - 1, 0)],
                                      np.minimum(mx, np.arange(0, 2000, dtype=np.uint64))])).astype(U)
        b = T.buckets(c).astype(np.int64)
        assert c[-1] == mx and np.all(np.diff(b) <= 0), mx
        assert b[0] == 1023 and b[-1] in (0, 1), mx


# ------------------------------------------------------------------------------------------------ (3) the contract
def _some_counting_sort(cost, rng):
    """An order the kernel may produce: buckets ascending, the tiles of a bucket in any order."""
    b = T.buckets(cost)
    shuffled = rng.permutation(len(cost)).astype(U)
    return shuffled[np.argsort(b[shuffled], kind="stable")]


def test_order_fault_accepts_what_the_kernel_may_produce_and_names_what_it_may_not():
    rng = np.random.default_rng(5)
    for n in (1, 2, 64, 1025, 2049):
        for name, cost in T.cost_classes(n):
            zeros = np.zeros(n, U)
            if not cost.any():
                assert T.order_fault(cost, np.arange(n, dtype=U), zeros) == "", (n, name)
                if n > 1:
                    assert "identity" in T.order_fault(cost, np.arange(n, dtype=U)[::-1], zeros)
                continue
            order = _some_counting_sort(cost, rng)
            assert T.order_fault(cost, order, zeros) == "", (n, name)
            assert "not cleared" in T.order_fault(cost, order, cost), (n, name)
            bad = order.copy()
            bad[-1] = T.UNWRITTEN
            assert "name no tile" in T.order_fault(cost, bad, zeros), (n, name)
            if n > 1:
                bad = order.copy()
                bad[0] = bad[1]
                assert "no permutation" in T.order_fault(cost, bad, zeros), (n, name)
                b = T.buckets(cost)[order]
                if b[0] != b[-1]:
                    bad = order.copy()
                    bad[0], bad[-1] = order[-1], order[0]
                    assert "buckets decrease" in T.order_fault(cost, bad, zeros), (n, name)
    assert "shapes" in T.order_fault(np.ones(4, U), np.arange(3, dtype=U), np.zeros(4, U))


def test_canonical_form_is_the_stable_sort_by_bucket():
    rng = np.random.default_rng(6)
    cost = rng.integers(0, 401, 3000).astype(U)
    b = T.buckets(cost)
    want = np.argsort(b, kind="stable").astype(U)
    for _ in range(3):
        assert T.canonical(_some_counting_sort(cost, rng), b).tolist() == want.tolist()
    assert np.all(np.diff(cost[want].astype(np.int64))[np.diff(b[want].astype(np.int64)) > 0] < 0)   # heavier buckets first


# ------------------------------------------------------------------------------------------------ (4) runs and inputs
def test_last_run():
    """per = ceil(n / 1024); 1056 tiles: 528 threads own two positions each and 496 own none."""
    assert T.last_run(1) == (0, 1) and T.last_run(1024) == (1023, 1024)
    assert T.last_run(1025) == (1024, 1025)        # per = 2, the 513th run is short
    assert T.last_run(1056) == (1054, 1056)
    assert T.last_run(2049) == (2046, 2049)        # per = 3, 683 full runs
    assert T.last_run(16512) == (16507, 16512)     # per = 17: 971 full runs and one of 5
    assert T.last_run(129600) == (129540, 129600)  # per = 127: 1020 full runs and one of 60
    for n in T.SIZES:
        per = (n + 1023) // 1024
        lo, hi = T.last_run(n)
        assert lo % per == 0 and 0 < hi - lo <= per and hi == n and lo // per < 1024


def test_shared_inputs_hold_what_their_names_say():
    for n in T.SIZES:
        classes = dict(T.cost_classes(n))
        assert all(c.dtype == U and c.shape == (n,) for c in classes.values())
        assert ("one non-zero at first index of the second trip" in classes) == (n > 1024)
        assert classes["one cost of 2^32 - 1"].max() == 0xFFFFFFFF
        assert int((classes["many ties at the maximum"] == 400).sum()) >= min(n, 2) - 1
        if n >= 3:
            assert set(classes["around 2^24"].tolist()) == set(T.AROUND_2_24.tolist())
        rng = np.random.default_rng(n)
        for order in (np.arange(n, dtype=U), rng.permutation(n).astype(U)):
            flags = dict(T.flag_classes(order))
            assert all(f.dtype == U and f.shape == (n,) for f in flags.values())
            assert not flags["none set"].any() and flags["all set"].all()
            assert np.flatnonzero(flags["only the first position"]).tolist() == [order[0]]
            assert np.flatnonzero(flags["only the last position"]).tolist() == [order[-1]]
            lo, hi = T.last_run(n)
            assert sorted(np.flatnonzero(flags["only the last thread's run"]).tolist()) == sorted(order[lo:hi].tolist())
            part = T.partition(order, flags["alternating positions"])
            assert part.tolist() == order[1::2].tolist() + order[0::2].tolist()
    assert T.partition is A.partition
