"""A plain restatement of the work queue's two tile-table kernels — pt_tile_order_kernel (csrc/pt_kernels.hip) and
pt_partition_order_kernel (csrc/pt_kernels_error.hip) — and the inputs their tests share (tests/test_tile_tables_ref.py on the
CPU, tests/test_gpu_tile_tables.py on the device through pt_debug_tile_order / pt_debug_partition_order).

TEST INFRASTRUCTURE ONLY.

    the order kernel: mx = max cost; all zero -> the identity.  Else, in float32, one IEEE operation per statement (the library
    is built with -ffp-contract=off, uint32 -> float32 rounds to nearest even like numpy's astype):
        scale = f32(1023) / f32(mx)
        p = f32(cost) * scale;  b = 1023 - uint32(p)  (truncation; modulo 2^32);  b > 1023 -> 0
    a 1024-bucket counting sort by b follows, so heavy tiles come first; WHERE a tile lands inside its bucket is decided by
    atomics and is not specified.  The costs are cleared afterwards.  The heaviest tile need not land in bucket 0: for many
    maxima f32(mx) * scale rounds below 1023 and it lands in bucket 1.

    the partition kernel: adaptive_ref.partition — the tiles of `order` whose flag is set, in their order, then the others in
    theirs; `base` receives `order` as it was.  Thread t of 1024 owns the positions [t per, min(n, t per + per)),
    per = ceil(n / 1024): last_run(n) is the last non-empty of those runs.
"""
import numpy as np

from adaptive_ref import partition  # noqa: F401  (the partition kernel's restatement: reused, not restated again)

F = np.float32
THREADS = 1024          # both kernels are one workgroup of this many threads
UNWRITTEN = 0xFFFFFFFF  # what the developer entry points fill their output buffers with before the launch


def buckets(cost):
    """The bucket of every tile, uint32 in 0..1023; all costs zero: every tile in bucket 0 (the kernel sorts nothing then)."""
    cost = np.ascontiguousarray(cost, dtype=np.uint32)
    mx = cost.max() if cost.size else np.uint32(0)
    if mx == 0:
        return np.zeros(cost.shape, np.uint32)
    scale = F(1023.0) / np.uint32(mx).astype(np.float32)
    p = cost.astype(np.float32) * scale
    b = np.uint32(1023) - p.astype(np.uint32)      # (uint32 arithmetic: wraps like the kernel's)
    return np.where(b > np.uint32(1023), np.uint32(0), b).astype(np.uint32)


def canonical(order, b):
    """`order` with the tiles of every bucket in ascending tile number: what is specified of a result."""
    order = np.ascontiguousarray(order, dtype=np.uint32)
    return order[np.lexsort((order, b[order]))]


def order_fault(cost, order, cost_out):
    """What is wrong with a result of the order kernel, "" if nothing: `order` is a permutation of 0..n-1, buckets(cost)[order]
    does not decrease, each bucket's slice of `order` holds exactly that bucket's tiles, cost_out is all zero; all costs zero:
    `order` is the identity."""
    cost = np.ascontiguousarray(cost, dtype=np.uint32)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    cost_out = np.ascontiguousarray(cost_out, dtype=np.uint32)
    n = len(cost)
    if order.shape != (n,) or cost_out.shape != (n,):
        return "shapes %s and %s for %d tiles" % (order.shape, cost_out.shape, n)
    bad = np.flatnonzero(cost_out)
    if len(bad):
        return "%d costs not cleared, first cost_out[%d] = 0x%08x" % (len(bad), bad[0], cost_out[bad[0]])
    if not cost.any():
        bad = np.flatnonzero(order != np.arange(n, dtype=np.uint32))
        return "all costs zero, %d entries off the identity, first order[%d] = 0x%08x" % (len(bad), bad[0], order[bad[0]]) if len(bad) else ""
    bad = np.flatnonzero(order >= n)
    if len(bad):
        return "%d entries name no tile, first order[%d] = 0x%08x" % (len(bad), bad[0], order[bad[0]])
    seen = np.bincount(order, minlength=n)
    bad = np.flatnonzero(seen != 1)
    if len(bad):
        return "no permutation: %d tiles missing or repeated, first tile %d (%d times)" % (len(bad), bad[0], seen[bad[0]])
    b = buckets(cost)
    bo = b[order].astype(np.int64)
    bad = np.flatnonzero(np.diff(bo) < 0)
    if len(bad):
        i = bad[0]
        return "buckets decrease at order[%d], order[%d]: tiles %d, %d in buckets %d, %d" % (i, i + 1, order[i], order[i + 1], bo[i], bo[i + 1])
    want = np.argsort(b, kind="stable").astype(np.uint32)
    bad = np.flatnonzero(canonical(order, b) != want)
    if len(bad):
        return "a bucket's slice does not hold its tiles, first at position %d" % bad[0]
    return ""


def last_run(n):
    """(lo, hi): the positions of the last non-empty run of the partition kernel; shorter than `per` when n % per != 0."""
    per = (n + THREADS - 1) // THREADS
    t = (n + per - 1) // per - 1
    return t * per, n


def table_fault(got, want, what):
    """Two tile tables entry for entry: "" or the first differing index."""
    got, want = np.ascontiguousarray(got, dtype=np.uint32), np.ascontiguousarray(want, dtype=np.uint32)
    if got.shape != want.shape:
        return "%s: shapes %s vs %s" % (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    return "%s: %d of %d entries differ, first [%d] = 0x%08x vs %d" % (what, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]]) if len(bad) else ""


# ------------------------------------------------------------------------------------------------ inputs
# 1 and 2; one tile per wave; around one tile per thread; around two (per = 2 starts at 1025); the second trip of the tile
# kernels' launch (16 385 and up), 1920x1080's tiles, the 4K frame's
SIZES = (1, 2, 64, 1023, 1024, 1025, 2047, 2048, 2049, 16512, 32400, 129600)
AROUND_2_24 = np.array([16777215, 16777216, 16777217], np.uint32)


def cost_classes(n, seed=0):
    """[(name, uint32 costs)] for n tiles."""
    rng = np.random.default_rng(1000 + seed + n)
    out = [("all zero", np.zeros(n, np.uint32)), ("all equal", np.full(n, 7, np.uint32))]
    for name, i in (("index 0", 0), ("index n - 1", n - 1), ("first index of the second trip", THREADS)):
        if i < n:
            c = np.zeros(n, np.uint32)
            c[i] = 5
            out.append(("one non-zero at " + name, c))
    up = np.arange(1, n + 1, dtype=np.uint32)
    out += [("ascending", up), ("descending", up[::-1].copy())]
    out.append(("random in [0, 400]", rng.integers(0, 401, n).astype(np.uint32)))
    ties = rng.integers(0, 401, n).astype(np.uint32)
    ties[rng.random(n) < 0.3] = 400
    ties[rng.integers(0, n)] = 400
    out.append(("many ties at the maximum", ties))
    big = rng.integers(0, 401, n).astype(np.uint32)
    big[rng.integers(0, n)] = 0xFFFFFFFF
    out.append(("one cost of 2^32 - 1", big))
    near = rng.choice(AROUND_2_24, n)
    near[:min(3, n)] = AROUND_2_24[:min(3, n)]
    out.append(("around 2^24", near.astype(np.uint32)))
    return out


def flag_classes(order, seed=0):
    """[(name, uint32 flags per TILE)] for the table `order` (a permutation); a set flag is any non-zero word."""
    order = np.asarray(order, np.uint32)
    n = len(order)
    rng = np.random.default_rng(2000 + seed + n)
    word = np.array([1, 2, 0x80000000, 0xFFFFFFFF], np.uint32)

    def at(positions):
        f = np.zeros(n, np.uint32)
        f[order[positions]] = word[np.arange(len(order[positions])) % 4]
        return f

    every = np.arange(n)
    lo, hi = last_run(n)
    return [("none set", np.zeros(n, np.uint32)), ("all set", at(every)), ("only the first position", at(every[:1])),
            ("only the last position", at(every[-1:])), ("alternating positions", at(every[1::2])),
            ("random at 0.1", at(every[rng.random(n) < 0.1])), ("random at 0.9", at(every[rng.random(n) < 0.9])),
            ("only the last thread's run", at(every[lo:hi]))]
