"""The context's buffer sets (csrc/pt_buffers.hpp: which buffers an option owns, how they are sized for a row partition, what a
failed allocation leaves) on the CPU, through tests/buffers_shim.cpp: the header compiled with g++ -Wall -Werror against a stand-in
allocator (malloc / free, with a counter that makes the k-th allocation fail).  Every buffer's size against a table stated here,
the fresh flags, the stage buffer's lifetime, the planes' index cap, and a refused allocation at every k of every transition;
then the stand-alone program tests/buffers_main.cpp under the address and undefined-behaviour sanitizers, run as a child.  CPU
only; nothing sanitized is loaded into this process."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FRAME, ESTIMATE, FEATURES, QUERIES, HISTORY = range(5)
SETS = (FRAME, ESTIMATE, FEATURES, QUERIES, HISTORY)
PLANES = 4  # PT_FEAT_PLANES
# every buffer in the shim's order: (name, its set, its bit among the set's fresh flags)
BUFFERS = (("own_accum", FRAME, 1), ("slab", FRAME, 2), ("tile_cost", FRAME, 4), ("tile_order", FRAME, 8), ("tex0", FRAME, 16),
           ("tex1", FRAME, 32), ("canvas", FRAME, 64), ("resolve", FRAME, 128),
           ("est_state", ESTIMATE, 1), ("est_tiles", ESTIMATE, 2), ("est_stage", ESTIMATE, 4),
           ("feat_planes", FEATURES, 1), ("query_planes", QUERIES, 1), ("query_order", QUERIES, 2),
           ("hist_planes", HISTORY, 1), ("hist_tally", HISTORY, 2))
NAMES = [b[0] for b in BUFFERS]


def extent(width, rows, passes=1):
    """(pixels, 8x8 tiles, passes) of `rows` local rows of a `width`-wide image, unclamped: the header makes 0 count as 1"""
    return (width * rows, ((width + 7) // 8) * ((rows + 7) // 8), passes)


# a band without rows, one tile, four tiles, 16x8 with one and three passes, a grow, a shrink, and two extents of four tiles
# with different pixel counts (9x9, then 16x16)
WALK = (extent(16, 0), extent(8, 8), extent(9, 9), extent(16, 8), extent(16, 8, 3), extent(64, 40, 3), extent(8, 8), extent(9, 9),
        extent(16, 16))


def sizes(e, stage=True):
    """The table: per buffer, ('>=', n) — at least n elements, grown only when smaller — or ('==', n) — exactly n"""
    pix, tiles, passes = (max(v, 1) for v in e)
    t = {"own_accum": (">=", pix), "slab": (">=", pix * passes), "tile_cost": ("==", tiles), "tile_order": ("==", tiles),
         "tex0": (">=", pix), "tex1": (">=", pix), "canvas": (">=", pix), "resolve": (">=", pix),
         "est_state": (">=", 2 * pix), "est_tiles": (">=", 2 * tiles), "feat_planes": ("==", PLANES * pix),
         "query_planes": ("==", PLANES * pix), "query_order": ("==", tiles), "hist_planes": ("==", 2 * pix), "hist_tally": (">=", 3)}
    if stage:
        t["est_stage"] = (">=", 2 * pix)
    return t


def expect_after(before, e, stage=True):
    """capacities after a clean fit of every set to `e` from the capacities `before`, and the names of the reallocated buffers"""
    after, fresh = dict(before), set()
    for name, (rule, n) in sizes(e, stage).items():
        have = before.get(name, 0)
        if (rule == ">=" and have < n) or (rule == "==" and have != n):
            after[name] = n
            fresh.add(name)
    if {"query_planes", "query_order"} & fresh:   # the query planes and their order are put in place together
        fresh |= {"query_planes", "query_order"}
    return after, fresh


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(tempfile.mkdtemp(prefix="buffers_"), "libbuffers_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", os.path.join(HERE, "buffers_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    u64, vp = C.c_uint64, C.c_void_p
    lib.buf_new.restype = vp
    lib.buf_delete.argtypes = [vp]
    lib.buf_fit.argtypes = [vp, C.c_int, u64, u64, u64, C.POINTER(C.c_uint32)]
    lib.buf_in_place.argtypes = [vp, C.c_int, u64, u64, u64]
    lib.buf_toggle.argtypes = [vp, C.c_int, C.c_int, u64, u64, u64]
    lib.buf_buffers.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    lib.buf_flags.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.buf_mark_valid.argtypes = [vp]
    lib.buf_accum.argtypes = [vp, C.POINTER(u64)]
    lib.buf_bind.argtypes = [vp, C.c_int]
    lib.alloc_fail_at.argtypes = [C.c_long]
    lib.alloc_count.restype = lib.alloc_live.restype = C.c_long
    lib.buf_plane_texels.restype = u64
    lib.buf_plane_texels.argtypes = lib.buf_planes_indexable.argtypes = [u64]
    return lib


class Ctx:
    """the five sets of one context behind the shim"""

    def __init__(self, lib, options=True):
        self.lib, self.h = lib, lib.buf_new()
        lib.alloc_reset()
        if options:   # every option turned on before the context has rows (each toggle fits its own set, as pt_set_option does)
            for s in (ESTIMATE, FEATURES, QUERIES, HISTORY):
                assert lib.buf_toggle(self.h, s, 1, 0, 0, 1) == 0

    def close(self):
        self.lib.buf_delete(self.h)
        self.h = None

    def fit(self, s, e):
        out = (C.c_uint32 * 2)()
        rc = self.lib.buf_fit(self.h, s, e[0], e[1], e[2], out)
        return rc, out[0]

    def fit_all(self, e):
        """as ensure_buffers: the sets in order, stopping at the first refusal; the fresh buffers' names"""
        fresh = set()
        for s in SETS:
            rc, bits = self.fit(s, e)
            fresh |= {n for n, bs, bit in BUFFERS if bs == s and bits & bit}
            if rc:
                return rc, fresh
        return 0, fresh

    def in_place(self, s, e):
        return bool(self.lib.buf_in_place(self.h, s, e[0], e[1], e[2]))

    def buffers(self):
        held, cap = (C.c_uint64 * 16)(), (C.c_uint64 * 16)()
        self.lib.buf_buffers(self.h, held, cap)
        return {n: (bool(held[k]), int(cap[k])) for k, n in enumerate(NAMES)}

    def caps(self):
        b = self.buffers()
        for name, (held, cap) in b.items():
            assert held == (cap != 0), (name, held, cap)   # no capacity for a pointer it does not hold, no pointer without one
        return {n: cap for n, (held, cap) in b.items() if held}

    def flags(self):
        out = (C.c_int32 * 8)()
        self.lib.buf_flags(self.h, out)
        return dict(zip(("est_on", "feat_on", "query_on", "hist_on", "est_spp", "feat_valid", "hist_valid", "hist_ran"), out))

    def accum(self):
        px = C.c_uint64()
        return ("null", "own", "bound", "STALE")[self.lib.buf_accum(self.h, C.byref(px))], px.value


def walked_to(lib, k):
    c = Ctx(lib)
    for e in WALK[:k]:
        assert c.fit_all(e)[0] == 0
    return c


def test_every_buffer_of_every_set_has_the_size_the_table_states_and_fresh_names_the_reallocated(shim):
    c = Ctx(shim)
    caps = c.caps()
    # the toggles sized their own sets for a band without rows — as one pixel and one tile —, the estimate's before reprojection
    # was on: no stage yet; the frame set waits for the first fit
    assert caps == {"est_state": 2, "est_tiles": 2, "feat_planes": PLANES, "query_planes": PLANES, "query_order": 1, "hist_planes": 2, "hist_tally": 3}
    for k, e in enumerate(WALK):
        c.lib.buf_mark_valid(c.h)
        want, fresh_want = expect_after(caps, e)
        rc, fresh = c.fit_all(e)
        assert rc == 0 and c.caps() == want and fresh == fresh_want, (k, e, c.caps(), want, fresh, fresh_want)
        assert all(c.in_place(s, e) for s in SETS)
        f = c.flags()
        # validity that belongs to a set ends exactly where the set reallocates; what a pt_reproject tallied stays
        assert (f["est_spp"] == 0) == ("est_state" in fresh) and (f["feat_valid"] == 0) == ("feat_planes" in fresh)
        assert (f["hist_valid"] == 0) == ("hist_planes" in fresh) and f["hist_ran"] == 1
        assert c.accum() == ("own", want["own_accum"])
        caps = want
        # ... and a second fit of the same extent touches nothing
        n = shim.alloc_count()
        assert c.fit_all(e) == (0, set()) and shim.alloc_count() == n and c.caps() == want
    # the last step kept the tile count (four) and changed the pixels: the exact-size planes went, the frame's tile order and
    # costs stayed as they were — nothing to reseed (the query planes' own order is the identity whenever it is put in place)
    assert WALK[-2][1] == WALK[-1][1] == 4 and WALK[-2][0] != WALK[-1][0]
    assert {"feat_planes", "query_planes", "hist_planes"} <= fresh and not {"tile_order", "tile_cost"} & fresh
    # an extent another context's partition would not be in place for
    assert not any(c.in_place(s, WALK[2]) for s in (FEATURES, QUERIES, HISTORY)) and not c.in_place(FRAME, extent(64, 40, 4))
    c.close()
    assert shim.alloc_live() == 0


def test_sets_that_are_off_hold_nothing_and_a_bound_accumulation_is_left_alone(shim):
    c = Ctx(shim, options=False)
    e = WALK[3]
    assert c.fit_all(e)[0] == 0 and set(c.caps()) == {n for n, s, _ in BUFFERS if s == FRAME}
    assert c.in_place(FRAME, e) and not any(c.in_place(s, e) for s in SETS[1:])
    shim.buf_bind(c.h, 1)
    big = extent(64, 40)
    rc, fresh = c.fit_all(big)
    assert rc == 0 and "own_accum" not in fresh and c.caps()["own_accum"] == e[0] and c.accum() == ("bound", 4) and c.in_place(FRAME, big)
    shim.buf_bind(c.h, 0)   # pt_bind_accum(ctx, NULL): the own buffer comes back, grown to the partition in place
    assert c.accum() == ("null", 0) and not c.in_place(FRAME, big)
    rc, fresh = c.fit_all(big)
    assert rc == 0 and "own_accum" in fresh and c.accum() == ("own", big[0]) and c.in_place(FRAME, big)
    c.close()
    assert shim.alloc_live() == 0


def test_the_stage_buffer_exists_exactly_while_the_estimate_and_reprojection_are_both_on(shim):
    e = WALK[3]
    for first, second in ((ESTIMATE, HISTORY), (HISTORY, ESTIMATE)):
        c = Ctx(shim, options=False)
        assert shim.buf_toggle(c.h, FEATURES, 1, *e) == 0 and c.fit_all(e)[0] == 0
        assert shim.buf_toggle(c.h, first, 1, *e) == 0 and c.fit_all(e)[0] == 0
        assert "est_stage" not in c.caps()
        assert shim.buf_toggle(c.h, second, 1, *e) == 0
        assert c.fit_all(e)[0] == 0 and c.caps()["est_stage"] == 2 * e[0]
        for off in (first, second):   # either one off: the stage goes with the next fit, the other set stays in place
            d = Ctx(shim, options=False)
            for s in (FEATURES, first, second):
                assert shim.buf_toggle(d.h, s, 1, *e) == 0
            assert d.fit_all(e)[0] == 0 and "est_stage" in d.caps()
            shim.buf_toggle(d.h, off, 0, *e)
            assert d.fit_all(e) == (0, set()) and "est_stage" not in d.caps()
            assert d.in_place(ESTIMATE if off == HISTORY else HISTORY, e) and not d.in_place(off, e)
            d.close()
        c.close()
    assert shim.alloc_live() == 0


def test_the_planes_index_cap_refuses_before_anything_is_freed(shim):
    cap = 0x3FFFFFFF // PLANES
    # the sizing arithmetic by itself: the cap is accepted and its planes' last texel is indexable with 32 bits, one more is not
    assert shim.buf_planes_indexable(cap) == 1 and shim.buf_planes_indexable(cap + 1) == 0
    assert shim.buf_plane_texels(cap) == PLANES * cap <= 0x3FFFFFFF and shim.buf_plane_texels(cap + 1) > 0x3FFFFFFF
    e = WALK[3]
    for s in (FEATURES, QUERIES):
        c = Ctx(shim)
        assert c.fit_all(e)[0] == 0
        before, n = c.caps(), shim.alloc_count()
        rc, fresh = c.fit(s, (cap + 1, e[1], 1))
        assert rc == 2 and fresh == 0 and shim.alloc_count() == n and c.caps() == before   # nothing asked for, nothing freed
        assert c.in_place(s, e) and not c.in_place(s, (cap + 1, e[1], 1))
        c.close()
    assert shim.alloc_live() == 0


def check_refused(c, s, e, at):
    """what a refused allocation leaves of set `s`"""
    assert not c.in_place(s, e), at
    c.caps()   # (asserts: no buffer reports a capacity for a pointer it does not hold)
    kind, pixels = c.accum()
    assert kind in ("null", "own") and (kind == "own" or pixels == 0), (at, kind, pixels)   # never stale
    if kind == "own":
        assert pixels == c.caps()["own_accum"], at


def test_a_refused_allocation_at_every_k_of_every_transition_of_every_set(shim):
    visited = 0
    for k in range(len(WALK)):
        prev, e = (WALK[k - 1] if k else None), WALK[k]
        for s in SETS:
            c = walked_to(shim, k)
            for earlier in SETS[:s]:   # (as ensure_buffers: the sets before it are in place already)
                assert c.fit(earlier, e)[0] == 0
            shim.alloc_reset()
            assert c.fit(s, e)[0] == 0
            n = shim.alloc_count()   # the allocations this transition makes of this set: counted, not stated
            c.close()
            ran = 0
            for fail in range(1, n + 1):
                c = walked_to(shim, k)
                for earlier in SETS[:s]:
                    assert c.fit(earlier, e)[0] == 0
                shim.alloc_fail_at(fail)
                rc, fresh = c.fit(s, e)
                assert rc == 1 and shim.alloc_count() == fail, (k, s, fail)
                shim.alloc_reset()
                check_refused(c, s, e, (k, s, fail))
                got = c.buffers()
                for name, bs, bit in BUFFERS:   # fresh names what was reallocated and is in place, never the refused buffer
                    if bs == s and fresh & bit:
                        assert got[name][0], (k, s, fail, name)
                if s == FRAME and prev is not None and "own_accum" in c.caps() and c.caps()["own_accum"] >= max(e[0], 1):
                    assert c.accum()[0] == "own"   # a later buffer's refusal leaves the accumulation readable
                assert c.fit(s, e)[0] == 0 and c.in_place(s, e), (k, s, fail)   # the next fit, unrefused, puts the set in place
                assert c.fit_all(e)[0] == 0 and all(c.in_place(t, e) for t in SETS)
                c.close()
                ran += 1
            assert ran == n, (k, s, ran, n)
            visited += n
    assert visited > 40 and shim.alloc_live() == 0


def test_a_toggle_that_is_refused_leaves_the_option_off_with_every_buffer_released(shim):
    e = WALK[3]
    for s in (ESTIMATE, FEATURES, QUERIES, HISTORY):
        own = {n for n, bs, _ in BUFFERS if bs == s}
        c = Ctx(shim, options=False)
        assert c.fit_all(e)[0] == 0
        if s != FEATURES:   # (reprojection needs the features on; with it on the estimate's toggle allocates the stage too)
            assert shim.buf_toggle(c.h, FEATURES, 1, *e) == 0
        if s == ESTIMATE:
            assert shim.buf_toggle(c.h, HISTORY, 1, *e) == 0
        shim.alloc_reset()
        assert shim.buf_toggle(c.h, s, 1, *e) == 0 and c.in_place(s, e)
        n = shim.alloc_count()
        assert n == len(own) and own <= set(c.caps())
        shim.buf_toggle(c.h, s, 0, *e)
        assert not own & set(c.caps()) and not c.in_place(s, e)
        ran = 0
        for fail in range(1, n + 1):
            shim.alloc_fail_at(fail)
            assert shim.buf_toggle(c.h, s, 1, *e) == 1
            shim.alloc_reset()
            f = c.flags()
            assert f[("est_on", "feat_on", "query_on", "hist_on")[s - 1]] == 0 and not own & set(c.caps()) and not c.in_place(s, e)
            assert c.in_place(FRAME, e)
            ran += 1
        assert ran == n
        assert shim.buf_toggle(c.h, s, 1, *e) == 0 and c.in_place(s, e)
        c.close()
    assert shim.alloc_live() == 0


def test_ownership_under_address_and_undefined_behaviour_sanitizers():
    """tests/buffers_main.cpp: a stand-alone program (its own main) over the same header and stand-in allocator, built with
    -fsanitize=address,undefined and run as a child: the walk above with a refused allocation at every k of every set and every
    toggle, moves and releases of the buffers.  A double free, a leak or a use after free ends it non-zero."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "buffers_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(HERE, "buffers_main.cpp"), "-o", exe])
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and "buffers: ok" in out.stdout, out.stdout[-2000:]
