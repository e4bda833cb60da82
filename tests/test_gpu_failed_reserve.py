"""A refused pt_reserve_passes on the device: the reservation that cannot be had frees the pass slabs (a buffer is freed before
its successor is asked for) and the context's buffers are then not in place — the render and read-out calls answer
PT_ERR_CAPACITY and enqueue nothing until a sizing call succeeds, the accumulation stays readable, and the frame rendered after
the next good reservation is the frame rendered before, bit for bit.

Two cautions.  This test must never be run against a library from before the frame set got its contract (pt_buffers.hpp,
frame_buffers_ready in pt_api.hip): there, step 3 launches a trace kernel through a null slab pointer — the device fault this
contract removes.  And on correct code step 3 launches NOTHING: each of the four entry points reaches frame_buffers_ready before
its first enqueue (pt_render_passes and pt_render_features through prepare_launch, pt_render_frame through frame_ready,
pt_resolve in resolve_common), which is what makes the step safe to run."""
import ctypes as C

import numpy as np
import pytest

from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer

pytestmark = pytest.mark.gpu

W, H = 16, 8
# 16 * 8 pixels * 2^30 passes * 16 bytes = 2 TiB of slabs: several times the card's memory, and the size_t product does not overflow
UNSATISFIABLE = 0x40000000


def test_a_refused_reservation_refuses_the_render_calls_until_the_next_good_one():
    sc = scenes.default_scene(W, H, spp=1, max_depth=6)
    t = PathTracer(W, H)
    try:
        lib, ctx = t.lib, t._ctx
        t.set_spheres(sc.spheres)
        t.error_estimate(True)
        t.feature_planes(True)
        t.set_params(sc.params)
        # 1. one pass
        t.render_passes(1)
        a = t.accum().copy()
        assert (a[..., 3] == 1).all()
        # 2. the reservation that cannot be had
        rc = lib.pt_reserve_passes(ctx, UNSATISFIABLE)
        assert rc == abi.PT_ERR_HIP, "pt_reserve_passes(2^30) returned %d: nothing more is rendered" % rc
        assert lib.pt_last_error(ctx)
        # 3. refused, by name, with nothing enqueued
        segments = t.stats().segments
        out = np.zeros((H, W, 4), np.float32)
        for who, call in (("pt_render_passes", lambda: lib.pt_render_passes(ctx, 1)),
                          ("pt_render_frame", lambda: lib.pt_render_frame(ctx, 1)),
                          ("pt_render_features", lambda: lib.pt_render_features(ctx)),
                          ("pt_resolve", lambda: lib.pt_resolve(ctx, out.ctypes.data_as(C.c_void_p), 1))):
            assert call() == abi.PT_ERR_CAPACITY, who
            msg = lib.pt_last_error(ctx).decode()
            assert who in msg and "not allocated for the rows in place" in msg, msg
        assert not out.any()
        st = t.stats()   # (pt_get_stats still answers)
        assert st.segments == segments and st.total_spp == 1
        b = t.accum()    # (and so does pt_read_accum)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        # 4. the next good reservation puts the slabs back; the same pass again is the same frame, and no stale error surfaces
        assert lib.pt_reserve_passes(ctx, 2) == abi.PT_OK
        t.reset()
        assert lib.pt_render_passes(ctx, 1) == abi.PT_OK
        b = t.accum()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        t.render_features()
        assert t.resolve().shape[:2] == (H, W)
    finally:
        t.close()
