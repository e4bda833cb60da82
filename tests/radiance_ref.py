"""The records of include/ptrace.h pt_query_radiance, restated from the oracle's exported pieces only: ora_v_position (the
pixel centre of a place), ora_init_seed (the seed of a place and a pass), ora_ray_color (the shader's loop for ANY ray, the seed
carried by the caller), query_ref.valid (the validity predicate) and numpy float32 adds.  TEST INFRASTRUCTURE ONLY.

The statement list of the header, line for line: ray i lies in batch b = i / B at place j = i % B (B the local pixel count);
the place gives the pixel centre, the pixel centre and the pass (first_pass + b * n_passes + p) give the seed, and the seed walks
samples_per_pixel chained ray_color calls along the caller's ray."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import query_ref as Q
from feature_ref import owned_rows
from oracle import oracle
from ray_tracer_webgl_amd import abi

F32 = np.float32


def batch(params):
    """B: the rays one launch takes, i.e. the local pixel count of a context with these uniforms"""
    return len(owned_rows(params)) * int(params.width)


def u_time(params, pass_number):
    """time + float(pass) * step in float32: multiply, then add; a step of 0 means 1; the pass number wraps at 2^32"""
    step = F32(params.time_step) if params.time_step != 0.0 else F32(1.0)
    return F32(F32(params.time) + F32(F32(np.uint32(pass_number & 0xffffffff)) * step))


def records(spheres, params, origins, directions, n_passes):
    """((n, 4) float32 {sum r, g, b, samples}, segments traced): the record of every ray under the list `spheres` and the
    uniforms `params`, and the total of ora_ray_color's segment counts"""
    L = oracle.load()
    sph = np.ascontiguousarray(spheres, dtype=abi.SPHERE_DTYPE)
    ptr, n_sph, keep = abi.spheres_as_ctypes(sph)
    p = params.copy()
    o_all = np.ascontiguousarray(origins, F32).reshape(-1, 3)
    d_all = np.ascontiguousarray(directions, F32).reshape(-1, 3)
    assert o_all.shape == d_all.shape and n_passes >= 1
    ok = Q.valid(o_all, d_all)
    rows, w = owned_rows(p), int(p.width)
    B = len(rows) * w
    spp = int(p.samples_per_pixel)
    out = np.zeros((len(o_all), 4), F32)

    def some(indices):
        """the records of these rays into `out` (every ray is independent of every other), their segments"""
        o, d, col = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)()
        total = 0
        for i in indices:
            b, j = divmod(int(i), B)
            px, ly = j % w, j // w
            vx, vy = L.ora_v_position(px, p.width), L.ora_v_position(int(rows[ly]), p.height)
            o[:] = [float(x) for x in o_all[i]]
            d[:] = [float(x) for x in d_all[i]]
            rec = np.zeros(4, F32)
            for k in range(n_passes):
                seed = C.c_float(L.ora_init_seed(vx, vy, float(u_time(p, int(p.first_pass) + b * n_passes + k))))
                s = np.zeros(3, F32)
                for _ in range(spp):
                    seg = C.c_uint64(0)
                    L.ora_ray_color(ptr, n_sph, C.byref(p), o, d, C.byref(seed), col, C.byref(seg))
                    total += int(seg.value)
                    s = s + np.array(col[:], F32)
                rec[:3] = rec[:3] + s
                rec[3] = rec[3] + F32(spp)
            out[i] = rec
        return total

    todo = np.flatnonzero(ok)  # an invalid ray: {+0, +0, +0, +0}, no segment
    # a long list makes ora_ray_color the whole cost, and ctypes calls run beside each other: the rays in interleaved shares
    workers = min(16, os.cpu_count() or 1) if len(todo) * n_sph * n_passes * spp > 20_000_000 else 1
    if workers > 1:
        with ThreadPoolExecutor(workers) as pool:
            return out, sum(pool.map(some, [todo[k::workers] for k in range(workers)]))
    return out, some(todo)


def raw(rec):
    """(n, 4) uint32: the 16 bytes of each record"""
    return np.ascontiguousarray(rec, F32).view(np.uint32).reshape(-1, 4)


def has_nan(rec):
    return bool(np.isnan(np.asarray(rec, F32)).any())
