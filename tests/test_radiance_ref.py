"""tests/radiance_ref.py (the restatement the GPU tests of pt_query_radiance compare against) pinned on the CPU, statement by
statement of the header's list: what a miss gives, what a first hit gives at depth 1, how samples chain on one seed, how passes
add, which passes a second batch takes, and that a time step of 0 means 1.  CPU only."""
import ctypes as C

import numpy as np

import query_ref as Q
import radiance_ref as RR
from oracle import oracle
from ray_tracer_webgl_amd import abi, scenes
from test_query_ref import sphere_list

D, M, G, E = abi.PT_DIFFUSE, abi.PT_METAL, abi.PT_GLASS, abi.PT_EMISSIVE
F32 = np.float32


def params(spp=2, depth=6, first_pass=0, step=abi.PT_TIME_STEP_DECORRELATED, bg=None, w=37, h=21):
    p = scenes.default_scene(w, h, spp=spp, max_depth=depth).params.copy()
    p.time, p.time_step, p.first_pass = 3.25, step, first_pass
    if bg is not None:
        p.background_mode = bg
    return p


SPH = sphere_list([((0, 0, -3), 1.0, D, (0.1, 0.2, 0.3)), ((4, 0, -3), 1.0, E, (2.0, 3.0, 4.0)), ((-4, 0, -3), 1.0, M, (0.8, 0.6, 0.4)),
                   ((0, 4, -3), 1.0, G, (1.0, 1.0, 1.0))])
UP = (F32([[0, 0, 0]]), F32([[0.3, 2.0, 0.1]]))        # misses everything
AT_DIFFUSE = (F32([[0, 0, 0]]), F32([[0, 0, -2.0]]))
AT_EMISSIVE = (F32([[0, 0, 0]]), F32([[4, 0, -3.0]]))


def chained(sph, p, o, d, seed, n):
    """n ora_ray_color calls on one carried seed: the colours, the seed afterwards"""
    L = oracle.load()
    ptr, n_sph, keep = abi.spheres_as_ctypes(np.ascontiguousarray(sph, dtype=abi.SPHERE_DTYPE))
    oo, dd, col = (C.c_float * 3)(*[float(x) for x in o]), (C.c_float * 3)(*[float(x) for x in d]), (C.c_float * 3)()
    s, seg, cols = C.c_float(seed), C.c_uint64(0), []
    for _ in range(n):
        L.ora_ray_color(ptr, n_sph, C.byref(p), oo, dd, C.byref(s), col, C.byref(seg))
        cols.append(F32(col[:]))
    return cols, s.value


def test_a_miss_adds_the_background_once_per_sample():
    for spp, n_passes in ((1, 1), (2, 3), (5, 2)):
        p = params(spp=spp)
        rec, seg = RR.records(SPH, p, *UP, n_passes)
        bg = Q.records(SPH, p, *UP)[0]
        assert bg["index"] == -1 and bg["albedo"][2] == F32(1.0)
        want = np.zeros(3, F32)
        for _ in range(n_passes):
            s = np.zeros(3, F32)
            for _ in range(spp):
                s = s + bg["albedo"]
            want = want + s
        assert np.array_equal(rec[0, :3].view(np.uint32), want.view(np.uint32)) and rec[0, 3] == spp * n_passes
        assert seg == spp * n_passes  # one segment per sample
    black, seg = RR.records(SPH, params(bg=abi.PT_BG_BLACK), *UP, 3)
    assert not black[0, :3].view(np.uint32).any() and black[0, 3] == 6 and seg == 6


def test_first_hits_at_depth_one_and_an_emissive_sphere_at_any_depth():
    for depth in (1, 6):
        p = params(depth=depth)
        rec, seg = RR.records(SPH, p, *AT_EMISSIVE, 1)
        assert np.array_equal(rec[0], F32([4.0, 6.0, 8.0, 2.0])) and seg == 2  # its albedo per sample, two samples
    rec, seg = RR.records(SPH, params(depth=1), *AT_DIFFUSE, 1)
    assert np.array_equal(rec[0, :3], F32([0.1, 0.2, 0.3]) + F32([0.1, 0.2, 0.3])) and rec[0, 3] == 2 and seg == 2


def test_samples_chain_on_one_seed_and_passes_do_not():
    L = oracle.load()
    p2, p1 = params(spp=2), params(spp=1)
    o, d = AT_DIFFUSE
    vx, vy = L.ora_v_position(0, 37), L.ora_v_position(0, 21)
    seed = L.ora_init_seed(vx, vy, float(RR.u_time(p2, 0)))
    cols, after = chained(SPH, p2, o[0], d[0], seed, 2)
    assert after != seed
    one_pass, _ = RR.records(SPH, p2, o, d, 1)
    assert np.array_equal(one_pass[0, :3].view(np.uint32), ((np.zeros(3, F32) + cols[0]) + cols[1]).view(np.uint32))
    two_passes, _ = RR.records(SPH, p1, o, d, 2)
    assert two_passes[0, 3] == one_pass[0, 3] == 2
    assert not np.array_equal(two_passes[0, :3], one_pass[0, :3])
    assert np.array_equal(cols[0], RR.records(SPH, p1, o, d, 1)[0][0, :3])  # the first sample is the same ...
    assert not np.array_equal(cols[0], cols[1])                              # ... and the second continues the stream


def test_two_passes_are_the_passes_f_and_f_plus_one_added_in_order():
    o, d = AT_DIFFUSE
    f = 7
    both, seg = RR.records(SPH, params(first_pass=f), o, d, 2)
    a, sa = RR.records(SPH, params(first_pass=f), o, d, 1)
    b, sb = RR.records(SPH, params(first_pass=f + 1), o, d, 1)
    want = (np.zeros(4, F32) + a[0]) + b[0]
    assert np.array_equal(both[0].view(np.uint32), want.view(np.uint32)) and seg == sa + sb
    assert not np.array_equal(a[0, :3], b[0, :3])


def test_the_second_batch_takes_passes_of_its_own():
    p = params(first_pass=2)
    B = RR.batch(p)
    assert B == 777
    rng = np.random.default_rng(2401)
    o = np.zeros((B + 40, 3), F32)
    d = rng.standard_normal((B + 40, 3)).astype(F32)
    d[:, 2] = -np.abs(d[:, 2]) - F32(1.0)
    n_passes = 2
    all_, seg = RR.records(SPH, p, o, d, n_passes)
    first, seg1 = RR.records(SPH, p, o[:B], d[:B], n_passes)
    later, seg2 = RR.records(SPH, params(first_pass=2 + n_passes), o[B:], d[B:], n_passes)
    assert np.array_equal(RR.raw(all_[:B]), RR.raw(first)) and np.array_equal(RR.raw(all_[B:]), RR.raw(later)) and seg == seg1 + seg2
    # the same ray at the same place of the two batches shares no random numbers
    same_o, same_d = np.tile(AT_DIFFUSE[0], (B + 1, 1)), np.tile(AT_DIFFUSE[1], (B + 1, 1))
    rec, _ = RR.records(SPH, p, same_o, same_d, n_passes)
    assert not np.array_equal(rec[0, :3], rec[B, :3]) and not RR.has_nan(rec)


def test_a_time_step_of_zero_means_one():
    o, d = AT_DIFFUSE
    zero, _ = RR.records(SPH, params(step=0.0, first_pass=3), o, d, 2)
    one, _ = RR.records(SPH, params(step=1.0, first_pass=3), o, d, 2)
    other, _ = RR.records(SPH, params(step=0.5, first_pass=3), o, d, 2)
    assert np.array_equal(RR.raw(zero), RR.raw(one)) and not np.array_equal(RR.raw(zero), RR.raw(other))


def test_invalid_rays_give_zeros_and_no_segment():
    o, d = Q.invalid_rays()
    rec, seg = RR.records(SPH, params(), o, d, 3)
    assert not RR.raw(rec).any() and seg == 0
