"""Gather queries on the CPU (pt_gather_irradiance, pt_bake_probes; include/ptrace.h has the contract): the restatement
tests/gather_ref.py the device tests compare with, and csrc/pt_gather.hpp, which the kernels compile.

  1. the arithmetic   csrc/pt_gather.hpp through tests/gather_shim.cpp equals the restatement's numpy statements bit for bit over
                      the sweep of tests/gather_sweep.hpp: every j of D = 64, 128 and 4096, the normals (axes both ways, the
                      frame's pole, unnormalised, tiny, huge), the reduction on records with mixed signs, a zero and a NaN;
                      tests/gather_main.cpp walks the same sweep under the sanitizers;
  2. the quadrature   the set in float64 on the shader's sky against the closed forms, within bounds derived from the set;
  3. sh_irradiance    against the cosine set on that sky;
  4. the surface      struct sizes, the symbols, ABI version 5, the header's, Python's and Rust's agreement, the error wording in
                      the source, the workspace set in place or refused, and that pt_set_option(14) is still an unknown key.
CPU only.

THE QUADRATURE BOUNDS (section 2 and 3).  The sky is L_c(omega) = A_c + B_c y with A = (1 + col) / 2, B = (col - 1) / 2,
col = (0.5, 0.7, 1): |A| <= 1, |B| <= 0.25.  Every integrand of the set is a sum of (i) a polynomial f(y) alone and (ii) products
P(y) Q(phi) with Q one of cos phi, sin phi, cos 2 phi, sin 2 phi (sin^2 and cos^2 are split into their mean, which goes to (i),
and half of cos 2 phi).
  (i)  y_j = 1 - (2 j + 1) / D is the MIDPOINT RULE on [-1, 1] with D cells of width h = 2 / D: the error of h sum f(y_j) is at
       most 2 h^2 / 24 max |f''| = max |f''| / (3 D^2); the sphere's weight is 2 pi.  That is the O(1 / D^2) of the stratified
       coordinate, and 0 for a linear f (sh[0]).
  (ii) phi_j = 2 pi frac(j g) with g = 0x9E3779B97F4A7C15 / 2^64 (cut to 24 bits: a change of phi of at most 2 pi 2^-24 per term), so
       sum_{j < m} exp(i k phi_j) is a geometric sum of modulus at most 1 / |sin(pi k g)| for every m, and by Abel summation
       |sum_j P(y_j) Q_k(phi_j)| <= (|P(y_{D-1})| + V(P)) / |sin(pi k g)|, V the total variation: an error of O(1 / D) — what
       the set's discrepancy gives.  With sup and V of the factors (V(f g) <= sup f V(g) + sup g V(f)):
       L: sup 1.25, V 0.5;  r = sqrt(1 - y^2): sup 1, V 2;  r^2: sup 1, V 2;  y r: sup 0.5, V 2;  and P(y_{D-1}) -> r = O(D^-1/2)
       is bounded by its sup.
For the cosine set about +y the frame gives omega = (lx, lz, -ly): omega_y = sqrt(1 - u) alone, u_j = (2 j + 1) / (2 D) the
midpoint rule on [0, 1] with h = 1 / D for f = sqrt(1 - u), whose second derivative is not bounded at 1: cell by cell,
h^3 / 24 |f''| summed over the cells but the last is at most h^1.5 zeta(1.5) / 96 <= 0.0273 h^1.5, and the last cell's error is
(1 / sqrt 2 - 2 / 3) h^1.5 <= 0.0405 h^1.5: 0.068 D^-1.5 in all, times pi |B|.  About another normal n, omega_y = n_y sqrt(1 - u)
+ sqrt(u) (t_y cos phi + bt_y sin phi) with |(t_y, bt_y)| <= 1: the first term as before, the second by (ii) with P = sqrt(u)
(sup 1, V 1, k = 1)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import gather_ref as G
from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd._lib import ADDED_WITHIN_ABI_5, LIB_PATH, SIGNATURES

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "ptrace.h")
F = np.float32
NAMES = ("pt_gather_irradiance", "pt_bake_probes")
GOLDEN = 0x9E3779B97F4A7C15 / 2.0 ** 64
COL = np.array([0.5, 0.7, 1.0])
A_SKY, B_SKY = (1.0 + COL) / 2.0, (COL - 1.0) / 2.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(tempfile.mkdtemp(prefix="gather_"), "libgather_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror", os.path.join(HERE, "gather_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    fp, u32, u64, vp = C.POINTER(C.c_float), C.c_uint32, C.c_uint64, C.c_void_p
    lib.gth_directions_valid.argtypes = [u32]
    lib.gth_total_rays.restype, lib.gth_total_rays.argtypes = u64, [u32, u32]
    lib.gth_items_per_batch.restype, lib.gth_items_per_batch.argtypes = u32, [u32]
    lib.gth_item_span.restype, lib.gth_item_span.argtypes = None, [u32, u32, u32, C.POINTER(u32)]
    lib.gth_item_valid.argtypes = [vp, C.c_int]
    lib.gth_stratum.restype, lib.gth_stratum.argtypes = C.c_float, [u32, u32]
    lib.gth_turn.restype, lib.gth_turn.argtypes = C.c_float, [u32]
    lib.gth_unit_normal.restype, lib.gth_unit_normal.argtypes = None, [fp, fp]
    lib.gth_ray.restype, lib.gth_ray.argtypes = None, [vp, C.c_int, u32, u32, C.c_float, C.c_float, fp]
    lib.gth_basis.restype, lib.gth_basis.argtypes = None, [fp, fp]
    lib.gth_reduce.restype, lib.gth_reduce.argtypes = None, [C.c_int, vp, u32, fp, fp]
    lib.gth_sweep_normals.restype, lib.gth_sweep_normals.argtypes = u32, [fp]
    lib.gth_sweep_counts.restype, lib.gth_sweep_counts.argtypes = u32, [C.POINTER(u32)]
    lib.gth_sweep_records.restype, lib.gth_sweep_records.argtypes = None, [u32, C.c_int, vp]
    lib.alloc_fail_at.argtypes = [C.c_long]
    lib.alloc_live.restype = C.c_long
    lib.set_new.restype = vp
    for f in (lib.set_delete, lib.set_release, lib.set_capacity):
        f.argtypes = [vp]
    lib.set_fit.argtypes = lib.set_in_place.argtypes = [vp, u64]
    lib.set_capacity.restype = u64
    lib.set_layout.restype, lib.set_layout.argtypes = None, [vp, u64, C.POINTER(u64)]
    lib.set_carry_slots.restype, lib.set_carry_slots.argtypes = None, [vp, C.POINTER(u64)]
    return lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def sweep_normals(shim):
    n = shim.gth_sweep_normals(None)
    buf = np.zeros((n, 3), F)
    shim.gth_sweep_normals(_fp(buf))
    return buf


def sweep_counts(shim):
    n = shim.gth_sweep_counts(None)
    buf = (C.c_uint32 * n)()
    shim.gth_sweep_counts(buf)
    return [int(v) for v in buf]


def point(position, normal=(0.0, 0.0, 0.0)):
    p = np.zeros(8, F)
    p[0:3], p[4:7] = position, normal
    return p


# ------------------------------------------------------------------------------------- 1. the arithmetic
def test_the_set_equals_the_restatement_for_every_j(ora, shim):
    assert sweep_counts(shim) == [64, 128, 4096]
    for D in sweep_counts(shim):
        j = np.arange(D)
        a = np.array([shim.gth_stratum(int(k), D) for k in j], F)
        u = np.array([shim.gth_turn(int(k)) for k in j], F)
        assert np.array_equal(bits(a), bits(G.stratum(j, D))) and np.array_equal(bits(u), bits(G.turn(j)))
        assert (u >= 0).all() and (u < 1).all() and np.allclose(u, np.mod(j * 0.61803398875, 1.0), atol=2.0 ** -24 + 4096 * 1e-13)
        _, s, c = G.the_set(D)
        want = G.sphere_directions(D)
        got, out = np.zeros((D, 3), F), np.zeros(8, F)
        probe = point((0.25, -3.0, 7.5))
        for k in j:
            shim.gth_ray(probe.ctypes.data, G.PROBE, int(k), D, float(s[k]), float(c[k]), _fp(out))
            assert np.array_equal(bits(out[0:3]), bits(probe[0:3])) and out[3] == 0 and out[7] == 0
            got[k] = out[4:7]
        assert np.array_equal(bits(got), bits(want)), D
        assert np.array_equal(bits(got[:, 1]), bits(F(1.0) - a)), "+y is the stratified axis"
        assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_the_frame_equals_the_restatement_for_every_normal_and_j(ora, shim):
    normals = sweep_normals(shim)
    assert any((n == (0, 0, -1)).all() for n in normals) and any(0 < np.abs(n).max() < 1e-25 for n in normals) and any(np.abs(n).max() > 1e25 for n in normals)
    for axis in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        assert any((n == axis).all() for n in normals), axis
    z, out = np.zeros(3, F), np.zeros(8, F)
    for n in normals:
        shim.gth_unit_normal(_fp(n.copy()), _fp(z))
        assert np.array_equal(bits(z), bits(G.unit_normal(n))), n
        assert abs(np.linalg.norm(z.astype(np.float64)) - 1.0) < 1e-6, n
        item = point((1.5, 0.5, -2.0), n)
        assert shim.gth_item_valid(item.ctypes.data, G.IRRADIANCE) == 1
        for D in sweep_counts(shim):
            _, s, c = G.the_set(D)
            want = G.hemisphere_directions(n, D)
            got = np.zeros((D, 3), F)
            for k in range(D):
                shim.gth_ray(item.ctypes.data, G.IRRADIANCE, k, D, float(s[k]), float(c[k]), _fp(out))
                got[k] = out[4:7]
            assert np.array_equal(bits(got), bits(want)), (n, D)
            w = got.astype(np.float64)
            assert np.abs(np.linalg.norm(w, axis=1) - 1.0).max() < 1e-5 and (w @ z.astype(np.float64) > 0).all(), (n, D)


def test_invalid_items(shim):
    nan, inf = np.nan, np.inf
    cases = [((nan, 0, 0), (0, 1, 0), False, False), ((0, inf, 0), (0, 1, 0), False, False), ((0, 0, -inf), (0, 1, 0), False, False),
             ((1, 2, 3), (0, 0, 0), False, True), ((1, 2, 3), (-0.0, 0.0, -0.0), False, True), ((1, 2, 3), (nan, 1, 0), False, True),
             ((1, 2, 3), (0, inf, 0), False, True), ((1, 2, 3), (0, 1e-45, 0), True, True), ((1e38, -1e38, 0), (1, 0, 0), True, True)]
    out = np.zeros(8, F)
    for pos, nrm, irr, probe in cases:
        item = point(pos, nrm)
        for kind, want in ((G.IRRADIANCE, irr), (G.PROBE, probe)):
            assert bool(shim.gth_item_valid(item.ctypes.data, kind)) == want == G.item_valid(kind, pos, nrm), (pos, nrm, kind)
            shim.gth_ray(item.ctypes.data, kind, 3, 64, 0.0, 1.0, _fp(out))
            assert (not bits(out).any()) == (not want), "an invalid item's ray is the null ray, all +0"
    o, d = G.rays(G.IRRADIANCE, [(1, 2, 3), (nan, 0, 0), (4, 5, 6)], [(0, 1, 0)] * 3, 64)
    assert not bits(o[64:128]).any() and not bits(d[64:128]).any() and (o[128] == (4, 5, 6)).all() and len(o) == 192


def test_the_basis_equals_the_restatement(shim):
    w = np.concatenate([G.sphere_directions(128), np.eye(3, dtype=F), -np.eye(3, dtype=F)])
    got = np.zeros((len(w), 9), F)
    for k in range(len(w)):
        shim.gth_basis(_fp(w[k].copy()), _fp(got[k]))
    assert np.array_equal(bits(got), bits(G.sh_basis(w)))
    y = got[128 + 1].astype(np.float64)  # omega = +y: the order (0,0), (1,-1) = y, (1,0) = z, (1,1) = x, ..., (2,2) = x^2 - y^2
    assert np.allclose(y, [0.282095, 0.488603, 0, 0, 0, 0, -0.315392, 0, -0.546274], atol=1e-7)


@pytest.mark.parametrize("with_nan", [False, True], ids=["finite", "nan"])
def test_the_reduction_equals_the_restatement(ora, shim, with_nan):
    for D in sweep_counts(shim):
        rec = np.zeros((D, 4), F)
        shim.gth_sweep_records(D, int(with_nan), rec.ctypes.data)
        assert (rec[:, :3] < 0).any() and (rec[:, :3] > 0).any() and (rec[:, :3] == 0).any() and np.isnan(rec).any() == with_nan
        _, s, c = G.the_set(D)
        sc = np.ascontiguousarray(np.stack([s, c], axis=1))
        for kind, floats in ((G.IRRADIANCE, 4), (G.PROBE, 28)):
            got = np.zeros(floats, F)
            shim.gth_reduce(kind, rec.ctypes.data, D, _fp(sc), _fp(got))
            want = G.reduce_item(kind, rec, D)
            nan_got, nan_want = np.isnan(got), np.isnan(want)
            assert np.array_equal(nan_got, nan_want) and nan_got.any() == with_nan, "a NaN stays a NaN, in its channel only"
            assert np.array_equal(bits(got)[~nan_got], bits(want)[~nan_want]), (D, kind)
            assert got[-1] == 4.0 * D
            if not with_nan:  # ... and the order matters: the plain ascending sum gives other bits somewhere, and agrees to rounding
                plain = rec[:, :3].astype(np.float64) / 4.0
                if kind == G.IRRADIANCE:
                    assert np.allclose(got[:3], np.pi / D * plain.sum(axis=0), rtol=0, atol=1e-5 * np.abs(plain).sum(axis=0).max() * np.pi / D)


def test_header_under_address_and_undefined_behaviour_sanitizers():
    """tests/gather_main.cpp: a stand-alone program (its own main) over csrc/pt_gather.hpp on the sweep and exactly sized heap
    arrays, built with -fsanitize=address,undefined and run as a child; nothing sanitized is loaded into this process"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "gather_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                               os.path.join(HERE, "gather_main.cpp"), "-o", exe])
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and "gather: ok" in out.stdout, out.stdout[-2000:]


# ------------------------------------------------------------------------------------- 2. the quadrature
def osc(k):
    """1 / |sin(pi k g)|: the bound of every partial sum of exp(i k phi_j)"""
    return 1.0 / abs(np.sin(np.pi * k * GOLDEN))


def float64_sum_slack(D):
    """the float64 sums themselves: D terms, each at most 4 pi 1.25 1.1 / D in magnitude (|L| <= 1.25, |Y_k| <= 1.1), summed with
    at most D roundings of 2^-53 relative to the running sum: D 2^-53 times 16"""
    return D * 2.0 ** -53 * 16.0


def probe_bounds(D, A=A_SKY, B=B_SKY):
    """(9, 3): the bound of |quadrature - integral| per coefficient and channel for the radiance A + B y, from the module
    docstring.  sup L <= |A| + |B|, V(L) = 2 |B| per channel; the cut of phi to 24 bits moves a term by at most
    k 2 pi 2^-24 sup|P| (added to every (ii) term)."""
    A_SKY, B_SKY = np.asarray(A, np.float64), np.asarray(B, np.float64)
    supL, varL = np.abs(A_SKY) + np.abs(B_SKY), 2.0 * np.abs(B_SKY)
    w = 4.0 * np.pi / D

    def mid(f2):  # (i): 2 pi max|f''| / (3 D^2)
        return 2.0 * np.pi * f2 / (3.0 * D * D)

    def abel(K, supR, varR, k):  # (ii) for P = K L(y) R(y), Q of frequency k
        supP, varP = K * supL * supR, K * (supL * varR + supR * varL)
        return w * (supP + varP) * osc(k) + 4.0 * np.pi * supP * k * 2.0 * np.pi * 2.0 ** -24

    k1, k2, k3, k4 = 0.488603, 1.092548, 0.315392, 0.546274
    round64 = np.zeros(3) + float64_sum_slack(D)
    return round64 + np.stack([
        np.zeros(3),                                               # Y0 L: linear in y, the midpoint rule is exact
        mid(2.0 * k1 * np.abs(B_SKY)),                             # Y1 L = k1 (A y + B y^2): f'' = 2 k1 B
        abel(k1, 1.0, 2.0, 1),                                     # Y2 = k1 r sin phi
        abel(k1, 1.0, 2.0, 1),                                     # Y3 = k1 r cos phi
        abel(k2, 0.5, 2.0, 1),                                     # Y4 = k2 (y r) cos phi
        abel(k2, 0.5, 2.0, 1),                                     # Y5 = k2 (y r) sin phi
        # Y6 = k3 (3 r^2 sin^2 phi - 1) = k3 (1.5 r^2 - 1) - 1.5 k3 r^2 cos 2 phi; f = k3 (0.5 - 1.5 y^2)(A + B y): |f''| <= k3 (3 |A| + 9 |B|)
        mid(k3 * (3.0 * np.abs(A_SKY) + 9.0 * np.abs(B_SKY))) + abel(1.5 * k3, 1.0, 2.0, 2),
        abel(0.5 * k2, 1.0, 2.0, 2),                               # Y7 = k2 r^2 sin phi cos phi = 0.5 k2 r^2 sin 2 phi
        # Y8 = k4 (r^2 cos^2 phi - y^2) = k4 (0.5 - 1.5 y^2) + 0.5 k4 r^2 cos 2 phi
        mid(k4 * (3.0 * np.abs(A_SKY) + 9.0 * np.abs(B_SKY))) + abel(0.5 * k4, 1.0, 2.0, 2),
    ])


def cosine_bound(normal, D, B=B_SKY):
    """(3,): |(pi / D) sum L(omega_j) - E(n)| about the unit normal n for the radiance A + B y (module docstring)"""
    B_SKY = np.asarray(B, np.float64)
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    stratified = np.pi * np.abs(B_SKY) * abs(n[1]) * 0.068 * D ** -1.5
    tangent = 0.0 if abs(abs(n[1]) - 1.0) < 1e-15 else (np.pi / D) * np.abs(B_SKY) * 2.0 * osc(1) + np.pi * np.abs(B_SKY) * 2.0 * np.pi * 2.0 ** -24
    return stratified + tangent + float64_sum_slack(D)


def sky_irradiance(normal):
    """the cosine convolution of A + B y: pi A + (2 pi / 3) B n_y"""
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    return np.pi * A_SKY + 2.0 * np.pi / 3.0 * B_SKY * n[1]


@pytest.mark.parametrize("D", [64, 4096])
def test_the_probe_set_integrates_the_sky(D):
    sh = G.probe64(G.sky, D)
    closed = np.zeros((9, 3))
    closed[0] = 2.0 * np.sqrt(np.pi) * np.array([0.75, 0.85, 1.0])
    closed[1] = np.sqrt(4.0 * np.pi / 3.0) * 0.5 * np.array([-0.5, -0.3, 0.0])
    # the integrals with the header's six-decimal constants in the basis: 0.282095 and 0.488603 are 1 / (2 sqrt pi) and
    # sqrt(3 / (4 pi)) to within 0.5e-6, i.e. to 1.8e-6 and 1.1e-6 of their value
    want = np.zeros((9, 3))
    want[0] = 4.0 * np.pi * 0.282095 * A_SKY
    want[1] = 4.0 * np.pi / 3.0 * 0.488603 * B_SKY
    assert (np.abs(want - closed) <= 1.8e-6 * np.abs(closed)).all()
    bound = probe_bounds(D)
    err = np.abs(sh - want)
    print("D = %d: largest error / bound per coefficient %s" % (D, np.array2string((err / bound).max(axis=1), precision=3)))
    assert (err <= bound).all(), (err, bound)
    assert bound[1].max() < 0.6 / D ** 2 and bound[2:].max() < 45.0 / D, "O(1 / D^2) on the stratified axis, O(1 / D) elsewhere"


@pytest.mark.parametrize("D", [64, 4096])
def test_the_cosine_set_about_plus_y_integrates_the_sky(D):
    e = G.irradiance64(G.sky, (0.0, 1.0, 0.0), D)
    want = np.pi * (1.0 / 6.0 + 5.0 / 6.0 * COL)
    assert np.allclose(want, sky_irradiance((0, 1, 0)), atol=1e-14)
    assert (np.abs(e - want) <= cosine_bound((0, 1, 0), D)).all(), (e - want, cosine_bound((0, 1, 0), D))
    w = G.hemisphere64((0.0, 1.0, 0.0), D)
    a, _ = G.set64(D)
    assert np.allclose(w[:, 1], np.sqrt(1.0 - a / 2.0), atol=1e-15), "omega_y is the stratified coordinate's alone"


# ------------------------------------------------------------------------------------- 3. sh_irradiance
@pytest.mark.parametrize("D", [64, 4096])
def test_sh_irradiance_against_the_cosine_set(D):
    """The sky has no band above 1, so the band-2 record convolves to its irradiance exactly, up to the two quadratures: the sum
    of their bounds, the probe's through the band factors and |Y_k(n)|."""
    sh = G.probe64(G.sky, D)
    band = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
    for n in ((0, 1, 0), (0, -1, 0), (1, 0, 0), (0, 0, -1), (0.6, 0.48, -0.64), (-0.3, -0.9, 0.1)):
        n = np.asarray(n, np.float64) / np.linalg.norm(n)
        from_sh = abi.sh_irradiance(sh, n)
        from_set = G.irradiance64(G.sky, n, D)
        bound_sh = (band[:, None] * np.abs(G.basis64(n))[:, None] * probe_bounds(D)).sum(axis=0) + 2e-5  # (the six-decimal constants enter twice, each within 1.8e-6 of its value: 3.6e-6 of at most 1.25 pi)
        assert (np.abs(from_sh - sky_irradiance(n)) <= bound_sh).all(), (n, from_sh - sky_irradiance(n), bound_sh)
        assert (np.abs(from_set - sky_irradiance(n)) <= cosine_bound(n, D)).all(), (n, from_set - sky_irradiance(n), cosine_bound(n, D))
        assert (np.abs(from_sh - from_set) <= bound_sh + cosine_bound(n, D)).all()
    # broadcasting: many records, many normals
    many = abi.sh_irradiance(np.stack([sh, 2.0 * sh]), np.array([[0.0, 1.0, 0.0], [0.0, 1.0, 0.0]]))
    assert many.shape == (2, 3) and np.allclose(many[1], 2.0 * many[0])


# ------------------------------------------------------------------------------------- 4. the surface
def test_symbols_signatures_and_the_abi_version(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB_PATH], text=True)
    exported = set(re.findall(r" T (pt_[a-z0-9_]+)", out))
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "ptrace_sys.rs")).read()
    for name in NAMES:
        assert name in exported and hasattr(lib, name) and name in SIGNATURES and name in ADDED_WITHIN_ABI_5, name
        h = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        r = re.search(r"pub fn %s\(([^)]*)\)" % name, rust)
        assert h and r
        args_h = [a.split()[-1].lstrip("*") for a in h.group(1).split(",")]
        args_r = [a.split(":")[0].strip() for a in r.group(1).split(",")]
        assert args_h == args_r == ["ctx", "points" if name == NAMES[0] else "probes", "n", "directions", "n_passes", "out"]
        assert len(SIGNATURES[name][1]) == 6
    assert lib.pt_abi_version() == 5 == abi.PT_ABI_VERSION and re.search(r"#define\s+PT_ABI_VERSION\s+5\b", header)
    assert "pt_gather_kernel" not in exported, "the kernels' accessor stays inside the library"


def test_the_structs_match_the_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "ptrace.h"
int main(void){
 printf("%zu %zu %zu ", sizeof(PtGatherPoint), offsetof(PtGatherPoint, position), offsetof(PtGatherPoint, normal));
 printf("%zu %zu %zu ", sizeof(PtIrradiance), offsetof(PtIrradiance, e), offsetof(PtIrradiance, samples));
 printf("%zu %zu %zu\n", sizeof(PtProbeSH), offsetof(PtProbeSH, sh), offsetof(PtProbeSH, samples));
 return 0; }'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got == [32, 0, 16, 16, 0, 12, 112, 0, 108]
    assert got == [C.sizeof(abi.PtGatherPoint), abi.PtGatherPoint.position.offset, abi.PtGatherPoint.normal.offset,
                   C.sizeof(abi.PtIrradiance), abi.PtIrradiance.e.offset, abi.PtIrradiance.samples.offset,
                   C.sizeof(abi.PtProbeSH), abi.PtProbeSH.sh.offset, abi.PtProbeSH.samples.offset]
    rust = open(os.path.join(ROOT, "bindings", "rust", "ptrace_sys.rs")).read()
    for name, fields in (("PtGatherPoint", ["position", "_pad0", "normal", "_pad1"]), ("PtIrradiance", ["e", "samples"]), ("PtProbeSH", ["sh", "samples"])):
        body = re.search(r"pub struct %s \{(.*?)\n\}" % name, rust, flags=re.S).group(1)
        assert re.findall(r"pub (\w+):", body) == fields
    assert "pub sh: [[f32; 3]; 9]" in rust


def test_the_header_carries_the_contract():
    text = " ".join(open(HEADER).read().split())
    for phrase in ("a = float(2 j + 1) / float(D)", "u = float(((j * 0x9E3779B97F4A7C15) mod 2^64) >> 40) * 2^-24", "y = 1 - a; r2 = fma(-y, y, 1); r = sqrt(r2); omega = (r * c, y, r * s)",
                   "h = a * 0.5; sh = sqrt(h); lx = sh * c; ly = sh * s; m = 1 - h; lz = sqrt(m)", "omega.k = fma(z.k, lz, fma(bt.k, ly, t.k * lx))",
                   "mean.c = r_j.sum.c / r_j.samples", "v[l] = v[l] + v[l xor o]", "no floating-point atomic is used",
                   "e.c = v.c * (3.14159265f / float(D))", "sh[k].c = v[k].c * (12.5663706f / float(D))", "Y6 = 0.315392f * fma(3, z * z, -1)",
                   "samples == 0 is the mark", "D is a multiple of 64 in [64, 4096], and n * D is at most 2^32 - 1", "calls pt_query_radiance(ctx, rays, n * D, n_passes, rec) ONCE"):
        assert phrase in text, phrase


def test_the_error_wording_and_their_order_in_the_source():
    api = open(os.path.join(ROOT, "ray_tracer_webgl_amd", "csrc", "pt_api.hip")).read()
    body = api[api.index("static int passes_ready("):api.index("static int radiance_batch(")] + api[api.index("static int gather_ready("):api.index("PT_API int pt_gather_irradiance")]
    order = ["n_passes == 0", "passes > %u reserved", "query_ready(c, who", "passes_ready(c, who", "directions (a multiple of 64 in", "are more than 2^32 - 1 rays",
             "estimator_ready(c, who", "static int gather_batches(", "c->gather.fit(e)", "call(ptsig::GatherRays{}", "static int gather(", "gather_ready(c, who", "return gather_batches("]
    at = [body.index(s) for s in order]
    assert at == sorted(at), "pt_query_radiance's checks in its order, then directions, then the workspace, then the first launch"
    assert api.count("directions (a multiple of 64 in") == api.count("are more than 2^32 - 1 rays") == api.count("passes > %u reserved (pt_reserve_passes)\", who") == 1, "stated once"
    assert "unknown key %d" in api and not re.search(r"#define\s+PT_OPT_\w+\s+14\b", open(HEADER).read()), "no new option key"
    assert 14 not in [v for k, v in vars(abi).items() if k.startswith("PT_OPT_")]


def test_errors_that_need_no_device(lib):
    pts, out = (abi.PtGatherPoint * 2)(), (abi.PtProbeSH * 2)()
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn(None, pts, 2, 64, 1, out) == abi.PT_ERR_INVALID and fn(None, None, 0, 0, 0, None) == abi.PT_ERR_INVALID
    assert not bytes(out).strip(b"\0")


def test_counts_and_batches(shim):
    for D in range(0, 4300):
        assert bool(shim.gth_directions_valid(D)) == G.directions_valid(D) == (D % 64 == 0 and 64 <= D <= 4096), D
    assert shim.gth_total_rays(67108863, 64) == 67108863 * 64 and shim.gth_total_rays(67108864, 64) == 0 and shim.gth_total_rays(1048576, 4096) == 0
    assert shim.gth_total_rays(1048575, 4096) == 1048575 * 4096
    # a batch of B rays (any first ray, any D) touches at most B / 64 + 2 items
    for B in (1, 63, 64, 240, 512, 777):
        worst = max((first + B - 1) // D - first // D + 1 for D in (64, 128, 4096) for first in range(0, 3 * D))
        assert worst <= shim.gth_items_per_batch(B) == B // 64 + 2, (B, worst)


def item_span(shim, first, m, D):
    out = (C.c_uint32 * 4)()
    shim.gth_item_span(first, m, D, out)
    return tuple(out)


def span_by_enumeration(first, m, D):
    """{item0, items, done0, done1} of the batch of rays [first, first + m), ray by ray: the items the rays belong to, and those
    whose last ray is among them (a range from the first item touched on: an item that started earlier ends first)"""
    rays = np.arange(first, first + m, dtype=np.uint64)
    items = rays // np.uint64(D)
    done = items[rays % np.uint64(D) == D - 1]
    assert (np.diff(items) <= 1).all() and (len(done) == 0 or done[0] == items[0])
    return int(items[0]), int(items[-1] - items[0]) + 1, int(items[0]), int(items[0]) + len(done)


def test_the_item_span_of_every_batch_equals_the_enumeration(shim):
    """csrc/pt_gather.hpp item_span, which sizes what a gather batch stages, reduces and copies (pt_api.hip gather_batches):
    every batch of calls of 1 to 5 items over the planes and direction counts below, ray by ray; and the bound that keeps the
    staged points and records inside GatherSet::work — never more items than plane / kMinDirections + 2, GatherSet::items'
    own expression."""
    assert "return e.pix / ptgather::kMinDirections + 2;" in open(os.path.join(ROOT, "ray_tracer_webgl_amd", "csrc", "pt_buffers.hpp")).read()
    most = 0
    for plane in (64, 72, 100, 4096):
        for D in (64, 128, 256, 4096):
            for n in range(1, 6):
                for first in range(0, n * D, plane):
                    m = min(plane, n * D - first)
                    got = item_span(shim, first, m, D)
                    assert got == span_by_enumeration(first, m, D), (plane, D, n, first)
                    assert got[1] <= plane // abi.PT_GATHER_MIN_DIRECTIONS + 2 == shim.gth_items_per_batch(plane), (plane, D, n, first)
                    most = max(most, got[1] - plane // 64)
    assert most == 2, "the bound is met: whole items and a straddling one at either end"
    assert abi.PT_GATHER_MIN_DIRECTIONS == 64
    # an item that straddles two batches (item 1 of D = 64 over planes of 100): touched by both, ends in the second
    assert item_span(shim, 0, 100, 64) == (0, 2, 0, 1)
    # ... whose first item only reads the carry and whose last only writes it: items 1 .. 3, of which 1 and 2 end
    assert item_span(shim, 100, 100, 64) == (1, 3, 1, 3)
    # an item that fills a whole batch and ends in neither it nor the one before: nothing is written
    assert item_span(shim, 64, 64, 256) == (0, 1, 0, 0) and item_span(shim, 128, 64, 256) == (0, 1, 0, 0) and item_span(shim, 192, 64, 256) == (0, 1, 0, 1)
    # a short last batch: 28 rays of 2 items of 64 over planes of 100
    assert item_span(shim, 100, 28, 64) == (1, 1, 1, 2)
    # the last batch of the largest call there is (67108863 items of 64: 2^32 - 64 rays) over planes of 4096 ...
    total = 67108863 * 64
    first = (total - 1) // 4096 * 4096
    assert first + (total - first) > 2 ** 32 - 1 - 64
    assert item_span(shim, first, total - first, 64) == (first // 64, 63, first // 64, 67108863) == span_by_enumeration(first, total - first, 64)
    # ... and a batch that ends at ray 2^32 itself: first + m in 32 bits would be 0
    assert item_span(shim, 2 ** 32 - 64, 64, 64) == (2 ** 26 - 1, 1, 2 ** 26 - 1, 2 ** 26)
    assert item_span(shim, 2 ** 32 - 100, 99, 4096) == (2 ** 20 - 1, 1, 2 ** 20 - 1, 2 ** 20 - 1)


def test_the_workspace_is_in_place_or_refused(shim):
    s = shim.set_new()
    try:
        assert shim.set_in_place(s, 240) == 0 and shim.alloc_live() == 0
        shim.alloc_fail_at(1)
        assert shim.set_fit(s, 240) == 1 and shim.set_in_place(s, 240) == 0 and shim.set_capacity(s) == 0 and shim.alloc_live() == 0
        shim.alloc_fail_at(0)
        assert shim.set_fit(s, 240) == 0 and shim.set_in_place(s, 240) == 1
        k = 240 // 64 + 2
        assert shim.set_capacity(s) == 2 * 64 * 28 + 36 * k and 4 * shim.set_capacity(s) == 14336 + 144 * k
        lay = (C.c_uint64 * 3)()
        shim.set_layout(s, 240, lay)
        assert list(lay) == [3584, 3584 + 8 * k, 3584 + 36 * k] and all(v % 4 == 0 for v in lay), "16-byte aligned parts"
        slots = (C.c_uint64 * 4)()
        shim.set_carry_slots(s, slots)
        assert list(slots) == [0, 1792, 0, 1792], "two carry slots of 64 x 28 floats, taken by batch parity: never one slot in one launch"
        assert shim.set_in_place(s, 100) == 1 and shim.set_fit(s, 100) == 0 and shim.set_capacity(s) == 2 * 64 * 28 + 36 * k, "a smaller extent keeps the buffer"
        assert shim.set_in_place(s, 512) == 0
        shim.alloc_fail_at(1)   # growing: the old buffer is freed first, the refused one leaves nothing
        assert shim.set_fit(s, 512) == 1 and shim.set_capacity(s) == 0 and shim.set_in_place(s, 100) == 0 and shim.alloc_live() == 0
        shim.alloc_fail_at(0)
        assert shim.set_fit(s, 512) == 0 and shim.set_in_place(s, 512) == 1 and shim.alloc_live() == 1
        shim.set_release(s)
        assert shim.alloc_live() == 0 and shim.set_in_place(s, 1) == 0
    finally:
        shim.set_delete(s)
