"""GATHER QUERIES (include/ptrace.h pt_gather_irradiance, pt_bake_probes), restated in numpy float32 from the header's statement
list: the direction set (ora_sincos2pi from the oracle's exports, libm's fmaf, numpy's correctly rounded `/` and sqrt), the rays
of the defining sentence, tests/radiance_ref.records for their records, and the reduction in its stated order — 64 lanes, each
ascending in j, then the xor tree.  It shares no source with csrc/pt_gather.hpp (tests/test_gather_ref.py compares the two bit
for bit).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import ctypes.util

import numpy as np

import radiance_ref as RR
from oracle import oracle

F = np.float32
IRRADIANCE, PROBE = 0, 1
LANES = 64
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = C.c_float
_libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]
_fma = np.frompyfunc(lambda a, b, c: _libm.fmaf(float(a), float(b), float(c)), 3, 1)
Y_CONST = (F(0.282095), F(0.488603), F(1.092548), F(0.315392), F(0.546274))
PI_F, FOUR_PI_F = F(3.14159265), F(12.5663706)


def fma(a, b, c):
    """fmaf element by element: one rounding"""
    with np.errstate(all="ignore"):
        return np.asarray(_fma(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F)), dtype=np.float64).astype(F)


def directions_valid(D):
    return 64 <= D <= 4096 and D % 64 == 0


def stratum(j, D):
    """a = float(2 j + 1) / float(D)"""
    return (2 * np.asarray(j, np.uint32) + 1).astype(F) / F(D)


def turn(j):
    """u = float(((j * 0x9E3779B97F4A7C15) mod 2^64) >> 40) * 2^-24"""
    with np.errstate(over="ignore"):
        h = np.atleast_1d(np.asarray(j, np.uint64)) * np.uint64(0x9E3779B97F4A7C15)  # (wraps at 2^64)
    return (h >> np.uint64(40)).astype(F) * F(2.0 ** -24)


def sincos(u):
    """(sin, cos) of 2 pi u by ora_sincos2pi, element by element"""
    L = oracle.load()
    u = np.atleast_1d(np.asarray(u, F))
    s, c = np.zeros(len(u), F), np.zeros(len(u), F)
    a, b = C.c_float(), C.c_float()
    for k, v in enumerate(u):
        L.ora_sincos2pi(C.c_float(float(v)), C.byref(a), C.byref(b))
        s[k], c[k] = a.value, b.value
    return s, c


_SET = {}


def the_set(D):
    """(a, s, c) of j = 0 .. D - 1: made once per D"""
    if D not in _SET:
        j = np.arange(D)
        s, c = sincos(turn(j))
        _SET[D] = (stratum(j, D), s, c)
    return _SET[D]


def sphere_directions(D):
    """(D, 3) float32: the probe's set"""
    a, s, c = the_set(D)
    y = F(1.0) - a
    r = np.sqrt(fma(-y, y, F(1.0)))
    return np.stack([r * c, y, r * s], axis=1)


def unit_normal(n):
    n = np.asarray(n, F)
    with np.errstate(all="ignore"):
        ax, ay, az = np.abs(n)
        gxy = ax if ax > ay else ay
        g = gxy if gxy > az else az
        p = n / g
        d2 = fma(p[2], p[2], fma(p[1], p[1], p[0] * p[0]))
        i = F(1.0) / np.sqrt(d2)
        return p * i


def hemisphere_directions(normal, D):
    """(D, 3) float32: the cosine-weighted set about a valid normal"""
    a, s, c = the_set(D)
    z = unit_normal(normal)
    with np.errstate(all="ignore"):
        h = a * F(0.5)
        sh = np.sqrt(h)
        lx, ly = sh * c, sh * s
        lz = np.sqrt(F(1.0) - h)
        zx, zy, zz = z
        sg = F(np.copysign(F(1.0), zz))
        q = -F(1.0) / (sg + zz)
        b = (zx * zy) * q
        t = (fma(sg * (zx * zx), q, F(1.0)), sg * b, -sg * zx)
        bt = (b, fma(zy * zy, q, sg), -zy)
        return np.stack([fma(z[k], lz, fma(bt[k], ly, t[k] * lx)) for k in range(3)], axis=1)


def sh_basis(w):
    """(..., 9) float32 of directions (..., 3)"""
    w = np.asarray(w, F)
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    k0, k1, k2, k3, k4 = Y_CONST
    with np.errstate(all="ignore"):
        return np.stack([np.full_like(x, k0), k1 * y, k1 * z, k1 * x, k2 * (x * y), k2 * (y * z), k3 * fma(F(3.0), z * z, F(-1.0)), k2 * (x * z),
                         k4 * fma(x, x, -(y * y))], axis=-1)


def item_valid(kind, position, normal):
    position, normal = np.asarray(position, F), np.asarray(normal, F)
    if not np.isfinite(position).all():
        return False
    return kind == PROBE or bool(np.isfinite(normal).all() and (normal != 0).any())


def rays(kind, positions, normals, D):
    """the n * D rays of the defining sentence: (origins, directions), ray j of item i at i * D + j; an invalid item's are null"""
    positions = np.asarray(positions, F).reshape(-1, 3)
    n = len(positions)
    normals = np.zeros((n, 3), F) if normals is None else np.asarray(normals, F).reshape(-1, 3)
    o, d = np.zeros((n, D, 3), F), np.zeros((n, D, 3), F)
    for i in range(n):
        if not item_valid(kind, positions[i], normals[i]):
            continue
        o[i] = positions[i]
        d[i] = sphere_directions(D) if kind == PROBE else hemisphere_directions(normals[i], D)
    return o.reshape(-1, 3), d.reshape(-1, 3)


def tree(v):
    """(64, A): for o = 32 .. 1, v[l] = v[l] + v[l xor o]; the item's sums are v[0]"""
    lanes = np.arange(LANES)
    with np.errstate(all="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[lanes ^ o]
    return v[0]


def reduce_item(kind, rec, D):
    """the item's record from its D records (D, 4): 4 floats {e, samples} or 28 {sh[9][3], samples}"""
    rec = np.asarray(rec, F).reshape(D, 4)
    Y = sh_basis(sphere_directions(D)) if kind == PROBE else None
    acc = np.zeros((LANES, 28 if kind == PROBE else 4), F)
    with np.errstate(all="ignore"):
        for r in range(D // LANES):
            j = r * LANES + np.arange(LANES)
            mean = rec[j, :3] / rec[j, 3:4]
            if kind == PROBE:
                for k in range(9):
                    for c in range(3):
                        acc[:, 3 * k + c] = fma(mean[:, c], Y[j, k], acc[:, 3 * k + c])
            else:
                acc[:, :3] = acc[:, :3] + mean
            acc[:, -1] = acc[:, -1] + rec[j, 3]
        v = tree(acc)
        scale = (FOUR_PI_F if kind == PROBE else PI_F) / F(D)
        out = v.copy()
        out[:-1] = v[:-1] * scale
    return out


def gather(spheres, params, kind, positions, normals, D, n_passes):
    """((n, 4 or 28) float32 records, segments, the n * D radiance records): the whole call by the defining sentence"""
    positions = np.asarray(positions, F).reshape(-1, 3)
    n = len(positions)
    normals = np.zeros((n, 3), F) if normals is None else np.asarray(normals, F).reshape(-1, 3)
    o, d = rays(kind, positions, normals, D)
    rec, seg = RR.records(spheres, params, o, d, n_passes)
    out = np.zeros((n, 28 if kind == PROBE else 4), F)
    for i in range(n):
        if item_valid(kind, positions[i], normals[i]):
            out[i] = reduce_item(kind, rec[i * D:(i + 1) * D], D)
    return out, seg, rec


def raw(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- float64 quadrature of the same set (no fp32 statement: the real-arithmetic set of the header) ------------------------
def set64(D):
    """(a, phi) in float64; phi from the same 24-bit turn (exact in float64)"""
    j = np.arange(D)
    return (2.0 * j + 1.0) / D, 2.0 * np.pi * turn(j).astype(np.float64)


def sphere64(D):
    a, phi = set64(D)
    y = 1.0 - a
    r = np.sqrt(1.0 - y * y)
    return np.stack([r * np.cos(phi), y, r * np.sin(phi)], axis=1)


def hemisphere64(normal, D):
    a, phi = set64(D)
    z = np.asarray(normal, np.float64)
    z = z / np.linalg.norm(z)
    sg = np.copysign(1.0, z[2])
    q = -1.0 / (sg + z[2])
    b = z[0] * z[1] * q
    t = np.array([1.0 + sg * z[0] * z[0] * q, sg * b, -sg * z[0]])
    bt = np.array([b, sg + z[1] * z[1] * q, -z[1]])
    u = a / 2.0
    lx, ly, lz = np.sqrt(u) * np.cos(phi), np.sqrt(u) * np.sin(phi), np.sqrt(1.0 - u)
    return lx[:, None] * t + ly[:, None] * bt + lz[:, None] * z


def basis64(w):
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    return np.stack([0.282095 * np.ones_like(x), 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * x * y, 1.092548 * y * z,
                     0.315392 * (3.0 * z * z - 1.0), 1.092548 * x * z, 0.546274 * (x * x - y * y)], axis=-1)


def probe64(radiance, D):
    """(9, 3) float64: (4 pi / D) sum_j L(omega_j) Y_k(omega_j) for a radiance function of (D, 3) directions -> (D, 3)"""
    w = sphere64(D)
    return (4.0 * np.pi / D) * np.einsum("jk,jc->kc", basis64(w), radiance(w))


def irradiance64(radiance, normal, D):
    return (np.pi / D) * radiance(hemisphere64(normal, D)).sum(axis=0)


def sky(w):
    """the shader's sky gradient for unit directions: (1 - t)(1, 1, 1) + t (0.5, 0.7, 1), t = (w.y + 1) / 2"""
    t = 0.5 * (w[..., 1:2] + 1.0)
    return (1.0 - t) * np.ones(3) + t * np.array([0.5, 0.7, 1.0])
