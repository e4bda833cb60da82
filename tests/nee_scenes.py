"""Scenes with light sources for the next-event tests (tests/test_nee_ref.py on the CPU, tests/test_gpu_next_event.py on the
device).  Every scene carries unique uuids: tests/nee_ref.py finds a hit's list index through them."""
import numpy as np

from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.scenes import PT_DIFFUSE, PT_EMISSIVE, PT_GLASS, PT_METAL, _base_params, _lib, _look_at, _pack, _sphere


def two_light_room(width, height, spp, n_passes, max_depth):
    """A closed room with two lights.  Five huge diffuse spheres are its walls; the side behind the camera is open onto a DOME:
    a large dim emissive sphere around everything, camera included — every diffuse surface point lies inside it, so the light
    cannot be sampled from anywhere (!P) and is found the plain way.  The LAMP is a small bright sphere under the ceiling, half
    hidden behind a diffuse sphere; a glass and a metal sphere stand on the floor (arrivals after GLASS and METAL add emission
    as always)."""
    R = 1000.0
    items = [
        _sphere((-(R + 1.0), 0.0, 0.0), R, PT_DIFFUSE, (0.65, 0.05, 0.05)),
        _sphere(((R + 1.0), 0.0, 0.0), R, PT_DIFFUSE, (0.12, 0.45, 0.15)),
        _sphere((0.0, -(R + 1.0), 0.0), R, PT_DIFFUSE, (0.73, 0.73, 0.73)),
        _sphere((0.0, (R + 1.0), 0.0), R, PT_DIFFUSE, (0.73, 0.73, 0.73)),
        _sphere((0.0, 0.0, -(R + 1.0)), R, PT_DIFFUSE, (0.73, 0.73, 0.73)),
        _sphere((0.0, 0.0, 0.0), 30.0, PT_EMISSIVE, (0.4, 0.5, 0.7)),          # the dome
        _sphere((-0.45, -0.65, 0.3), 0.35, PT_GLASS, (1.0, 1.0, 1.0), ri=1.5),
        _sphere((0.45, -0.6, -0.3), 0.4, PT_METAL, (0.8, 0.85, 0.88), fuzz=0.05),
        _sphere((0.25, 0.6, -0.2), 0.25, PT_EMISSIVE, (12.0, 11.0, 9.0)),       # the lamp
        _sphere((-0.05, 0.35, 0.0), 0.3, PT_DIFFUSE, (0.6, 0.6, 0.2)),          # ... and what half hides it
    ]
    p = _base_params(spp, max_depth, background=abi.PT_BG_BLACK)
    _look_at(_lib(), p, width, height, (0.0, 0.0, 3.6), (0.0, 0.0, 0.0), 40.0, 0.0, 3.6)
    return scenes.Scene("two_light_room", _pack(items), p, n_passes, "closed room, a lamp and a dome")


def with_lights(sc, indices, albedo=(6.0, 5.0, 4.0)):
    """the scene with the spheres at `indices` turned into lights (a copy)"""
    sph = sc.spheres.copy()
    for k, i in enumerate(indices):
        sph[i]["type"] = abi.PT_EMISSIVE
        sph[i]["albedo"] = np.asarray(albedo, np.float32) * np.float32(1.0 + 0.25 * k)
    sph["uuid"] = np.arange(len(sph))
    out = scenes.Scene(sc.name + "_lit", sph, sc.params.copy(), sc.n_passes, sc.note)
    return out


def without_lights(sc):
    """the scene with every emissive sphere turned diffuse (a copy): L == 0"""
    sph = sc.spheres.copy()
    sph["type"][sph["type"] == abi.PT_EMISSIVE] = abi.PT_DIFFUSE
    sph["albedo"] = np.minimum(sph["albedo"], np.float32(0.9))
    sph["uuid"] = np.arange(len(sph))
    return scenes.Scene(sc.name + "_unlit", sph, sc.params.copy(), sc.n_passes, sc.note)


def random_lit(seed, n, n_lights, width=64, height=36, spp=2, depth=6, passes=2):
    """tests/test_gpu_fuzz.py's random scene of n spheres with exactly n_lights emissive ones (duplicates, concentric and
    negative-radius spheres, cameras inside spheres, lens on and off among them), unique uuids"""
    from test_gpu_fuzz import random_scene

    rng = np.random.default_rng(88000 + seed)
    sc = random_scene(rng, n, width, height, spp, depth, passes)
    sph = sc.spheres
    em = sph["type"] == abi.PT_EMISSIVE
    sph["type"][em] = abi.PT_DIFFUSE
    sph["albedo"][em] = np.float32(0.5)
    for k in rng.choice(n, size=min(n_lights, n), replace=False):
        sph[k]["type"] = abi.PT_EMISSIVE
        sph[k]["albedo"] = rng.uniform(1, 8, 3).astype(np.float32)
        if abs(float(sph[k]["radius"])) > 5.0:
            sph[k]["radius"] = np.float32(0.7)
    sph["uuid"] = np.arange(n)
    return sc
