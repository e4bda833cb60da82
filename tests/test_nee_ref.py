"""Next-event estimation on the CPU (PT_OPT_NEXT_EVENT; include/ptrace.h has the contract): the restatement tests/nee_ref.py the
device tests compare with, and csrc/pt_nee.hpp, which the kernels compile.

  1. the scaffold     with the light sample disabled the restatement IS ora_ray_color, bit for bit, segment counts included;
  2. the arithmetic   csrc/pt_nee.hpp through tests/nee_shim.cpp equals the restatement's numpy statements bit for bit over the
                      sweep of tests/nee_sweep.hpp, and the light table over lists with every kind of sphere that is no light;
                      tests/nee_main.cpp walks the same sweep under the sanitizers;
  3. the weight       its mean over 2^16 fixed draws against (r / d)^2 cos(theta) for an unoccluded light above the horizon;
  4. the expectation  the restatement with and without the light sample on a closed room with two lights;
  5. the option       exclusions and keys in the source, the side table's cells, the header's and the Rust binding's symbols.
CPU only."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import nee_ref
import nee_scenes
from ray_tracer_webgl_amd import abi, scenes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ray_tracer_webgl_amd", "csrc")
F = np.float32
ROWS = ["list_lds", "scalar", "scalar_nolds", "small_t0", "small_t1", "small_t2", "small_t3", "bvh", "bvh_nodes", "bvh_gmem", "grid", "grid_cells",
        "grid_gmem", "grid_layers"]
VARIANTS = ["small_t0", "small_t1", "small_t2", "small_t3", "scalar", "scalar_nolds", "bvh", "bvh_nodes", "bvh_gmem", "grid", "grid_cells", "grid_gmem"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(tempfile.mkdtemp(prefix="nee_"), "libnee_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror", os.path.join(HERE, "nee_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    fp, u32 = C.POINTER(C.c_float), C.c_uint32
    lib.nee_lights.restype, lib.nee_lights.argtypes = u32, [C.POINTER(abi.PtSphere), u32, C.c_void_p]
    lib.nee_choose.restype, lib.nee_choose.argtypes = C.c_int, [C.c_float, C.c_int]
    lib.nee_sample.restype, lib.nee_sample.argtypes = None, [fp, fp, fp, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float, fp]
    lib.nee_add.restype, lib.nee_add.argtypes = None, [fp, fp, fp, C.c_float]
    lib.nee_sweep_count.restype = u32
    lib.nee_sweep_read.restype, lib.nee_sweep_read.argtypes = None, [fp]
    lib.nee_cell.restype = C.c_int
    lib.nee_cell.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
    lib.nee_rr_name.restype = C.c_char_p
    lib.alloc_fail_at.argtypes = [C.c_long]
    lib.alloc_live.restype = C.c_long
    lib.set_new.restype = C.c_void_p
    for f in (lib.set_delete, lib.set_in_place, lib.set_n, lib.set_capacity):
        f.argtypes = [C.c_void_p]
    lib.set_on.argtypes = [C.c_void_p, C.c_int]
    lib.set_fit.argtypes = [C.c_void_p, u32]
    lib.set_n.restype = u32
    lib.set_capacity.restype = C.c_uint64
    return lib


def f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


# ------------------------------------------------------------------------------------- 1. the scaffold
def _random_scene():
    from test_gpu_fuzz import random_scene

    sc = random_scene(np.random.default_rng(88123), 14, 32, 18, 2, 8, 2)
    sc.spheres["uuid"] = np.arange(len(sc.spheres))
    return sc


@pytest.mark.parametrize("make", [lambda: scenes.default_scene(32, 18, spp=2, max_depth=8, n_passes=2), lambda: scenes.config4(32, 18, 2, 2, 8), _random_scene],
                         ids=["default", "config4", "random"])
def test_without_the_light_sample_the_restatement_is_the_oracle(ora, make):
    sc = make()
    for lens in (0.0, 0.05):
        p = sc.params.copy()
        p.lens_radius = lens
        p.time_step = abi.PT_TIME_STEP_DECORRELATED
        ref, seg = ora.render(sc.spheres, p, 2, nthreads=4)
        got, seg_got, shadow = nee_ref.render(sc.spheres, p, 2, light_sample=False)
        assert shadow == 0 and seg_got == seg, (seg_got, seg)
        assert np.array_equal(bits(got), bits(ref))
    # one row band
    p.band_rows, p.band_index, p.band_count = 4, 1, 3
    ref, seg = ora.render(sc.spheres, p, 2, nthreads=4)
    got, seg_got, _ = nee_ref.render(sc.spheres, p, 2, light_sample=False)
    assert seg_got == seg and np.array_equal(bits(got), bits(ref))


def test_a_scene_without_lights_is_the_oracle_with_the_light_sample_on(ora):
    sc = nee_scenes.without_lights(scenes.config4(32, 18, 2, 2, 8))
    assert nee_ref.lights_of(sc.spheres) == []
    ref, seg = ora.render(sc.spheres, sc.params, 2, nthreads=4)
    got, seg_got, shadow = nee_ref.render(sc.spheres, sc.params, 2)
    assert shadow == 0 and seg_got == seg and np.array_equal(bits(got), bits(ref))


# ------------------------------------------------------------------------------------- 2. the arithmetic
def _sweep(shim):
    n = shim.nee_sweep_count()
    buf = np.zeros((n, 14), np.float32)
    shim.nee_sweep_read(buf.ctypes.data_as(C.POINTER(C.c_float)))
    return buf


def test_the_header_equals_the_restatement_over_the_sweep(ora, shim):
    cases = _sweep(shim)
    assert len(cases) > 2000
    out = (C.c_float * 8)()
    seen = {"P": 0, "notP": 0, "om0": 0, "cos+": 0, "cos-": 0, "cos0": 0, "pole": 0, "edge_hi": 0, "edge_lo": 0, "L": set(), "last_bin": 0}
    for row in cases:
        x, n, c, r2, L = row[0:3], row[3:6], row[6:9], F(row[9]), int(row[10])
        u0, u1, u2 = F(row[11]), F(row[12]), F(row[13])
        k = shim.nee_choose(float(u0), L)
        assert k == nee_ref.choose(u0, L) and 0 <= k < L, (u0, L, k)
        seen["L"].add(L)
        seen["last_bin"] += int(k == L - 1 and u0 >= F(1.0) - F(2.0 ** -24))
        s, co = C.c_float(), C.c_float()
        ora.load().ora_sincos2pi(C.c_float(float(u2)), C.byref(s), C.byref(co))
        shim.nee_sample(f3(x), f3(n), f3(c), float(r2), L, float(u1), s.value, co.value, out)
        ok, w, d2 = nee_ref.reach(x, c, r2)
        assert bool(out[0]) == ok and F(out[1]).view(np.uint32) == d2.view(np.uint32), row
        seen["P" if ok else "notP"] += 1
        if not ok:
            seen["edge_hi"] += int(d2 == r2)
            continue
        seen["edge_lo"] += int(np.nextafter(r2, F(np.inf)) == d2)
        omega, om = nee_ref.sample(w, d2, r2, u1, F(s.value), F(co.value))
        cos_s = nee_ref.cos_at(n, omega)
        wgt = nee_ref.weight(L, om, cos_s)
        want = np.array([omega[0], omega[1], omega[2], om, cos_s, wgt], np.float32)
        got = np.array(out[2:8], np.float32)
        assert np.array_equal(bits(got), bits(want)), (row, got, want)
        assert np.isfinite(want).all()
        seen["om0"] += int(om == 0 and wgt == 0)
        seen["cos+"] += int(cos_s > 0)
        seen["cos-"] += int(cos_s < 0)
        seen["cos0"] += int(cos_s == 0)
        seen["pole"] += int(w[0] == 0 and w[1] == 0 and w[2] < 0)
    assert seen["L"] >= {1, 2, 65} and all(seen[k] > 0 for k in seen if k != "L"), seen
    # the add: one product, one product, one sum per channel
    sm, t, a = f3((0.5, 0.25, 0.125)), f3((0.3, 0.6, 0.9)), f3((4.0, 3.0, 2.0))
    shim.nee_add(sm, t, a, 0.37)
    for ch in range(3):
        want = F((0.5, 0.25, 0.125)[ch]) + (F((0.3, 0.6, 0.9)[ch]) * F((4.0, 3.0, 2.0)[ch])) * F(0.37)
        assert F(sm[ch]).view(np.uint32) == want.view(np.uint32)


def test_the_light_table_keeps_out_what_is_no_light(shim):
    """list order, r * r of a negative radius, and outside the table: another type, a NaN or infinite centre, a zero, infinite
    or NaN radius, a NaN or infinite albedo"""
    sc = scenes.config4(32, 18, 2, 2, 8)
    base = sc.spheres[8].copy()
    assert base["type"] == abi.PT_EMISSIVE
    sph = np.zeros(12, abi.SPHERE_DTYPE)
    sph[:] = base
    sph[0]["type"] = abi.PT_DIFFUSE
    sph[1]["radius"] = -0.75
    sph[2]["center"][1] = np.nan
    sph[3]["center"][2] = np.inf
    sph[4]["radius"] = 0.0
    sph[5]["radius"] = np.inf
    sph[6]["radius"] = np.nan
    sph[7]["albedo"][0] = np.nan
    sph[8]["albedo"][2] = -np.inf
    sph[9]["type"] = 9
    sph[10]["center"] = (1.0, 2.0, 3.0)
    sph[11]["radius"] = -0.0
    sph["uuid"] = np.arange(12)
    want = nee_ref.lights_of(sph)
    assert [l[3] for l in want] == [1, 10]
    ptr, n, keep = abi.spheres_as_ctypes(sph)
    out = np.zeros((12, 8), np.float32)
    assert shim.nee_lights(ptr, n, out.ctypes.data_as(C.c_void_p)) == 2
    for k, (c, r2, alb, i) in enumerate(want):
        assert np.array_equal(bits(out[k, 0:3]), bits(c)) and bits(out[k, 3:4])[0] == r2.view(np.uint32)
        assert np.array_equal(bits(out[k, 4:7]), bits(alb)) and int(out[k, 7:8].view(np.int32)[0]) == i
    assert out[0, 3] == np.float32(0.5625)
    assert shim.nee_lights(ptr, 0, out.ctypes.data_as(C.c_void_p)) == 0


def test_the_light_set_is_in_place_or_refused(shim):
    s = shim.set_new()
    try:
        assert shim.set_fit(s, 3) == 0 and not shim.set_in_place(s) and shim.set_capacity(s) == 0  # off: never built
        shim.set_on(s, 1)
        assert not shim.set_in_place(s)
        assert shim.set_fit(s, 0) == 0 and shim.set_in_place(s) and shim.set_n(s) == 0 and shim.set_capacity(s) == 1
        assert shim.set_fit(s, 5) == 0 and shim.set_in_place(s) and shim.set_n(s) == 5 and shim.set_capacity(s) == 5
        assert shim.set_fit(s, 2) == 0 and shim.set_n(s) == 2 and shim.set_capacity(s) == 5  # it only grows
        shim.alloc_fail_at(1)
        assert shim.set_fit(s, 9) == 1 and not shim.set_in_place(s) and shim.set_n(s) == 0 and shim.set_capacity(s) == 0
        shim.alloc_fail_at(0)
        assert shim.set_fit(s, 9) == 0 and shim.set_in_place(s) and shim.set_n(s) == 9
        shim.set_on(s, 0)
        assert not shim.set_in_place(s) and shim.set_capacity(s) == 0 and shim.alloc_live() == 0
    finally:
        shim.set_delete(s)


def test_header_under_address_and_undefined_behaviour_sanitizers():
    """tests/nee_main.cpp: a stand-alone program (its own main) over csrc/pt_nee.hpp on exactly sized heap lists and the sweep,
    built with -fsanitize=address,undefined and run as a child; nothing sanitized is loaded into this process"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "nee_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                               os.path.join(HERE, "nee_main.cpp"), "-o", exe])
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and "nee: ok" in out.stdout, out.stdout[-2000:]


# ------------------------------------------------------------------------------------- 3. the weight
@pytest.mark.parametrize("geometry", [((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 2.0, 0.0), 0.5),       # overhead
                                      ((0.3, -1.0, 0.2), (0.0, 1.0, 0.0), (1.5, 0.5, -0.7), 0.6),     # oblique, large
                                      ((0.0, 0.0, 0.0), (0.6, 0.0, 0.8), (0.4, 0.3, 3.0), 0.3)],       # a tenth of its distance
                         ids=["overhead", "oblique", "far"])
def test_the_mean_weight_is_the_lights_form_factor(ora, shim, geometry):
    """E[2 (1 - cosmax) cos_s] over the cone = (1 / pi) * integral of cos over the sphere's solid angle = (r / d)^2 cos(theta) for a
    sphere wholly above the horizon of n.  2^16 draws (u1, u2) from a fixed sequence; the bound is 5 standard errors of the mean,
    from the draws' own variance.  (The geometries keep r / d at a tenth and above: 1 - cosmax is an fp32 difference with an
    absolute error of about 2^-24, a RELATIVE error of 2^-24 / (1 - cosmax) in every weight — 1e-5 at r / d = 0.1, below these
    standard errors, 4e-4 at r / d = 0.016, where the same test reads 7.7 standard errors: the contract's own rounding, DESIGN.md
    §4.8m.)"""
    x, n, c, r = geometry
    x, n, c = np.asarray(x, np.float64), np.asarray(n, np.float64), np.asarray(c, np.float64)
    d = np.linalg.norm(c - x)
    cos_theta = float(np.dot(n, (c - x) / d))
    assert cos_theta * d > r  # wholly above the horizon
    want = (r / d) ** 2 * cos_theta
    rng = np.random.default_rng(20240613)
    u = rng.random((1 << 16, 2)).astype(np.float32)
    out = (C.c_float * 8)()
    L = ora.load()
    s, co = C.c_float(), C.c_float()
    xs, ns, cs, r2 = f3(x), f3(n), f3(c), float(F(r) * F(r))
    w = np.zeros(len(u))
    for i in range(len(u)):
        L.ora_sincos2pi(C.c_float(float(u[i, 1])), C.byref(s), C.byref(co))
        shim.nee_sample(xs, ns, cs, r2, 1, float(u[i, 0]), s.value, co.value, out)
        assert out[0] == 1.0 and out[6] > 0.0
        w[i] = out[7]
    mean, se = w.mean(), w.std(ddof=1) / np.sqrt(len(w))
    print("mean weight %.6f against %.6f: %.2f standard errors of %.2e" % (mean, want, abs(mean - want) / se, se))
    assert abs(mean - want) <= 5.0 * se, (mean, want, se)


# ------------------------------------------------------------------------------------- 4. the expectation
def test_the_light_sample_keeps_the_expectation():
    """The two-light room (tests/nee_scenes.py: a lamp half hidden behind a diffuse sphere, and a dome that contains every
    diffuse surface point, so !P occurs), 8 x 8 pixels, 448 samples per pixel each way.  Per channel, the frame mean and each
    4 x 4 block mean of the two estimators differ by at most 5 standard errors of the difference, computed from both sides'
    per-sample variances."""
    w = h = 8
    spp = 448
    sc = nee_scenes.two_light_room(w, h, spp, 1, 6)
    lights = nee_ref.lights_of(sc.spheres)
    assert len(lights) == 2
    stats = {}
    for on in (False, True):
        r = nee_ref.Restatement(sc.spheres, sc.params, light_sample=on)
        mean = np.zeros((h, w, 3))
        var = np.zeros((h, w, 3))
        for y in range(h):
            for x in range(w):
                per = []
                r.pixel_pass(x, y, F(sc.params.time), per_sample=per)
                per = np.asarray(per)
                mean[y, x], var[y, x] = per.mean(axis=0), per.var(axis=0, ddof=1) / spp
        stats[on] = (mean, var, r.segments, r.shadow_segments)
    assert stats[False][3] == 0 and stats[True][3] > 0
    # !P occurred: some light samples chose the dome, from inside it
    dome = lights[0]
    assert not nee_ref.reach(np.zeros(3, F), dome[0], dome[1])[0]
    worst = 0.0
    for blocks in ((2, 2), (1, 1)):
        by, bx = h // blocks[0], w // blocks[1]
        m = [s[0].reshape(blocks[0], by, blocks[1], bx, 3).mean(axis=(1, 3)) for s in (stats[False], stats[True])]
        v = [s[1].reshape(blocks[0], by, blocks[1], bx, 3).sum(axis=(1, 3)) / (by * bx) ** 2 for s in (stats[False], stats[True])]
        z = np.abs(m[0] - m[1]) / np.sqrt(v[0] + v[1])
        worst = max(worst, float(z.max()))
        assert (z <= 5.0).all(), (blocks, z)
    print("plain %s against next-event %s; worst |difference| / standard error %.2f; segments %d against %d (%d shadow)" % (
        stats[False][0].mean(axis=(0, 1)), stats[True][0].mean(axis=(0, 1)), worst, stats[False][2], stats[True][2], stats[True][3]))
    # the point of it: less variance per sample in this room
    assert stats[True][1].mean() < stats[False][1].mean()


# ------------------------------------------------------------------------------------- 5. the option
def read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_the_key_and_its_exclusions_in_the_source():
    api = read("ray_tracer_webgl_amd", "csrc", "pt_api.hip")
    hdr = read("include", "ptrace.h")
    assert re.search(r"PT_OPT_NEXT_EVENT = 13,", hdr) and abi.PT_OPT_NEXT_EVENT == 13 and abi.BUILD_NEXT_EVENT == 16
    # key 14 is still nobody's: the unknown-key answer is untouched
    assert not re.search(r"PT_OPT_\w+ = 14\b", hdr)
    assert 'return fail(c, PT_ERR_INVALID, "pt_set_option: unknown key %d", key);' in api
    # the three exclusions, both ways round, worded like the existing pairs
    for a, b in (("PT_OPT_NEXT_EVENT", "PT_OPT_RUSSIAN_ROULETTE"), ("PT_OPT_RUSSIAN_ROULETTE", "PT_OPT_NEXT_EVENT"),
                 ("PT_OPT_NEXT_EVENT", "the debug overlay"), ("the debug overlay", "PT_OPT_NEXT_EVENT"),
                 ("PT_OPT_NEXT_EVENT", "PT_OPT_COUNT_WORK"), ("PT_OPT_COUNT_WORK", "PT_OPT_NEXT_EVENT")):
        assert re.search(r'"pt_set_(option|debug_overlay): %s and %s exclude each other \(turn ' % (re.escape(a), re.escape(b)), api), (a, b)
    # the doors stay the plain estimator; the side table's cell only where the column is the plain build
    assert "const bool nee = !door && c->lights.on;" in api and "takes_nee_cell(nee, build)" in api
    # no _nee build reads a uuid: the table travels there
    shade = read("ray_tracer_webgl_amd", "csrc", "pt_shade.hpp")
    assert "static_assert(!NEE || (!RR && !DBG && !FEAT && !COUNT)" in shade


def test_the_side_table(shim):
    assert shim.nee_rows() == len(ROWS) == 14
    assert shim.nee_build_value() == abi.BUILD_NEXT_EVENT >= shim.nee_build_count() == 7
    serves = {"list_lds": "scalar", "grid_layers": "grid"}
    names = set()
    for row, name in enumerate(ROWS):
        obj, kid, waves, sym = C.c_int(), C.c_int(), C.c_int(), C.c_char_p()
        assert shim.nee_cell(row, C.byref(obj), C.byref(kid), C.byref(waves), C.byref(sym)) == 0
        v = serves.get(name, name)
        assert sym.value.decode() == "pt_trace_kernel_%s_nee" % v
        assert obj.value == shim.nee_obj_count() == 7  # behind the seven objects of the trace table
        assert kid.value == VARIANTS.index(v) == shim.nee_rr_id(row) if name != "list_lds" else kid.value == VARIANTS.index("scalar")
        assert shim.nee_rr_name(row).decode() == ("pt_trace_kernel_%s_rr" % v if name != "list_lds" else "pt_trace_kernel")
        # the waves: the namesake's, five for the two walks whose shadow state does not fit at six
        plain = shim.nee_plain_waves(row if name != "list_lds" else ROWS.index("scalar"))
        assert waves.value == (5 if v in ("bvh_nodes", "grid_cells") else plain), (name, waves.value, plain)
        names.add(sym.value.decode())
    assert len(names) == 12
    assert shim.nee_cell(14, None, None, None, None) == 1 and shim.nee_cell(-1, None, None, None, None) == 1
    for on in (0, 1):
        for build in range(7):
            assert shim.nee_takes_cell(on, build) == int(on == 1 and build == 0)
    # the kernels are defined from the same rows: the code object's twelve symbols
    unit = read("ray_tracer_webgl_amd", "csrc", "pt_kernels_nee.hip")
    assert "PT_VARIANT_ROWS(PT_NEE_VARIANT, _nee, Nee)" in unit and "PT_VARIANT_ACCESSOR(pt_nee_kernel, _nee, Nee)" in unit
    extra = read("ray_tracer_webgl_amd", "csrc", "pt_extra.h")
    objects = extra[extra.index("#define PT_TRACE_OBJECTS(X)"):extra.index("#define PT_TRACE_ACCESSOR_DECL")]
    assert "nee" not in objects.lower() and 'extern "C" const void* pt_nee_kernel(int id);' in extra
    assert "pt_kernels_nee.hip" in read("ray_tracer_webgl_amd", "csrc", "Makefile")


def test_header_python_and_rust_name_the_same_values():
    src = '#include <stdio.h>\n#include "ptrace.h"\nint main(void) { printf("%d\\n", (int)PT_OPT_NEXT_EVENT); return 0; }\n'
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        assert int(subprocess.check_output([exe], text=True)) == abi.PT_OPT_NEXT_EVENT == 13
    rust = read("bindings", "rust", "ptrace_sys.rs")
    assert re.search(r"pub const PT_OPT_NEXT_EVENT: c_int = 13;", rust) and re.search(r"pub const PT_BUILD_NEXT_EVENT: c_int = 16;", rust)
    table = read("ray_tracer_webgl_amd", "csrc", "pt_nee_table.hpp")
    assert "enum { BUILD_NEXT_EVENT = 16 };" in table
    # the layers above
    assert "def next_event(self, on=True):" in read("ray_tracer_webgl_amd", "tracer.py")
    assert "next_event=False" in read("ray_tracer_webgl_amd", "app.py") and '"--next-event"' in read("ray_tracer_webgl_amd", "render.py")
