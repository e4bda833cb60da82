"""pt_query_radiance_nee, pt_gather_irradiance_nee and pt_bake_probes_nee on the CPU (include/ptrace.h has the contract): the
restatement tests/radiance_nee_ref.py the device tests compare with, and the surface of the three entry points.

  1. the scaffold     with the light sample disabled, and with it enabled over a scene without lights, the restatement IS
                      tests/radiance_ref.records — equal uint32 views, equal segment totals;
  2. the expectation  the two-light room, 64 rays: the per-sample terms of the plain and of the lit restatement, block means
                      within 5 standard errors of their difference; less variance per sample; a first segment that ends on the
                      lamp adds the lamp's emission;
  3. the gather       tests/gather_ref.reduce_item over the lit records; with the light sample disabled, gather_ref.gather;
  4. the surface      the exported symbols, header / ctypes / Rust argument lists, the ABI version, no new option key, the side
                      table of csrc/pt_rad_nee_table.hpp through tests/rad_nee_shim.cpp, kNeeKernels and the 14 x 7 table as
                      they were;
  5. the errors that need no device.
CPU only."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import gather_ref as G
import nee_ref
import nee_scenes
import query_ref as Q
import radiance_nee_ref as RN
import radiance_ref as RR
from ray_tracer_webgl_amd import abi
from ray_tracer_webgl_amd._lib import ADDED_WITHIN_ABI_5, LIB_PATH, SIGNATURES
from ray_tracer_webgl_amd.tracer import PathTracer
from test_gpu_ray_queries import SplitMix64

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "ptrace.h")
CSRC = os.path.join(ROOT, "ray_tracer_webgl_amd", "csrc")
F = np.float32
NAMES = ("pt_query_radiance_nee", "pt_gather_irradiance_nee", "pt_bake_probes_nee")
ROWS = ["list_lds", "scalar", "scalar_nolds", "small_t0", "small_t1", "small_t2", "small_t3", "bvh", "bvh_nodes", "bvh_gmem", "grid", "grid_cells",
        "grid_gmem", "grid_layers"]
VARIANTS = ["small_t0", "small_t1", "small_t2", "small_t3", "scalar", "scalar_nolds", "bvh", "bvh_nodes", "bvh_gmem", "grid", "grid_cells", "grid_gmem"]
SERVES = {"list_lds": "scalar", "grid_layers": "grid"}


def read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def settings(p, spp=2, depth=6):
    q = p.copy()
    q.samples_per_pixel, q.max_depth, q.first_pass, q.time_step = spp, depth, 0, abi.PT_TIME_STEP_DECORRELATED
    return q


def mixed_rays(sph, p, n_bounce, n_inside, seed):
    """the context's pinhole rays, bounce-style rays from their hit points and rays from inside spheres"""
    o, d = Q.pinhole_rays(p)
    first = Q.records(sph, p, o, d)
    pts = first["point"][first["index"] >= 0]
    rng = SplitMix64(seed)
    bo, bd = pts[(np.arange(n_bounce) * 3) % len(pts)], rng.unit(n_bounce)
    io, idir = sph["center"][(np.arange(n_inside) * 7 + 1) % len(sph)].astype(F), rng.unit(n_inside)
    return np.concatenate([o, bo, io]), np.concatenate([d, bd, idir])


# ------------------------------------------------------------------------------------- 1. the scaffold
@pytest.mark.parametrize("make", [lambda: nee_scenes.two_light_room(16, 9, 2, 2, 6), lambda: nee_scenes.random_lit(2, 11, 3, width=16, height=9)],
                         ids=["two_light_room", "random_lit"])
def test_without_the_light_sample_the_restatement_is_the_plain_one(make):
    sc = make()
    p = settings(sc.params)
    o, d = mixed_rays(sc.spheres, p, 40, 10, 0x3200 + len(sc.spheres))
    assert len(o) > RR.batch(p), "two batches"
    plain, seg = RR.records(sc.spheres, p, o, d, 2)
    assert not RR.has_nan(plain)
    got, seg_got, shadow = RN.records(sc.spheres, p, o, d, 2, light_sample=False)
    assert shadow == 0 and seg_got == seg, (seg_got, seg)
    assert np.array_equal(RN.raw(got), RR.raw(plain))
    # the light sample enabled over a scene without lights: L == 0, no draw, nothing skipped
    unlit = nee_scenes.without_lights(sc).spheres
    assert nee_ref.lights_of(unlit) == []
    plain, seg = RR.records(unlit, p, o, d, 2)
    got, seg_got, shadow = RN.records(unlit, p, o, d, 2)
    assert shadow == 0 and seg_got == seg and np.array_equal(RN.raw(got), RR.raw(plain))
    # ... and over the lit scene the light sample is at work
    lit, seg_lit, shadow = RN.records(sc.spheres, p, o, d, 2)
    assert shadow > 0 and seg_lit > shadow and not np.array_equal(RN.raw(lit), RR.raw(RR.records(sc.spheres, p, o, d, 2)[0]))
    assert (RN.raw(lit)[:, 3] == RR.raw(plain)[:, 3]).all(), "the samples and the invalid marks are the namesake's"


def test_invalid_rays_give_zeros_and_no_segment():
    sc = nee_scenes.two_light_room(16, 9, 2, 2, 6)
    o, d = Q.invalid_rays()
    rec, seg, shadow = RN.records(sc.spheres, settings(sc.params), o, d, 3)
    assert not RN.raw(rec).any() and seg == 0 and shadow == 0


# ------------------------------------------------------------------------------------- 2. the expectation
def room_rays():
    """64 rays in the two-light room: 48 pinhole rays of an 8 x 6 view (some end on the lamp), 16 bounce-style rays from the walls"""
    sc = nee_scenes.two_light_room(8, 6, 48, 4, 6)
    p = settings(sc.params, spp=48)
    o, d = Q.pinhole_rays(p)
    first = Q.records(sc.spheres, p, o, d)
    pts = first["point"][first["type"] == abi.PT_DIFFUSE]
    rng = SplitMix64(0x3264)
    o, d = np.concatenate([o, pts[(np.arange(16) * 5) % len(pts)]]), np.concatenate([d, rng.unit(16)])
    assert len(o) == 64
    return sc, p, o, d


def test_same_expectation_less_variance_and_the_first_segment_sees_the_lamp():
    """Per ray 4 passes of 48 chained samples each way.  Per channel, the mean over all 64 rays and over each block of 16 rays of
    the two estimators differ by at most 5 standard errors of the difference, from both sides' per-sample variances (the bound
    and the statistic of tests/test_nee_ref.py's block-wise test)."""
    sc, p, o, d = room_rays()
    n_passes = 4
    stats = {}
    for on in (False, True):
        per = {}
        rec, seg, shadow = RN.records(sc.spheres, p, o, d, n_passes, light_sample=on, per_sample=per)
        terms = np.asarray([per[i] for i in range(64)])  # (64 rays, 192 samples, 3)
        assert terms.shape == (64, n_passes * 48, 3) and not RN.has_nan(rec)
        stats[on] = (terms.mean(axis=1), terms.var(axis=1, ddof=1) / terms.shape[1], seg, shadow, rec, terms.var(axis=1, ddof=1))
    assert stats[False][3] == 0 and stats[True][3] > 0
    worst = 0.0
    for blocks in (4, 1):
        m = [s[0].reshape(blocks, 64 // blocks, 3).mean(axis=1) for s in (stats[False], stats[True])]
        v = [s[1].reshape(blocks, 64 // blocks, 3).sum(axis=1) / (64 // blocks) ** 2 for s in (stats[False], stats[True])]
        z = np.abs(m[0] - m[1]) / np.sqrt(np.maximum(v[0] + v[1], 1e-300))
        worst = max(worst, float(z.max()))
        assert (z <= 5.0).all(), (blocks, z)
    print("plain %s against next-event %s; worst |difference| / standard error %.2f; segments %d against %d (%d shadow)" % (
        stats[False][0].mean(axis=0), stats[True][0].mean(axis=0), worst, stats[False][2], stats[True][2], stats[True][3]))
    # the point of it: less variance per sample along these rays
    assert stats[True][5].mean() < stats[False][5].mean()
    # a first segment that ends on the lamp: no light sample precedes it, so its record holds the lamp's emission — every sample
    lamp = 8
    first = Q.records(sc.spheres, p, o, d)
    on_lamp = np.flatnonzero(first["index"] == lamp)
    assert len(on_lamp) >= 1 and sc.spheres[lamp]["type"] == abi.PT_EMISSIVE
    e = sc.spheres[lamp]["albedo"].astype(F)
    want = np.zeros(3, F)
    for _ in range(n_passes):
        s = np.zeros(3, F)
        for _ in range(48):
            s = s + e
        want = want + s
    for on in (False, True):
        for i in on_lamp:
            assert np.array_equal(stats[on][4][i, :3].view(np.uint32), want.view(np.uint32)) and stats[on][4][i, 3] == n_passes * 48


# ------------------------------------------------------------------------------------- 3. the gather sentence
def test_the_gather_calls_are_the_reduce_over_the_lit_records():
    sc = nee_scenes.two_light_room(16, 9, 2, 2, 6)
    p = settings(sc.params)
    pos = F([[0.0, -0.99, 0.2], [0.6, 0.0, 0.1], [np.nan, 0.0, 0.0]])
    nrm = F([[0.0, 1.0, 0.0], [-3.0, 0.5, 0.25], [0.0, 1.0, 0.0]])
    D = 64
    for kind, normals in ((G.IRRADIANCE, nrm), (G.PROBE, None)):
        out, seg, shadow, rec = RN.gather(sc.spheres, p, kind, pos, normals, D, 2)
        o, d = G.rays(kind, pos, normals, D)
        rec2, seg2, shadow2 = RN.records(sc.spheres, p, o, d, 2)
        assert np.array_equal(RN.raw(rec), RN.raw(rec2)) and (seg, shadow) == (seg2, shadow2) and shadow > 0
        for i in range(2):
            assert np.array_equal(G.raw(out[i]), G.raw(G.reduce_item(kind, rec2[i * D:(i + 1) * D], D)))
        assert not G.raw(out[2]).any() and not RN.raw(rec[2 * D:]).any(), "an invalid item: null rays, a zero record"
        assert out[0, -1] == D * 2 * 2
        # the light sample disabled: gather_ref.gather, bit for bit
        plain, seg_plain, rec_plain = G.gather(sc.spheres, p, kind, pos, normals, D, 2)
        off, seg_off, shadow_off, rec_off = RN.gather(sc.spheres, p, kind, pos, normals, D, 2, light_sample=False)
        assert shadow_off == 0 and seg_off == seg_plain and np.array_equal(G.raw(off), G.raw(plain)) and np.array_equal(RN.raw(rec_off), RR.raw(rec_plain))
        assert not np.array_equal(G.raw(out), G.raw(plain))


# ------------------------------------------------------------------------------------- 4. the surface
def test_the_three_symbols_are_exported_and_declared_alike(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB_PATH], text=True)
    exported = set(re.findall(r" T (pt_[a-z0-9_]+)", out))
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    rust = read("bindings", "rust", "ptrace_sys.rs")
    for name in NAMES:
        plain = name[:-len("_nee")]
        assert name in exported and hasattr(lib, name) and name in SIGNATURES and name in ADDED_WITHIN_ABI_5, name
        h, hp = (re.search(r"\bint %s\(([^)]*)\);" % n, header) for n in (name, plain))
        r, rp = (re.search(r"pub fn %s\(([^)]*)\) -> c_int;" % n, rust) for n in (name, plain))
        assert h and hp and r and rp, name
        assert h.group(1) == hp.group(1) and r.group(1) == rp.group(1), "the namesake's argument list"
        args_h = [a.split()[-1].lstrip("*") for a in h.group(1).split(",")]
        args_r = [a.split(":")[0].strip() for a in r.group(1).split(",")]
        assert args_h == args_r and len(args_h) == len(SIGNATURES[name][1]) and SIGNATURES[name] == SIGNATURES[plain]
    assert "pt_rad_nee_kernel" not in exported and "pt_nee_kernel" not in exported, "the kernels' accessors stay inside the library"
    assert lib.pt_abi_version() == 5 == abi.PT_ABI_VERSION and re.search(r"#define\s+PT_ABI_VERSION\s+5\b", header)


def test_no_option_key_was_added():
    hdr = read("include", "ptrace.h")
    keys = {k: int(v) for k, v in re.findall(r"\b(PT_OPT_[A-Z_]+) = (\d+),", hdr)}
    assert keys["PT_OPT_NEXT_EVENT"] == 13 == max(keys.values()) and len(set(keys.values())) == len(keys)
    mine = {k: v for k, v in vars(abi).items() if k.startswith("PT_OPT_") and isinstance(v, int)}
    assert max(mine.values()) == 13 and 14 not in mine.values()
    assert 'return fail(c, PT_ERR_INVALID, "pt_set_option: unknown key %d", key);' in read("ray_tracer_webgl_amd", "csrc", "pt_api.hip")
    assert "stay the plain estimator" in " ".join(hdr.split()) and "pt_query_radiance_nee" in hdr


def test_the_python_keyword_defaults_to_the_plain_call():
    import inspect

    for method in (PathTracer.query_radiance, PathTracer.gather_irradiance, PathTracer.bake_probes):
        assert inspect.signature(method).parameters["next_event"].default is False, method.__name__


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(tempfile.mkdtemp(prefix="rad_nee_"), "librad_nee_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", os.path.join(HERE, "rad_nee_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    cell = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
    lib.rn_cell.argtypes = lib.rn_nee_cell.argtypes = [C.c_int] + cell
    lib.rn_table_cell.argtypes = [C.c_int, C.c_int] + cell
    return lib


def _cell(fn, *where):
    obj, kid, waves, sym = C.c_int(), C.c_int(), C.c_int(), C.c_char_p()
    assert fn(*where, C.byref(obj), C.byref(kid), C.byref(waves), C.byref(sym)) == 0
    return obj.value, kid.value, waves.value, sym.value.decode()


def test_the_side_table(shim):
    assert shim.rn_rows() == len(ROWS) == 14 and shim.rn_builds() == 7 and shim.rn_variants() == 12
    assert shim.rn_obj_count() == 7 == shim.rn_obj_nee() and shim.rn_obj_rad_nee() == 8, "behind the seven objects of the trace table and OBJ_NEE"
    names = set()
    for row, name in enumerate(ROWS):
        v = SERVES.get(name, name)
        obj, kid, waves, sym = _cell(shim.rn_cell, row)
        assert sym == "pt_trace_kernel_%s_rad_nee" % v and obj == shim.rn_obj_rad_nee() and kid == VARIANTS.index(v)
        # the waves: the statement the kernels' attribute reads, of the row's radiance cell — the _nee build's figure: five for the
        # two walks whose shadow state does not fit at six, the namesake's elsewhere
        # (the LDS list walk has no variants: its launches are steered to the scalar row, whose cell the side table repeats)
        r_obj, r_kid, r_waves, r_sym = _cell(shim.rn_table_cell, ROWS.index("scalar") if name == "list_lds" else row, shim.rn_build_rad())
        assert r_kid == kid and r_sym == "pt_trace_kernel_%s_rad" % v
        assert waves == shim.rn_waves(kid, r_waves) == (5 if v in ("bvh_nodes", "grid_cells") else r_waves), (name, waves, r_waves)
        # kNeeKernels as it was
        n_obj, n_kid, n_waves, n_sym = _cell(shim.rn_nee_cell, row)
        assert (n_obj, n_kid, n_waves, n_sym) == (7, kid, waves, "pt_trace_kernel_%s_nee" % v)
        names.add(sym)
    assert len(names) == 12
    assert shim.rn_cell(14, None, None, None, None) == 1 and shim.rn_cell(-1, None, None, None, None) == 1
    for on in (0, 1):
        for build in range(7):
            assert shim.rn_takes_cell(on, build) == int(on == 1 and build == shim.rn_build_rad() == 6)
            assert shim.rn_takes_nee_cell(on, build) == int(on == 1 and build == 0)
    assert shim.rn_reads_ring(shim.rn_row_grid(), shim.rn_build_rad()) == 0, "the _rad_nee build of the row `grid` gets the plain cell array"
    # the 14 x 7 table: every cell's object is one of the seven, its name the row's kernel under the column's suffix
    suffix = ["", "_rr", None, "_dbg", "_feat", "_qry", "_rad"]
    for row, name in enumerate(ROWS):
        for build in range(7):
            obj, kid, waves, sym = _cell(shim.rn_table_cell, row, build)
            assert 0 <= obj < 7 and "nee" not in sym
            if build == 0:
                assert sym == ("pt_trace_kernel" if name == "list_lds" else "pt_trace_kernel_" + name)
            elif suffix[build] is not None and name != "list_lds":
                assert sym == "pt_trace_kernel_%s%s" % (SERVES.get(name, name), suffix[build])
    # the kernels are defined from the same rows, with the same statement for their waves
    unit = read("ray_tracer_webgl_amd", "csrc", "pt_kernels_radiance_nee.hip")
    assert "PT_VARIANT_ROWS(PT_RAD_NEE_VARIANT, _rad_nee, RadNee)" in unit and "PT_VARIANT_ACCESSOR(pt_rad_nee_kernel, _rad_nee, RadNee)" in unit
    assert "pt_rad_nee_waves(PT_VARIANT_ID(stem), waves)" in unit and "pt_rad_nee_waves(PT_VARIANT_ID(stem), waves)" in read("ray_tracer_webgl_amd", "csrc", "pt_rad_nee_table.hpp")
    assert "template <class Row> using RadNee = Nee<Rad<Row>>;" in read("ray_tracer_webgl_amd", "csrc", "pt_trace_body.hpp")
    extra = read("ray_tracer_webgl_amd", "csrc", "pt_extra.h")
    objects = extra[extra.index("#define PT_TRACE_OBJECTS(X)"):extra.index("#define PT_TRACE_ACCESSOR_DECL")]
    assert "nee" not in objects.lower() and 'extern "C" const void* pt_rad_nee_kernel(int id);' in extra
    assert "pt_kernels_radiance_nee.hip" in read("ray_tracer_webgl_amd", "csrc", "Makefile")


def test_the_launch_text_that_must_stay_and_the_transport():
    api = read("ray_tracer_webgl_amd", "csrc", "pt_api.hip")
    assert "const bool nee = !door && c->lights.on;" in api and "takes_nee_cell(nee, build)" in api and "takes_rad_nee_cell(rad_nee, build)" in api
    assert "static_assert(!NEE || (!RR && !DBG && !FEAT && !COUNT)" in read("ray_tracer_webgl_amd", "csrc", "pt_shade.hpp")
    # one body each: the estimator is a parameter
    assert api.count("static int query_radiance(") == 1 and api.count("static int gather(") == 1
    body = api[api.index("static int query_radiance("):api.index("PT_API int pt_query_radiance(")]
    order = ["query_ready(c, who", "passes_ready(c, who", "estimator_ready(c, who, next_event)", "stage_rays(", "radiance_batch(c, who, next_event"]
    at = [body.index(s) for s in order]
    assert at == sorted(at), "the namesake's checks in its order, then the option"
    passes = api[api.index("static int passes_ready("):api.index("static int radiance_batch(")]
    assert passes.index("n_passes == 0") < passes.index("passes > %u reserved")
    # one batch body for both estimators and both families: the estimator reaches the launch through it
    batch = api[api.index("static int radiance_batch("):api.index("static int query_radiance(")]
    assert "use.next_event = next_event;" in batch and api.count("use.next_event = next_event;") == 1 and batch.index("trace_once(") < batch.index("call(ptsig::RadianceFold{}")
    body = api[api.index("static int gather_ready("):api.index("PT_API int pt_gather_irradiance")]
    order = ["query_ready(c, who", "passes_ready(c, who", "directions (a multiple of 64 in", "are more than 2^32 - 1 rays", "estimator_ready(c, who, next_event)",
             "static int gather_batches(", "c->gather.fit(e)", "call(ptsig::GatherRays{}", "radiance_batch(c, who, next_event", "static int gather(", "gather_ready(c, who, next_event",
             "return gather_batches("]
    at = [body.index(s) for s in order]
    assert at == sorted(at)
    assert '"next-event estimation is off (pt_set_option PT_OPT_NEXT_EVENT)"' in api and '"ray queries are off (pt_set_option PT_OPT_RAY_QUERIES)"' in api
    # PtKernelArgs keeps its layout; the note on where the table travels stands beside the two on uuid
    args = read("ray_tracer_webgl_amd", "csrc", "pt_kernel_args.h")
    assert "slot_uuid" in args and "dbg_cursor[0]" in args and "_rad_nee" in args


# ------------------------------------------------------------------------------------- 5. errors that need no device
def test_errors_that_need_no_device(lib):
    """(a context needs a device: PT_OK for n == 0 is asserted in tests/test_gpu_radiance_nee.py; a NULL context is refused
    first, as the namesakes refuse it)"""
    rays, rec = (abi.PtRay * 2)(), (abi.PtRayRadiance * 2)()
    fn = lib.pt_query_radiance_nee
    assert fn(None, rays, 2, 1, rec) == abi.PT_ERR_INVALID and fn(None, None, 0, 0, None) == abi.PT_ERR_INVALID
    assert fn(None, rays, 2, 1, rec) == lib.pt_query_radiance(None, rays, 2, 1, rec)
    pts, out = (abi.PtGatherPoint * 2)(), (abi.PtProbeSH * 2)()
    for name in NAMES[1:]:
        fn = getattr(lib, name)
        assert fn(None, pts, 2, 64, 1, out) == abi.PT_ERR_INVALID and fn(None, None, 0, 0, 0, None) == abi.PT_ERR_INVALID
    assert not bytes(out).strip(b"\0") and not bytes(rec).strip(b"\0")
