"""AddressSanitizer + UBSan over the CPU-side native code (the oracle and the host half of the
C ABI, csrc/pt_host.cpp).  GPU sanitizers are not available on the pool, so the device code is
covered by the parity tests instead; this catches out-of-bounds / UB in the C and C++ host paths."""
import os
import shutil
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib(name):
    p = subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_oracle_and_host_code_under_asan_ubsan(tmp_path):
    asan, ubsan = _lib("libasan.so"), _lib("libubsan.so")
    if not asan or not ubsan:
        pytest.skip("sanitizer runtimes not installed")
    san = ["-O1", "-g", "-fPIC", "-shared", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    ora_so = str(tmp_path / "libpt_oracle_asan.so")
    host_so = str(tmp_path / "libpt_host_asan.so")
    subprocess.check_call(["gcc", "-std=c11", "-march=x86-64-v3", "-fno-builtin-sin", "-fno-builtin-cos"] + san +
                          [os.path.join(ROOT, "oracle", "pt_oracle.c"), "-o", ora_so, "-lm", "-lpthread"])
    subprocess.check_call(["g++", "-std=c++17"] + san +
                          [os.path.join(ROOT, "ray_tracer_webgl_amd", "csrc", "pt_host.cpp"), "-o", host_so])
    grid_so = str(tmp_path / "libgrid_class_shim_asan.so")  # ptgrid::build at any margin class (tests/grid_class_shim.cpp)
    subprocess.check_call(["g++", "-std=c++17"] + san + [os.path.join(ROOT, "tests", "grid_class_shim.cpp"), "-o", grid_so])
    script = textwrap.dedent('''
        import ctypes as C, sys
        import numpy as np
        sys.path.insert(0, %r)
        from ray_tracer_webgl_amd import abi
        O = C.CDLL(%r); H = C.CDLL(%r); G = C.CDLL(%r)
        fp = C.POINTER(C.c_float)
        # host: State lifecycle, movement with autofocus, uniforms, scene narrowing, pick ray
        h = C.c_void_p()
        H.pt_state_create.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32]
        assert H.pt_state_create(C.byref(h), 96, 54) == 0
        H.pt_state_set_camera_angles.argtypes = [C.c_void_p, C.c_double, C.c_double]
        H.pt_state_set_keys.argtypes = [C.c_void_p, C.c_uint32]
        H.pt_state_update_position.argtypes = [C.c_void_p, C.c_double]
        H.pt_state_set_lens.argtypes = [C.c_void_p, C.c_double, C.c_double]
        H.pt_state_spheres.argtypes = [C.c_void_p, C.POINTER(abi.PtSphere), C.c_uint32]
        H.pt_state_to_params.argtypes = [C.c_void_p, C.c_double, C.POINTER(abi.PtParams)]
        H.pt_state_destroy.argtypes = [C.c_void_p]
        for i in range(64):
            H.pt_state_set_camera_angles(h, -90.0 + 3 * i, (i %% 50) - 25.0)
            H.pt_state_set_keys(h, i)
            H.pt_state_update_position(h, 16.0)
            H.pt_state_set_lens(h, 0.05 * (i %% 3), 1.0)
        sp = (abi.PtSphere * 16)()
        n = H.pt_state_spheres(h, sp, 16)
        p = abi.PtParams()
        assert H.pt_state_to_params(h, 3.0, C.byref(p)) == 0
        p.band_rows, p.band_index, p.band_count = 4, 1, 3
        p.samples_per_pixel, p.max_depth = 2, 6
        # oracle: a banded, windowed, multi-threaded render of that state + read-out paths
        O.ora_local_rows.restype = C.c_uint32
        O.ora_local_rows.argtypes = [C.POINTER(abi.PtParams)]
        rows = O.ora_local_rows(C.byref(p))
        acc = np.zeros((rows, p.width, 4), np.float32)
        O.ora_render_passes.restype = C.c_uint64
        O.ora_render_passes.argtypes = [C.POINTER(abi.PtSphere), C.c_uint32, C.POINTER(abi.PtParams), C.c_uint32, fp] + [C.c_uint32] * 5
        seg = O.ora_render_passes(sp, n, C.byref(p), 2, acc.ctypes.data_as(fp), 3, p.width - 5, 0, p.height, 3)
        # ... and the same render with the Russian roulette of PT_OPT_RUSSIAN_ROULETTE after two bounces: fewer segments
        O.ora_render_passes_rr.restype = C.c_uint64
        O.ora_render_passes_rr.argtypes = O.ora_render_passes.argtypes + [C.c_int32]
        acc_rr = np.zeros_like(acc)
        seg_rr = O.ora_render_passes_rr(sp, n, C.byref(p), 2, acc_rr.ctypes.data_as(fp), 3, p.width - 5, 0, p.height, 3, 2)
        assert 0 < seg_rr < seg and np.isfinite(acc_rr).all() and not np.array_equal(acc_rr, acc)
        out = np.empty_like(acc)
        O.ora_resolve.argtypes = [fp, C.c_size_t, C.c_uint32, C.c_int, fp]
        O.ora_resolve(acc.ctypes.data_as(fp), acc.size // 4, 4, 1, out.ctypes.data_as(fp))
        px = np.empty((rows, p.width, 4), np.uint8)
        O.ora_resolve_rgba8.argtypes = [fp, C.c_size_t, C.c_uint32, C.c_int, C.c_void_p]
        O.ora_resolve_rgba8(acc.ctypes.data_as(fp), acc.size // 4, 4, 1, px.ctypes.data_as(C.c_void_p))
        assert seg > 0 and np.isfinite(out[:, 3:p.width - 5]).all()
        H.pt_state_destroy(h)
        # host: the hierarchy builder (binned SAH, outliers, binary16 packing) on awkward scenes
        from ray_tracer_webgl_amd import scenes
        vp = C.c_void_p
        H.pt_build_bvh.argtypes = [C.POINTER(abi.PtSphere), C.c_uint32, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t,
                                   vp, vp, vp, C.c_size_t, C.POINTER(C.c_float), vp, C.c_size_t]
        rng = np.random.default_rng(3)
        cover = scenes.config2(64, 36, 1, 1, 8).spheres
        same = cover[:200].copy(); same["center"][:] = (1.0, 2.0, 3.0)
        huge = cover.copy(); huge["center"] *= np.float32(1e12)
        tiny = cover[:17].copy(); tiny["radius"] = np.float32(1e-30)
        flat = cover.copy(); flat["center"][:, 1] = 0.0; flat["center"][:, 2] = 0.0
        built = 0
        for sph in (cover, same, huge, tiny, flat, cover[:15], cover[:16]):
            ptr, n, keep = abi.spheres_as_ctypes(sph)
            cnt = np.zeros(5, np.uint32); mar = np.zeros(4, np.float32)
            rc = H.pt_build_bvh(ptr, n, None, 0, None, 0, None, 0, mar.ctypes.data, cnt.ctypes.data, None, 0, None, None, 0)
            if rc != 0:
                continue
            nodes = np.zeros(int(cnt[0]) * 8, np.float32); slots = np.zeros(int(cnt[1]) * 4, np.float32)
            idx = np.zeros(int(cnt[1]), np.uint32); n16 = np.zeros((int(cnt[0]) + 1) * 4, np.uint32)
            n32 = np.zeros((int(cnt[0]) + 1) * 8, np.float32); k = C.c_float(0)
            rc = H.pt_build_bvh(ptr, n, nodes.ctypes.data, nodes.size, slots.ctypes.data, slots.size, idx.ctypes.data, idx.size,
                                mar.ctypes.data, cnt.ctypes.data, n16.ctypes.data, n16.size, C.byref(k), n32.ctypes.data, n32.size)
            assert rc == 0 and sorted(idx[idx != 0xFFFFFFFF].tolist()) == list(range(n))
            built += 1
        assert built >= 5
        # host: the grid builder (registration, Morton runs) at every margin class, size query then filled call, plus the
        # walk constants, on the same scenes and the 10 000-sphere field
        G.grid_class_build.restype = C.c_int
        G.grid_class_build.argtypes = [C.POINTER(abi.PtSphere), C.c_uint32, C.c_double, C.c_int, vp, vp, vp, vp, vp, vp,
                                          C.c_size_t, vp, C.c_size_t, vp, C.c_size_t]
        H.pt_grid_walk_constants.argtypes = [C.POINTER(abi.PtSphere), C.c_uint32, vp]
        field = scenes.config5(64, 36, 1, 1, 8).spheres
        per_class = {}
        capacity_seen = 0
        for sph in (cover, same, huge, tiny, flat, cover[:15], cover[:16], field):
            ptr, n, keep = abi.spheres_as_ctypes(sph)
            w10 = np.zeros(10, np.float32)
            rc = H.pt_grid_walk_constants(ptr, n, w10.ctypes.data)
            assert rc in (0, abi.PT_ERR_NOT_READY), rc
            for f in (2.5, 3.0, 4.0, 5.5, 8.0, 12.0, 16.0):
                for layout in (0, 1):
                    cnt = np.zeros(8, np.uint32); geo = np.zeros(12, np.float32); mar = np.zeros(4, np.float32)
                    dg = np.zeros(1, np.float32)
                    rc = G.grid_class_build(ptr, n, f, layout, cnt.ctypes.data, geo.ctypes.data, mar.ctypes.data, dg.ctypes.data,
                                               w10.ctypes.data, None, 0, None, 0, None, 0)
                    if rc != 0:
                        assert rc == abi.PT_ERR_NOT_READY, rc
                        continue
                    cells = np.zeros(int(cnt[0]) * int(cnt[1]) * int(cnt[2]), np.uint32)
                    ent = np.zeros(int(cnt[5]) * 4, np.float32); idx = np.zeros(int(cnt[5]), np.uint32)
                    if capacity_seen < 3:  # undersized arrays: refused, nothing written past them
                        short = [(cells.size - 1, ent.size, idx.size), (cells.size, ent.size - 4, idx.size), (cells.size, ent.size, idx.size - 1)][capacity_seen]
                        rc = G.grid_class_build(ptr, n, f, layout, None, None, None, None, None, cells.ctypes.data, short[0],
                                                   ent.ctypes.data, short[1], idx.ctypes.data, short[2])
                        assert rc == abi.PT_ERR_CAPACITY, rc
                        capacity_seen += 1
                    rc = G.grid_class_build(ptr, n, f, layout, cnt.ctypes.data, geo.ctypes.data, mar.ctypes.data, dg.ctypes.data,
                                               w10.ctypes.data, cells.ctypes.data, cells.size, ent.ctypes.data, ent.size,
                                               idx.ctypes.data, idx.size)
                    assert rc == 0 and int((cells >> 24).sum()) == int(cnt[3]), rc
                    per_class[f] = per_class.get(f, 0) + 1
        assert len(per_class) == 7 and capacity_seen == 3, (per_class, capacity_seen)
        print("SANITIZED-OK", int(seg))
    ''') % (ROOT, ora_so, host_so, grid_so)
    env = dict(os.environ, LD_PRELOAD=asan + ":" + ubsan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "SANITIZED-OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
