"""The debug overlay (pt_set_debug_overlay; static/shader.frag:307-318) without a GPU.

  (1) tests/overlay_ref.c — the restatement the GPU tests compare against — with the overlay DISABLED is ora_render_pass bit
      for bit: the default scene, a crop of the cover scene, a crop of the closed room, a row band.  That validates the
      restatement; with the overlay enabled it differs from the oracle exactly where it says it coloured a pixel.
  (2) The state layer: pt_state_debug_overlay is the narrowed cursor and the selection of PtStateView, `enable` follows
      pt_state_set_debugging; the new symbols exist and the ABI is still version 5.
  (3) The inputs of tests/test_gpu_overlay.py cannot pass vacuously: per case at least 20 pixels with a blue and 20 with a red
      contribution and an overlay-ended path after a bounce; in some case a hit on the selected sphere that is not outlined.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import overlay_ref as R
from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.state import State

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ (1) the restatement
def _disabled_cases():
    d = scenes.default_scene(160, 88, spp=3, max_depth=8, n_passes=2)
    cover = scenes.config2(192, 108, 2, 2, 12)
    room = scenes.config4(96, 96, 2, 2, 50)
    banded = scenes.default_scene(96, 54, spp=2, max_depth=8, n_passes=2)
    banded.params.band_rows, banded.params.band_index, banded.params.band_count = 4, 1, 3
    lens = scenes.default_scene(64, 36, spp=2, max_depth=8, n_passes=2)
    lens.params.lens_radius = 0.03
    return [("default", d, None), ("cover crop", cover, (70, 130, 30, 70)), ("room crop", room, (20, 70, 10, 60)),
            ("default, band 1 of 3", banded, None), ("default, lens on", lens, None)]


@pytest.mark.parametrize("case", _disabled_cases(), ids=lambda c: c[0])
def test_disabled_restatement_is_the_oracle_bit_for_bit(ora, case):
    name, sc, window = case
    p = sc.params.copy()
    p.time_step = abi.PT_TIME_STEP_DECORRELATED
    ref, seg = ora.render(sc.spheres, p, sc.n_passes, window=window)
    got, tally, flags = R.render(sc.spheres, p, sc.n_passes, None, window=window)
    assert seg > 0 and tally["segments"] == seg, (name, tally["segments"], seg)
    assert np.array_equal(bits(got), bits(ref)), "%s: %d values differ" % (name, int((bits(got) != bits(ref)).sum()))
    assert not flags.any() and tally["blue_paths"] == tally["red_paths"] == 0


def test_enabled_restatement_differs_from_the_oracle_where_it_coloured(ora):
    c = R.default_case()
    ref, seg = ora.render(c.spheres, c.params, c.n_passes)
    got, tally, flags = R.render(c.spheres, c.params, c.n_passes, c.overlay)
    differs = (bits(got) != bits(ref)).any(axis=-1)
    assert differs.any() and tally["segments"] < seg  # (paths end early)
    assert not (differs & (flags == 0)).any()  # a pixel no overlay-ended path touched has the oracle's bits
    # the sample's value is not multiplied by the throughput: a pixel whose EVERY path ended on the dot at depth 0 is exactly
    # (0, 0, samples)
    n = c.n_passes * c.params.samples_per_pixel
    pure = (got[..., 0] == 0.0) & (got[..., 1] == 0.0) & (got[..., 2] == float(n))
    assert pure.sum() >= 20


# ------------------------------------------------------------------------------------------------ (2) the state layer
def test_state_overlay_uniforms_are_the_narrowed_view(lib):
    st = State(320, 176)
    try:
        en, sel, cur = st.debug_overlay()
        assert (en, sel, cur) == (False, abi.NO_SELECTED_OBJECT_ID, (0.0, 0.0, 0.0))  # State::default, src/state.rs:259-261
        st.set_debugging(True)
        assert st.debug_overlay()[0] is True and st.view().render_count == 0
        st.set_camera_origin((0.13, 0.07, 1.0))
        st.set_keys(abi.KEY_W)
        st.update_position(16.5)  # -> update_cursor_position_in_world
        v = st.view()
        en, sel, cur = st.debug_overlay()
        assert en and sel == v.selected_object == 1
        want = tuple(float(np.float32(x)) for x in v.cursor_point)  # Vec3::to_array
        assert cur == want and any(float(x) != w for x, w in zip(v.cursor_point, want))  # (the narrowing is not the identity here)
        st.set_camera_angles(-90.0, 80.0)  # looking at the sky: nothing selected
        st.update_position(0.0)
        assert st.debug_overlay()[1:] == (abi.NO_SELECTED_OBJECT_ID, (0.0, 0.0, 0.0))
        st.set_debugging(False)
        assert st.debug_overlay()[0] is False
        # NULL out pointers are allowed, a NULL state is not
        assert lib.pt_state_debug_overlay(st._h, None, None, None) == abi.PT_OK
        assert lib.pt_state_debug_overlay(None, None, None, None) == abi.PT_ERR_INVALID
        assert lib.pt_state_set_debugging(None, 1) == abi.PT_ERR_INVALID
    finally:
        st.close()


def test_new_symbols_exist_and_the_abi_version_stays(lib):
    for name in ("pt_set_debug_overlay", "pt_last_trace_build", "pt_state_set_debugging", "pt_state_debug_overlay"):
        assert hasattr(lib, name), name
    assert lib.pt_abi_version() == 5 == abi.PT_ABI_VERSION
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptrace.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "ptrace_sys.rs")).read()
    for name in ("pt_set_debug_overlay", "pt_last_trace_build"):
        r = re.search(r"pub fn %s\(([^)]*)\)" % name, rust)
        h = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert r and h, name
        assert len([a for a in r.group(1).split(",") if a.strip()]) == len([a for a in h.group(1).split(",") if a.strip()])
    # a context-free call fails cleanly (no device is needed to see that)
    assert lib.pt_set_debug_overlay(None, 1, 0, (C.c_float * 3)()) == abi.PT_ERR_INVALID


def test_frame_loop_state_wrappers_pick_the_crosshair():
    assert R.state_overlay(320, 176) == (1, (0.0, 0.0, -0.5))  # the centre sphere's nearest point


# ------------------------------------------------------------------------------------------------ (3) coverage of the GPU cases
def test_every_gpu_case_shows_the_dot_the_outline_and_a_deep_ending():
    plain = 0
    for name, make in R.CASES.items():
        c = make()
        assert len(set(int(u) for u in c.spheres["uuid"])) == len(c.spheres), name  # uuid -> sphere is a look-up
        got, tally, flags = R.render(c.spheres, c.params, c.n_passes, c.overlay)
        blue, red = int((flags & 1).astype(bool).sum()), int((flags & 2).astype(bool).sum())
        print("%s: %d pixels with blue, %d with red, %s" % (name, blue, red, tally))
        assert blue >= 20, (name, blue)
        assert red >= 20, (name, red)
        assert tally["deep_overlay_paths"] >= 1, name
        plain += tally["selected_plain_hits"]
    assert plain > 0
    # uuids that are not list indices, in one case
    f = R.field_case()
    assert not np.array_equal(f.spheres["uuid"], np.arange(len(f.spheres)))
