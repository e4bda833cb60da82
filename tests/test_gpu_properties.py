"""BASELINE.json's configurations at their FULL sizes on the GPU (through the C ABI).

The oracle cannot render these frames whole in test time, so each config is checked by
  (a) an oracle spot-check: a small pixel window rendered by the oracle at the config's full
      resolution, full sample count and full depth, compared bit for bit, and
  (b) size-independent properties: row-band partition invariance, pass additivity (one batched
      launch == several launches), run-to-run determinism under a different work-queue order
      (the tile order is fed back from the previous launch, so the second run schedules
      differently), sample-count bookkeeping, finiteness, and — for config 2 — the committed
      checksum of the full frame.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer, render_scene

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def spot_check(ora, sc, got, window):
    x0, x1, y0, y1 = window
    ref, _ = ora.render(sc.spheres, sc.params, sc.n_passes, window=window)
    g, r = bits(got[y0:y1, x0:x1]), bits(ref[y0:y1, x0:x1])
    assert np.array_equal(g, r), "%s: %d of %d window values differ" % (sc.name, (g != r).sum(), g.size)


def test_config2_full(ora):
    """Cover scene, 1920x1080, 1024 spp (16 x 64), 50 bounces, one GPU."""
    sc = scenes.config2()
    t, a = render_scene(sc)
    st = t.stats()
    assert st.total_spp == 1024 and np.all(a[..., 3] == 1024.0)
    assert np.isfinite(a).all() and (a[..., :3] >= 0).all()
    spot_check(ora, sc, a, (1000, 1012, 400, 408))   # glass / metal spheres near the centre
    spot_check(ora, sc, a, (40, 48, 1060, 1068))     # sky corner
    # pass additivity + a different queue order: 8 + 8 passes in two launches on the same context
    t.reset()
    q = sc.params.copy()
    t.set_params(q)
    t.render_passes(8)
    q.time = 8.0
    t.set_params(q)
    t.render_passes(8)
    b = t.accum()
    assert np.array_equal(bits(a), bits(b))
    assert t.stats().segments == st.segments
    # row bands: 3 ranks' worth, interleaved 8-row bands
    out = np.zeros_like(a)
    seg = 0
    for r in range(3):
        tb, part = render_scene(sc, band=(8, r, 3))
        out[abi.owned_rows(1080, 8, r, 3)] = part
        seg += tb.stats().segments
        tb.close()
    assert np.array_equal(bits(out), bits(a)) and seg == st.segments
    # the committed checksum of the whole frame (tests/golden/full_frame_digests.json)
    with open(os.path.join(GOLDEN, "full_frame_digests.json")) as f:
        want = json.load(f)["config2_1920x1080_1024spp"]
    assert digest(a) == want["sha256"] and st.segments == want["segments"]
    t.close()


def test_config2_as_the_bench_renders_it(ora):
    """The same frame in the pass shape bench.py uses: 64 passes of 16 spp with pass times that do
    not line up with the seed step (PtParams.time_step).  Oracle windows at the full 1024 spp,
    batching invariance (16 + 48 passes through first_pass), the committed checksum."""
    sc = scenes.config2(1920, 1080, 16, 64, 50)
    sc.params.time_step = abi.PT_TIME_STEP_DECORRELATED
    t, a = render_scene(sc)
    st = t.stats()
    assert st.total_spp == 1024 and np.all(a[..., 3] == 1024.0) and np.isfinite(a).all()
    spot_check(ora, sc, a, (1000, 1012, 400, 408))
    spot_check(ora, sc, a, (700, 708, 200, 206))
    t2, b = render_scene(sc, passes_per_launch=48)  # 48 + 16
    assert np.array_equal(bits(a), bits(b)) and t2.stats().segments == st.segments
    with open(os.path.join(GOLDEN, "full_frame_digests.json")) as f:
        want = json.load(f).get("config2_1920x1080_64x16spp_decorrelated")
    assert want is not None and digest(a) == want["sha256"] and st.segments == want["segments"]
    t.close()
    t2.close()


def test_config3_4k(ora):
    """BASELINE config 3 as stated: the cover scene at 3840x2160, 4096 spp (64 passes of 64),
    50 bounces — the whole frame on one GPU, an oracle window at the full 4096 spp, and the row
    partition of the 8-GPU run: all eight ranks' interleaved bands, rendered one after the other
    on this GPU, reassemble the full frame bit for bit (each rank's share is the dist.py layout
    the RCCL all_gather moves)."""
    sc = scenes.config3()
    assert sc.n_passes == 64 and sc.params.samples_per_pixel == 64
    t, a = render_scene(sc)
    st = t.stats()
    assert st.total_spp == 4096 and np.all(a[..., 3] == 4096.0) and np.isfinite(a).all()
    spot_check(ora, sc, a, (2000, 2008, 800, 806))
    spot_check(ora, sc, a, (3836, 3840, 2154, 2160))  # sky corner, last tile column / row
    t.close()
    out = np.zeros_like(a)
    seg = 0
    shares = []
    for r in range(8):
        tb, part = render_scene(sc, band=(8, r, 8))
        ys = abi.owned_rows(2160, 8, r, 8)
        assert part.shape[0] == len(ys)
        out[ys] = part
        shares.append(tb.stats().segments)
        seg += shares[-1]
        tb.close()
    assert np.array_equal(bits(out), bits(a)) and seg == st.segments
    assert max(shares) < 1.04 * seg / 8  # interleaved bands: no rank carries more than 4 % extra


def test_config4_room_8192spp(ora):
    """Enclosed room + emissive sphere, 1024x1024, 8192 spp (128 x 64), depth 50."""
    sc = scenes.config4()
    t, a = render_scene(sc, passes_per_launch=32)
    assert t.stats().total_spp == 8192 and np.all(a[..., 3] == 8192.0)
    assert np.isfinite(a).all() and a[..., :3].max() > 0
    spot_check(ora, sc, a, (508, 514, 300, 304))
    spot_check(ora, sc, a, (10, 14, 10, 13))
    t.close()


def test_config5_field_256spp(ora):
    """10 001 spheres (the whole LDS list), 1920x1080, 256 spp (4 x 64), depth 50."""
    sc = scenes.config5()
    t, a = render_scene(sc)
    assert t.stats().total_spp == 256 and np.all(a[..., 3] == 256.0)
    assert np.isfinite(a).all()
    spot_check(ora, sc, a, (960, 964, 300, 303))
    t2, b = render_scene(sc, passes_per_launch=2)  # 2 + 2
    assert np.array_equal(bits(a), bits(b)) and t2.stats().segments == t.stats().segments
    t.close()
    t2.close()


def test_default_scene_reference_resolution(ora):
    """The reference's own operating point: State::default scene, 1280x702 (images/14.png's
    size), 25 spp per frame while paused (src/webgl.rs:342-346), depth 8 — 16 frames."""
    sc = scenes.default_scene(1280, 702, 25, 8, n_passes=16)
    t, a = render_scene(sc)
    assert np.all(a[..., 3] == 400.0)
    spot_check(ora, sc, a, (600, 616, 340, 350))
    spot_check(ora, sc, a, (300, 310, 250, 258))  # the negative-radius metal spheres
    t.close()


def test_config2_full_resolution_whole_frame_vs_oracle(ora):
    """Every one of the 1920x1080 pixels of the cover scene against the oracle (2 passes x 8 spp,
    depth 50: the oracle needs a few seconds on the box's cores)."""
    sc = scenes.config2(1920, 1080, 8, 2, 50)
    t, a = render_scene(sc)
    ref, seg = ora.render(sc.spheres, sc.params, 2)
    g, r = bits(a), bits(ref)
    assert np.array_equal(g, r), "%d of %d values differ" % ((g != r).sum(), g.size)
    assert t.stats().segments == seg
    t.close()


def _whole_frame_vs_oracle(ora, t, sc, what):
    """One launch of sc.n_passes passes on the context `t` AS IT STANDS (its grid, its settled path) against the oracle,
    every pixel and the segment count."""
    t.reset()
    t.set_params(sc.params)
    t.render_passes(sc.n_passes)
    a = t.accum()
    ref, seg = ora.render(sc.spheres, sc.params, sc.n_passes)
    g, r = bits(a), bits(ref)
    assert np.array_equal(g, r), "%s: %d of %d values differ from the oracle" % (what, (g != r).sum(), g.size)
    assert t.stats().segments == seg, (what, t.stats().segments, seg)
    return a


def test_config5_as_benchmarked_whole_frame_vs_list_walk_and_oracle(ora):
    """VERDICT r5 #1a.  `bench.py --config 5` times the grid AFTER pt_tune has refitted it to the camera (margin class
    2.5 s0 instead of the 3 s0 pt_set_spheres builds for, each sphere registered with its own margin: fewer entries) —
    not the grid the other full-size tests walk.  Here the as-benchmarked context (same scene call, same pass shape,
    same decorrelated pass times, pt_tune(8) like bench.py) renders the WHOLE 1920x1080 frame: one 16-spp pass against
    the reference's own algorithm on the device (the scalar list walk: every sphere for every ray), bits and segments,
    and one 1-spp pass against the ORACLE (2x10^6 pixels x 10 001 spheres: ~half a minute of the box's cores)."""
    sc = scenes.config5(1920, 1080, 16, 1, 50)
    sc.params.time_step = abi.PT_TIME_STEP_DECORRELATED
    built = PathTracer(1920, 1080)
    built.set_spheres(sc.spheres)
    n_built = built.stats().grid_entries
    built.close()
    t, a = render_scene(sc, tune=8)  # bench.py: pt.tune(min(passes per launch, 8))
    st = t.stats()
    assert st.geometry_path == abi.PT_GEOM_GRID and st.geometry_tuned == 1
    # the grid pt_tune KEPT after timing its candidates (2.5 s0 — what the camera needs — against the 3 s0 pt_set_spheres builds
    # for): on this view the tight class wins, and then it is the refit grid, with fewer entries, that the frame below walks
    print("pt_tune kept %.1f s0: %d entries (as built %d)" % (st.grid_near_factor, st.grid_entries, n_built))
    assert st.grid_near_factor in (2.5, 3.0) and st.grid_fit_stale == 0, (st.grid_near_factor, st.grid_fit_stale)
    assert (st.grid_entries < n_built) == (st.grid_near_factor == 2.5), (st.grid_entries, n_built)
    assert st.far_rays < 1e-4 * st.segments, (st.far_rays, st.segments)
    t2, b = render_scene(sc, geometry_path=abi.PT_GEOM_SCALAR)
    assert t2.stats().geometry_path == abi.PT_GEOM_SCALAR
    g, r = bits(a), bits(b)
    assert np.array_equal(g, r), "refit grid vs list walk: %d of %d values differ" % ((g != r).sum(), g.size)
    assert t2.stats().segments == st.segments
    t2.close()
    one = scenes.config5(1920, 1080, 1, 1, 50)
    one.params.time_step = abi.PT_TIME_STEP_DECORRELATED
    _whole_frame_vs_oracle(ora, t, one, "config 5 on the refit grid, 1 spp")
    assert t.stats().grid_entries == st.grid_entries and t.stats().geometry_path == abi.PT_GEOM_GRID
    t.close()


def test_config3_4k_as_benchmarked_whole_frame_vs_oracle(ora):
    """VERDICT r5 #1b.  The cover scene at 3840x2160 through the context bench.py --config 3 sets up (pt_tune: the grid
    refitted to the camera at (13, 2, 3), PT_GEOM_AUTO settled): every one of the 8.3x10^6 pixels against the oracle,
    one pass of 2 spp at depth 50."""
    sc = scenes.config3(3840, 2160, 2, 1, 50)
    sc.params.time_step = abi.PT_TIME_STEP_DECORRELATED
    t, _ = render_scene(sc, tune=8)
    assert t.stats().geometry_path == abi.PT_GEOM_GRID and t.stats().grid_fit_stale == 0
    _whole_frame_vs_oracle(ora, t, sc, "config 3 at 4K, 2 spp")
    t.close()


def test_config4_as_benchmarked_whole_frame_vs_oracle(ora):
    """VERDICT r5 #1c.  The closed room at 1024x1024 through the small-list kernel PT_GEOM_AUTO settles on after pt_tune
    (nine spheres: no grid to fit): every pixel against the oracle, one pass of 8 spp at depth 50 (mean path ~40 segments)."""
    sc = scenes.config4(1024, 1024, 8, 1, 50)
    sc.params.time_step = abi.PT_TIME_STEP_DECORRELATED
    t, _ = render_scene(sc, tune=8)
    # (whichever list kernel PT_GEOM_AUTO measured fastest on this box — at this size the small-list kernel, bench.py's
    # pt_trace_kernel_small_t1; the other two candidates walk the same nine spheres)
    assert t.stats().geometry_path in (abi.PT_GEOM_SMALL, abi.PT_GEOM_LDS, abi.PT_GEOM_SCALAR) and t.stats().grid_near_factor == 0.0
    _whole_frame_vs_oracle(ora, t, sc, "config 4, 8 spp")
    t.close()


def _bench(*extra, timeout=900, full=True):
    """One bench.py line; --full by default: the tests below read the legs a plain run leaves out."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + (["--full"] if full else []) + list(extra),
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    d["_stdout_lines"] = len([ln for ln in r.stdout.splitlines() if ln.strip()])
    return d


def test_bench_two_ranks_on_one_device():
    """bench.py's N > 1 path on hardware, as far as a one-GPU box allows: two self-started ranks
    (gloo collectives, both on cuda:0) render their row bands of BASELINE config 2 — the DEFAULT
    workload: strong scaling, the fixed 1920x1080x1024-spp frame — through libptrace; rank 0's
    gathered frame must hash to the committed single-GPU digest (the check an RCCL run makes
    too), and the weak-scaling point must be reported beside it."""
    d = _bench("--gpus", "2", "--backend", "gloo", "--same-device", "--warmup", "4",
               "--no-cpu-baseline", "--no-list-walk", "--no-work-count")
    assert d["n_gpus"] == 2 and d["ranks"] == 2 and d["scaling"] == "strong"
    assert d["steps"] == 16 and d["converged_frame_spp"] == 1024 and "config2" in d["config"]["workload"]
    assert len(d["per_rank_render_kernel_ms"]) == 2 and min(d["per_rank_render_kernel_ms"]) > 0
    assert d["config"]["passes_per_launch"] == 16 * 4  # steps per launch x passes per step, whatever N
    gc = d["gather_check"]
    assert gc and gc["key"] == "config2_1920x1080_64x16spp_decorrelated"
    assert d["gather_matches_single_gpu"] is True and gc["segments_match"] is True, gc
    ws = d["weak_series"]
    assert ws and ws["scaling"] == "weak" and ws["spp"] == 2 * 1024 and ws["sec"] > 0
    assert abs(d["sec_to_converged_frame"] - d["ms_per_step"] * 16 / 1e3) < 1e-3
    assert d["value"] > 0 and d["segments"] > 0 and d["first_frame_ms"] > 0


def test_bench_under_the_drivers_flags_still_carries_its_verdicts():
    """The driver runs `bench.py --steps 20 --warmup 5` (1280 spp: not the committed 1024-spp frame), at N = 1
    and — on an 8-GPU node — under torchrun with the same flags.  The line must verify itself anyway: every
    rank renders the committed workload once more after the timed region, through the same partition and the
    same gather, and rank 0 hashes that (`gather_matches_single_gpu` true, never null); the measuring twin is
    compared with a launch of the timed kernel over the same passes.  Two self-started ranks on one device
    (gloo collectives), then one rank."""
    d = _bench("--gpus", "2", "--backend", "gloo", "--same-device", "--steps", "20", "--warmup", "5",
               "--no-cpu-baseline", "--no-list-walk", "--no-work-count", "--no-first-frame", "--no-weak-series")
    assert d["n_gpus"] == 2 and d["ranks"] == 2 and d["steps"] == 20 and d["warmup"] == 5
    gc = d["gather_check"]
    assert d["gather_matches_single_gpu"] is True and gc["segments_match"] is True, gc
    assert "rendered again after the timed region" in gc["frame"]
    assert abs(d["sec_to_converged_frame"] - d["ms_per_step"] * 16 / 1e3) < 1e-3  # still quoted on the 1024-spp frame
    d = _bench("--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-list-walk", "--no-first-frame")
    assert d["n_gpus"] == 1 and d["gather_matches_single_gpu"] is True, d["gather_check"]
    assert d["roofline"]["executed"]["twin_segments_equal_timed_kernel"] is True
    c = d["roofline"]["counters"]  # the committed PMC record of this kernel: attached when it was collected on THIS build, refused otherwise
    assert c is None or (c["stale"] is True and "valu_issue_frac" not in c) or (c["stale"] is False and c["valu_issue_frac"] > 0)
    assert c is None or c["prior_over_this_run_kernel_ms"] > 0
    assert d["build"]["csrc_sha256"] and (c is None or c["this_build_csrc_sha256"] == d["build"]["csrc_sha256"])


def test_bench_rccl_path_with_one_rank():
    """--force-dist: the RCCL code path (init with device_id, all_gather_into_tensor on device buffers,
    all_reduce of the timings) as far as one GPU allows.  Rank 0's stdout must carry the JSON line and
    NOTHING else — RCCL prints a version banner to stdout when its communicator comes up — and the frame
    that went through the collective must hash to the committed digest."""
    d = _bench("--force-dist", "--no-cpu-baseline", "--no-list-walk", "--no-work-count", "--no-first-frame", "--warmup", "4")
    assert d["_stdout_lines"] == 1
    assert d["ranks"] == 1 and d["gather_matches_single_gpu"] is True and d["scaling"] == "strong"


def test_bench_weak_scaling_and_small_frames():
    """--scaling weak keeps the round-2 semantics (N x the passes per step on 1/N of the rows); a
    workload that is not the committed one reports no digest verdict instead of a wrong one."""
    d = _bench("--gpus", "2", "--backend", "gloo", "--same-device", "--scaling", "weak",
               "--width", "480", "--height", "270", "--steps", "2", "--warmup", "1", "--steps-per-launch", "2",
               "--no-cpu-baseline", "--no-list-walk", "--no-work-count", "--no-first-frame")
    assert d["n_gpus"] == 2 and d["scaling"] == "weak"
    assert d["config"]["passes_per_launch"] == 2 * 4 * 2  # steps per launch x passes per step x ranks
    assert d["gather_matches_single_gpu"] is None and d["weak_series"] is None
    assert d["value"] > 0 and d["segments"] > 0


def test_bench_single_gpu_line_matches_the_committed_digest():
    """N = 1, default flags (minus the slow legs): the frame bench.py times IS the committed frame."""
    d = _bench("--no-cpu-baseline", "--no-list-walk", "--warmup", "4")
    assert d["n_gpus"] == 1 and d["scaling"] == "strong" and d["gather_matches_single_gpu"] is True
    ex = d["roofline"]["executed"]
    assert ex and ex["twin_segments_equal_timed_kernel"] is True
    assert d["roofline"]["frac"] and 0 < d["roofline"]["frac"] <= 1


def test_a_plain_bench_run_times_its_steps_and_dumps_what_they_computed(tmp_path):
    """Without --full the line is the headline alone (no leg beside it) and --steps sets the timed steps; --dump-outputs
    writes what those steps accumulated: (height, width, 4) fp32 with steps x 64 spp in every pixel's 4th channel and the
    line's segment count, the same bits again from a second run with the same flags.  At a reduced size."""
    import numpy as np

    flags = ("--width", "192", "--height", "108", "--steps", "3", "--warmup", "2")
    d = _bench(*flags, "--dump-outputs", str(tmp_path / "a"), full=False)
    assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "Mray/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["_stdout_lines"] == 1
    assert all(d[k] is None for k in ("first_frame", "gather_check", "list_walk", "cpu_baseline", "weak_series"))
    assert d["roofline"]["executed"] is None
    acc = np.load(tmp_path / "a" / "accum.npy")
    assert acc.dtype == np.float32 and acc.shape == (108, 192, 4) and np.all(acc[..., 3] == 3 * 64)
    seg = np.load(tmp_path / "a" / "segments.npy")
    assert seg.dtype == np.float64 and seg.tolist() == [float(d["segments"])]
    _bench(*flags, "--dump-outputs", str(tmp_path / "b"), full=False)
    assert np.array_equal(np.load(tmp_path / "b" / "accum.npy").view(np.uint32), acc.view(np.uint32))
    assert np.array_equal(np.load(tmp_path / "b" / "segments.npy"), seg)


def test_a_plain_frame_loop_bench_run_times_its_steps_and_dumps_the_canvas(tmp_path):
    """`--config default` without --full: the replayed animation loop alone, --steps timed frames, and the canvas of the last
    one (RGBA8 as fp32) from --dump-outputs."""
    import numpy as np

    d = _bench("--config", "default", "--steps", "70", "--warmup", "16", "--dump-outputs", str(tmp_path), full=False)
    assert d["full"] is False and d["steps"] == 70 and d["animation"]["frames"] == 70 and d["ms_per_step"] > 0
    assert d["unit"] == "frames/s" and d["group_trace_kernel"] is None and "roofline" not in d and "cpu_baseline" not in d
    assert d["animation_issued_per_frame_from_the_host"] is None and d["paused_25spp"] is None
    c = np.load(tmp_path / "canvas.npy")
    assert c.dtype == np.float32 and c.shape == (702, 1280, 4)
    assert np.array_equal(c, np.round(c)) and c.min() >= 0 and c.max() <= 255 and np.all(c[..., 3] == 255)


@pytest.mark.parametrize("config,kernels", [("4",("pt_trace_kernel_small_t1", "pt_trace_kernel", "pt_trace_kernel_scalar")),
                                            ("5", ("pt_trace_kernel_grid_cells", "pt_trace_kernel_bvh_nodes"))])
def test_bench_lines_of_the_stress_configs(config, kernels):
    """`bench.py --config 4 / 5`: BASELINE's closed room and 10 000-sphere field through the same line
    (roofline + cpu_baseline), here at a reduced size; the kernel named is one this scene can get
    (PT_GEOM_AUTO measures on a small frame here, so which of them wins is not asserted)."""
    d = _bench("--config", config, "--width", "192", "--height", "108", "--steps", "2", "--warmup", "1", "--cpu-strip", "8")
    assert ("config" + config) in d["config"]["workload"] and d["n_gpus"] == 1 and d["value"] > 0
    r = d["roofline"]
    assert r["kernel"] in kernels, r["kernel"]
    assert d["cpu_baseline"]["value"] > 0 and d["gather_matches_single_gpu"] is None
    if config == "5":
        assert d["list_walk"]["roofline_frac"] > 0
    if r["kernel"] != "pt_trace_kernel_bvh_nodes":  # (that build has no measuring twin)
        assert r["frac"] and 0 < r["frac"] <= 1
    if config == "4":  # list kernels: the algorithmic tests AND the per-segment shade / RNG / camera term
        pp = r["per_pass"]
        assert pp["executed_flop"] > pp["algorithmic_flop"] and abs(pp["executed_flop"] - pp["algorithmic_flop"] - 150 * pp["segments"]) < 1e-3 * pp["executed_flop"]


@pytest.mark.parametrize("config", ["4", "5"])
def test_bench_stress_config_frames_match_the_committed_digests(config):
    """The full frames `bench.py --config 4 / 5` time (8192 spp of the closed room, 256 spp of the
    10 001-sphere field) hash to tests/golden/full_frame_digests.json — drift guards of the HIP path
    across rounds (their pixels are pinned by the oracle windows of test_config4_room_8192spp
    and test_config5_field_256spp), and the frame an N > 1 run of these configs would have to gather."""
    d = _bench("--config", config, "--no-cpu-baseline", "--no-list-walk", "--no-work-count", "--no-first-frame", "--warmup", "1")
    assert d["gather_matches_single_gpu"] is True, d["gather_check"]
    assert d["gather_check"]["segments_match"] is True
    assert d["converged_frame_spp"] == {"4": 8192, "5": 256}[config]


def test_the_dev_tools_watchdog_polls_instead_of_blocking():
    """pt_debug_wait (include/ptrace_dev.h): records an event behind what is enqueued and polls it with a
    deadline.  An idle stream answers at once; a launch in flight is waited for (well inside the deadline);
    a zero deadline on a long launch reports "timeout" without blocking — and the launch still finishes."""
    import time

    sc = scenes.config2(1920, 1080, 16, 16, 50)
    t = PathTracer(1920, 1080)
    t.set_geometry_path(abi.PT_GEOM_GRID)
    t.set_spheres(sc.spheres)
    t.set_params(sc.params)
    t.reserve_passes(16)
    assert t.wait(1.0) is True            # nothing enqueued
    t.render_passes(16)                   # ~28 ms of kernel time
    t0 = time.perf_counter()
    timed_out = not t.wait(0.0)
    assert time.perf_counter() - t0 < 0.02   # did not block on the launch
    assert t.wait(30.0) is True
    st = t.stats()
    assert st.segments > 0 and (timed_out or st.render_kernel_ms > 0)
    t.close()


def test_bench_line_of_the_references_own_operating_point():
    """`bench.py --config default` (State::default, 1280x702, 1 spp per tick, the shader's
    temporal blend: src/state.rs:127-135, src/webgl.rs:180-205) is under the measurement contract like the main
    line: `roofline` prices the trace launch of one group of 64 frames (a list kernel: executed = algorithmic),
    timed with HIP events around that kernel alone, and `cpu_baseline` is the oracle replaying the same ticks."""
    d = _bench("--config", "default", "--frames", "96", "--warmup", "16")
    assert d["unit"] == "frames/s" and d["value"] > 1000 and d["config"]["workload"].startswith("default: State::default")
    r = d["roofline"]
    assert r["kernel"] == "pt_trace_kernel_small_t1" and r["passes_per_launch"] == 64 and r["spp_per_pass"] == 1
    assert r["avg_launch_ms"] > 0 and r["launches"] >= 8 and 0 < r["frac"] <= 1 and r["bound"] == "valu"
    # the group's trace launch is most of a group's device time (trace + blend + advance)
    assert r["avg_launch_ms"] <= 64 * d["animation"]["device_ms_per_frame"] * 1.05
    assert abs(r["segments_per_launch"] / 64 / d["animation"]["segments_per_frame"] - 1) < 0.01
    c = d["cpu_baseline"]
    assert c["unit"] == "frames/s" and c["value"] > 0 and c["cores"] >= 1 and c["kind"] == "port" and "frames" in c["sample"]
    assert d["gpu_over_cpu"] > 10
    assert d["paused_25spp"]["spp_per_frame"] == 25 and d["animation_issued_per_frame_from_the_host"]["frames_per_s"] > 0
