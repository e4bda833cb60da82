// probe_main.cpp — a stand-alone program over csrc/pt_probe.hpp for -fsanitize=address,undefined: the sweep of
// tests/probe_sweep.hpp — every pixel against every record set, the half-space test on and off, a bias of 0 and of 0.05 —
// through the functions the kernels compile, with the records in an exactly sized heap array: a corner node past the lattice, a
// float-to-int conversion out of range or an index past the 28 floats of a record is a report, not a wrong bit.  The node
// positions and the buried rule over exactly sized arrays likewise.  tests/test_probe_ref.py builds it and runs it as a child;
// nothing sanitized is loaded into Python.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../ray_tracer_webgl_amd/csrc/pt_probe.hpp"
#include "probe_sweep.hpp"

int main() {
  const PtProbeLattice L = probesweep::lattice();
  if (ptprobe::lattice_error(L)) { std::printf("probe: the sweep's lattice is refused\n"); return 1; }
  {
    PtProbeLattice bad = L;
    bad.nx = 1;
    if (!ptprobe::lattice_error(bad)) { std::printf("probe: nx = 1\n"); return 1; }
    bad = L; bad.nx = bad.ny = bad.nz = 256;
    if (!ptprobe::lattice_error(bad)) { std::printf("probe: 2^24 nodes\n"); return 1; }
    bad = L; bad.step[1] = NAN;
    if (!ptprobe::lattice_error(bad)) { std::printf("probe: a NaN step\n"); return 1; }
    if (!ptprobe::slice_valid(L, 30u, 6u) || ptprobe::slice_valid(L, 30u, 7u) || ptprobe::slice_valid(L, 0xffffffffu, 2u)) { std::printf("probe: slice_valid\n"); return 1; }
  }
  const uint32_t nodes = ptprobe::node_count(L);
  if (nodes != 36u) { std::printf("probe: node_count\n"); return 1; }
  // the nodes into an exactly sized array, and the buried rule
  std::unique_ptr<float[]> pos(new float[3 * (size_t)nodes]);
  for (uint32_t i = 0; i < nodes; i++) ptprobe::node_position(L, i, pos.get() + 3 * (size_t)i);
  if (pos[0] != L.origin[0] || pos[3 * (size_t)(nodes - 1u) + 2] != 1.0f) { std::printf("probe: node positions\n"); return 1; }
  {
    const float* p = pos.get() + 3 * 13;  // node (1, 1, 1)
    const float at[4] = {p[0], p[1], p[2], 0.25f}, nan_centre[4] = {NAN, p[1], p[2], 100.0f}, zero[4] = {p[0], p[1], p[2], 0.0f};
    if (!ptprobe::buried_by(p, at, PT_DIFFUSE) || !ptprobe::buried_by(p, at, PT_EMISSIVE) || !ptprobe::buried_by(p, at, 7) || ptprobe::buried_by(p, at, PT_GLASS) ||
        ptprobe::buried_by(p, nan_centre, PT_METAL) || ptprobe::buried_by(p, zero, PT_DIFFUSE)) { std::printf("probe: buried_by\n"); return 1; }
  }
  const std::vector<probesweep::Pixel> pixels = probesweep::pixels();
  size_t unusable = 0, lit = 0, flat = 0;
  for (int set = 0; set < probesweep::SET_COUNT; set++) {
    const std::vector<float> r = probesweep::records(set);
    if (r.size() != (size_t)nodes * ptprobe::kRecordFloats) { std::printf("probe: a set's size\n"); return 1; }
    std::unique_ptr<float[]> exact(new float[r.size()]);
    std::memcpy(exact.get(), r.data(), r.size() * sizeof(float));
    const float* records = exact.get();
    auto load = [records, nodes](uint32_t node, int, float rec[ptprobe::kRecordFloats]) {
      if (node >= nodes) { std::printf("probe: node %u of %u\n", node, nodes); std::abort(); }
      std::memcpy(rec, records + (size_t)node * ptprobe::kRecordFloats, sizeof(float) * ptprobe::kRecordFloats);
    };
    for (uint32_t flags = 0; flags < 2; flags++)
      for (float bias : {0.0f, 0.05f})
        for (const probesweep::Pixel& px : pixels) {
          std::unique_ptr<float[]> out(new float[4]);
          ptprobe::shade_pixel(px.albedo, px.n, px.hp, px.index, px.type, L, flags, bias, probesweep::camera(), load, out.get());
          if (!(out[3] == 0.0f || out[3] == 1.0f)) { std::printf("probe: alpha %g\n", (double)out[3]); return 1; }
          const bool is_flat = px.index < 0 || (px.type != PT_DIFFUSE && px.type != PT_METAL && px.type != PT_GLASS);
          if (is_flat && out[3] != 1.0f) { std::printf("probe: a flat pixel without alpha\n"); return 1; }
          for (int c = 0; c < 3; c++)
            if (!(out[c] >= 0.0f)) { std::printf("probe: channel %d = %g\n", c, (double)out[c]); return 1; }
          if (out[3] == 0.0f && (out[0] != 0.0f || out[1] != 0.0f || out[2] != 0.0f)) { std::printf("probe: colour without alpha\n"); return 1; }
          if (set == probesweep::SET_ALL_EMPTY && !is_flat && out[3] != 0.0f) { std::printf("probe: a texel from empty records\n"); return 1; }
          if (set == probesweep::SET_NEGATIVE && !is_flat && px.type == PT_DIFFUSE && out[3] == 1.0f && (out[0] != 0.0f || out[1] != 0.0f || out[2] != 0.0f)) {
            std::printf("probe: a negative blend does not clamp\n");
            return 1;
          }
          flat += is_flat;
          lit += !is_flat && out[3] == 1.0f;
          unusable += !is_flat && out[3] == 0.0f;
        }
  }
  if (!flat || !lit || !unusable) { std::printf("probe: the sweep misses a class of pixels (%zu flat, %zu lit, %zu unusable)\n", flat, lit, unusable); return 1; }
  std::printf("probe: ok (%zu flat, %zu lit, %zu unusable)\n", flat, lit, unusable);
  return 0;
}
