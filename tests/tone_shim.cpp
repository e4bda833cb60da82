// tone_shim.cpp — csrc/pt_tone.hpp behind a C interface, compiled by tests/test_tone_ref.py with g++ -ffp-contract=off (the
// library's own arithmetic contract) so that the header's statements are checked on the CPU against tests/tone_ref.py: the
// tally of a luminance, the bin edges, the luminance of a colour and the tone curves.  TEST INFRASTRUCTURE ONLY.
#include <stddef.h>
#include <stdint.h>

#include "../ray_tracer_webgl_amd/csrc/pt_tone.hpp"

extern "C" {

// x: n colours of three floats; y: n * 3 toned values
void tone_curves(const float* x, size_t n, int32_t curve, int gamma, float exposure, float white, float* y) {
  for (size_t i = 0; i < n; i++) pttone::tone(x + 3 * i, curve, gamma, exposure, white, y + 3 * i);
}

// x: n colours; bytes: n packed RGBA8 words of the toned colours
void tone_bytes(const float* x, size_t n, int32_t curve, int gamma, float exposure, float white, uint32_t* bytes) {
  for (size_t i = 0; i < n; i++) {
    float y[3];
    pttone::tone(x + 3 * i, curve, gamma, exposure, white, y);
    bytes[i] = pttone::pack_rgba8(y);
  }
}

void tone_luminance(const float* x, size_t n, float* Y) {
  for (size_t i = 0; i < n; i++) Y[i] = pttone::luminance(x + 3 * i);
}

void tone_tally_of(const float* Y, size_t n, uint32_t* slot) {
  for (size_t i = 0; i < n; i++) slot[i] = pttone::tally_of(Y[i]);
}

float tone_bin_edge(uint32_t k) { return pttone::bin_edge(k); }

// texels: rows * width of four floats; tallies: 258 counts (256 bins, below, metered), added to
void tone_meter(const float* texels, uint32_t rows, uint32_t width, int from_accum, const uint32_t window7[7], uint32_t* tallies) {
  const pttone::Window win = {window7[0], window7[1], window7[2], window7[3], window7[4], window7[5], window7[6]};
  for (uint32_t ly = 0; ly < rows; ly++)
    for (uint32_t px = 0; px < width; px++) {
      if (!pttone::in_window(win, px, ly)) continue;
      const float* t = texels + 4 * ((size_t)ly * width + px);
      const pttone::F4 v = {t[0], t[1], t[2], t[3]};
      float x[3];
      pttone::source_colour(v, from_accum != 0, x);
      tallies[pttone::tally_of(pttone::luminance(x))]++;
      tallies[pttone::kMetered]++;
    }
}

}  // extern "C"
