// tone_main.cpp — a stand-alone program over csrc/pt_tone.hpp, built by tests/test_tone_ref.py with
// -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off and run as a child process: the metering loop with its
// window clipping, the solve and the curves over EXACTLY sized heap vectors, so that an index one past an array, a shift or a
// conversion out of range ends the program.  Prints "tone: ok".  TEST INFRASTRUCTURE ONLY.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../ray_tracer_webgl_amd/csrc/pt_tone.hpp"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("tone_main.cpp:%d: %s\n", __LINE__, #cond);         \
      failures++;                                                     \
    }                                                                 \
  } while (0)

static const float kInf = std::numeric_limits<float>::infinity();
static const float kNan = std::numeric_limits<float>::quiet_NaN();

// the values every loop below is fed: the specials, every bin edge with both neighbours
static std::vector<float> operands() {
  std::vector<float> v = {0.0f, -0.0f, 1e-45f, 1e-40f, 0x1p-100f, 0x1p-17f, 1e-10f, 0.18f, 0.5f, 1.0f, 4.0f, 7.99f, 1e10f, 3e38f, kInf, -kInf, kNan, -1e-30f, -1.0f};
  for (uint32_t k = 0; k <= 256; k++) {
    const float e = pttone::bin_edge(k);
    v.push_back(std::nextafterf(e, 0.0f));
    v.push_back(e);
    v.push_back(std::nextafterf(e, kInf));
  }
  return v;
}

// one metering over an exactly sized image and exactly sized tallies: returns the pixels looked at
static uint32_t meter(const std::vector<pttone::F4>& img, uint32_t rows, uint32_t width, bool from_accum, const pttone::Window& win,
                      std::vector<uint32_t>& tallies) {
  tallies.assign(pttone::kTallies, 0u);
  for (uint32_t ly = 0; ly < rows; ly++)
    for (uint32_t px = 0; px < width; px++) {
      if (!pttone::in_window(win, px, ly)) continue;
      float x[3];
      pttone::source_colour(img.at((size_t)ly * width + px), from_accum, x);
      tallies.at(pttone::tally_of(pttone::luminance(x)))++;
      tallies.at(pttone::kMetered)++;
    }
  return tallies.at(pttone::kMetered);
}

int main() {
  const std::vector<float> ops = operands();

  // ---- the tally of every operand, and the bin edges
  for (float Y : ops) {
    const uint32_t s = pttone::tally_of(Y);
    CHECK(s <= pttone::kBelow);
    CHECK((s == pttone::kBelow) == !(Y >= 0x1p-16f));
  }
  for (uint32_t k = 0; k <= 256; k++) {
    const float e = pttone::bin_edge(k);
    CHECK(pttone::tally_of(e) == (k < 256 ? k : 255u));
    CHECK(pttone::tally_of(std::nextafterf(e, kInf)) == (k < 256 ? k : 255u));
    CHECK(pttone::tally_of(std::nextafterf(e, 0.0f)) == (k == 0 ? pttone::kBelow : k - 1));
  }
  CHECK(pttone::bin_edge(0) == 0x1p-16f && pttone::bin_edge(256) == 0x1p16f && pttone::bin_edge(8) == 0x1p-15f);

  // ---- metering: a 7 x 5 image (7 rows of 5) of the operands as accumulation texels and as external texels; windows inside, across
  // and beyond the frame; a band
  const uint32_t rows = 7, width = 5;
  std::vector<pttone::F4> img(rows * width);
  for (size_t i = 0; i < img.size(); i++)
    img[i] = {ops[(3 * i) % ops.size()], ops[(3 * i + 1) % ops.size()], ops[(3 * i + 2) % ops.size()], ops[(7 * i) % ops.size()]};
  std::vector<uint32_t> tallies;
  const uint32_t big = 0xffffffffu;
  struct Case { pttone::Window win; uint32_t expect; };
  const Case cases[] = {
      {{0, 0, 0, 0, 0, 0, 1}, 35},       {{0, 0, 5, 7, 0, 0, 1}, 35},     {{2, 3, 1, 1, 0, 0, 1}, 1},   {{3, 5, big, big, 0, 0, 1}, 4},
      {{5, 0, 3, 3, 0, 0, 1}, 0},        {{0, 7, 3, 3, 0, 0, 1}, 0},      {{big, big, big, big, 0, 0, 1}, 0}, {{4, 6, 9, 9, 0, 0, 1}, 1},
      {{0, 0, 5, 0, 0, 0, 1}, 35},       {{1, 0, big - 1, 2, 0, 0, 1}, 8},
      // band (2, 1, 3): local rows 0..6 are image rows 2, 3, 8, 9, 14, 15, 20
      {{0, 0, 0, 0, 2, 1, 3}, 35},       {{0, 3, 5, 6, 2, 1, 3}, 10},     {{0, 10, 5, big, 2, 1, 3}, 15}, {{0, 0, 5, 2, 2, 1, 3}, 0},
      {{0, 20, 1, 1, 2, 1, 3}, 1},       {{0, big, 5, 5, 2, 1, 3}, 0},
  };
  for (const Case& c : cases)
    for (int from_accum = 0; from_accum < 2; from_accum++) {
      const uint32_t n = meter(img, rows, width, from_accum != 0, c.win, tallies);
      CHECK(n == c.expect);
      uint64_t sum = 0;
      for (uint32_t k = 0; k <= pttone::kBelow; k++) sum += tallies[k];
      CHECK(sum == n);
    }
  CHECK(pttone::band_row(2, 1, 3, 6) == 20u && pttone::band_row(0, 1, 3, 6) == 6u && pttone::band_row(2, 0, 1, 6) == 6u);

  // ---- the solve: exactly 256 bins
  PtMeterOptions opt = PT_METER_OPTIONS_DEFAULT;
  CHECK(pttone::meter_options_valid(opt));
  const PtExposure none{};
  std::vector<uint32_t> hist(pttone::kBins, 0u);
  PtExposure r = pttone::solve(hist, 9u, opt, false, none);
  CHECK(r.exposure == 1.0f && r.white == 1.0f && r.lit == 0 && r.below == 9u && r.meterings == 1u);
  hist[0] = 0xffffffffu;
  hist[255] = 0xffffffffu;  // N beyond 32 bits
  r = pttone::solve(hist, 0u, opt, true, r);
  CHECK(r.lit == 2ull * 0xffffffffull && r.meterings == 2u && r.y_key == pttone::bin_edge(255) && r.y_high == pttone::bin_edge(255));
  CHECK(r.exposure == opt.e_min && r.white == pttone::bin_edge(255) * opt.e_min);
  for (uint32_t p = 0; p <= 1000; p += 125)
    for (uint32_t k : {0u, 1u, 100u, 254u, 255u}) {
      hist.assign(pttone::kBins, 0u);
      hist[k] = 1u;
      hist[(k + 128u) % 256u] = 3u;
      opt.key_permille = p < 990u ? p : 990u;
      opt.high_permille = p < 990u ? 990u : p;
      opt.rate = 0.25f;
      const PtExposure next = pttone::solve(hist, 1u, opt, true, r);
      CHECK(next.lit == 4 && next.meterings == r.meterings + 1u && next.exposure > 0.0f && next.white >= opt.white_min);
      r = next;
    }
  PtMeterOptions bad = PT_METER_OPTIONS_DEFAULT;
  bad.rate = kNan;
  CHECK(!pttone::meter_options_valid(bad));
  bad = PT_METER_OPTIONS_DEFAULT;
  bad.key_permille = 1001u;
  CHECK(!pttone::meter_options_valid(bad));

  // ---- the curves: every operand under every exposure, into exactly sized outputs; the bytes' conversion never sees a value
  // outside (0, 1)
  const float exposures[] = {0x1p-8f, 0.37f, 1.0f, 15.0f, 0x1p8f};
  const float whites[] = {1.0f, 4.0f, kInf, 1e-20f};
  std::vector<float> y(3 * ops.size());
  std::vector<uint32_t> bytes(ops.size());
  for (int32_t curve = PT_TONE_CLAMP; curve <= PT_TONE_FILMIC; curve++)
    for (int gamma = 0; gamma < 2; gamma++)
      for (float e : exposures)
        for (float w : whites)
          for (size_t i = 0; i < ops.size(); i++) {
            const float x[3] = {ops[i], ops[(i + 1) % ops.size()], ops[(i + 2) % ops.size()]};
            pttone::tone(x, curve, gamma, e, w, &y.at(3 * i));
            bytes.at(i) = pttone::pack_rgba8(&y.at(3 * i));
            CHECK((bytes[i] >> 24) == 255u);
            if (curve == PT_TONE_CLAMP && gamma == 0 && e == 1.0f && x[0] == x[0]) CHECK(std::memcmp(&y[3 * i], &x[0], sizeof(float)) == 0);
          }
  if (failures) {
    std::printf("tone: %d checks failed\n", failures);
    return 1;
  }
  std::printf("tone: ok\n");
  return 0;
}
