// ctx_state_main.cpp — a stand-alone program over csrc/pt_ctx_state.hpp and the stand-in context of tests/ctx_state_shim.cpp for
// a sanitizer build (tests/test_ctx_state.py compiles it with -fsanitize=address,undefined and runs it as a child).  The walks of
// the Python test: every change from every combination of the flags against the rows stated here, the tallies' transitions with
// their numbers (the 64-bit products included: a signed or 32-bit overflow is the sanitizers'), the partitions.
// Exit status 0: every check held.
#include "ctx_state_shim.cpp"

#include <cstdio>

namespace {
int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad++ < 10) std::printf("line %d: %s\n", __LINE__, #c); } } while (0)

enum : uint32_t { F = 1, H = 2, A = 4, U = 8, G = 16, S = 32, P = 64 };  // feat, hist, adapt, uuid, grid cells build, spheres, params
struct Want { uint32_t drops, makes; bool gen; };
const Want kWant[] = {
    {S | U | F | H, 0, false}, {G | A, S, true}, {F, P, false}, {F | H, 0, false}, {F | H | A, P, false}, {P | F | H | A, 0, false},
    {U | F, 0, false}, {A, 0, false}, {A, 0, false}, {0, A, false}, {H, 0, false}, {0, U, false}, {G, 0, false}, {0, G, false}};

void changes() {
  CHECK(ctx_change_count() == (int)(sizeof kWant / sizeof kWant[0]));
  for (int ch = 0; ch < ctx_change_count(); ch++)
    for (uint32_t bits = 0; bits < (1u << N_FLAGS); bits++) {
      uint64_t out[3];
      ctx_changed(ch, bits, out);
      CHECK(out[0] == ((bits & ~kWant[ch].drops) | kWant[ch].makes));
      CHECK(out[1] == (kWant[ch].gen ? 42u : 41u) && out[2] == 1);
    }
}

struct T4 { uint64_t v[4]; };
T4 apply(T4 s, int op, uint64_t a = 0, uint64_t b = 0, uint64_t c = 0, uint64_t d = 0) {
  const int nothing = tally_apply(s.v, op, a, b, c, d);
  CHECK(nothing == (s.v[0] == 0 && s.v[1] == 0 ? 1 : 0));
  return s;
}
bool is(const T4& s, uint64_t spp, uint64_t captured, uint64_t launches, uint64_t samples) {
  return s.v[0] == spp && s.v[1] == captured && s.v[2] == launches && s.v[3] == samples;
}

void tallies() {
  const T4 s0 = {{12, 1, 7, 46080}};
  CHECK(is(apply(s0, T_EMPTIED), 0, 0, 0, 0));
  CHECK(is(apply(s0, T_REPARTITIONED), 0, 0, 7, 46080));
  CHECK(is(apply(s0, T_OWN_FRESH), 0, 1, 7, 46080));
  CHECK(is(apply(s0, T_REBOUND), 0, 1, 7, 46080));
  CHECK(is(apply(s0, T_LOADED, 5, 960), 5, 0, 7, 4800));
  CHECK(is(apply(s0, T_LOADED, 0, 960), 0, 0, 7, 0));
  CHECK(is(apply(s0, T_LOADED, 16777215, 960), 16777215, 0, 7, 16777215ull * 960));
  CHECK(is(apply(s0, T_LOADED, 16777215, 1ull << 30), 16777215, 0, 7, 16777215ull << 30));
  CHECK(is(apply(s0, T_UNIFORM, 0, 960, 3, 4), 24, 1, 8, 46080 + 11520));
  CHECK(is(apply(s0, T_UNIFORM, 1, 960, 3, 4), 12, 1, 7, 46080));
  CHECK(is(apply(T4{{12, 0, 7, 46080}}, T_UNIFORM, 1, 960, 3, 4), 12, 1, 7, 46080));
  CHECK(is(apply(s0, T_FRAMES, 1, 960, 4), 12, 1, 8, 46080 + 3840));
  CHECK(is(apply(s0, T_FRAMES, 70, 960, 2), 12, 1, 77, 46080 + 134400));
  CHECK(is(apply(s0, T_PARTIAL, 200, 2, 4), 12, 1, 8, 46080 + 1600));
  CHECK(is(apply(T4{{0, 0, 0, 0}}, T_UNIFORM, 0, 1ull << 31, 8, 64), 512, 0, 1, 1ull << 40));
}

void partitions() {
  const uint32_t every[4][3] = {{8, 0, 1}, {0, 0, 0}, {0, 3, 5}, {8, 0, 0}};
  const uint32_t bands[3][3] = {{4, 1, 3}, {4, 2, 3}, {1, 0, 2}};
  for (const auto& e : every) {
    uint32_t out[3];
    CHECK(partition_get(e[0], e[1], e[2], out) == 1 && out[0] == 0 && out[1] == 0 && out[2] == 1);
    for (const auto& o : every) CHECK(partition_equal(e[0], e[1], e[2], o[0], o[1], o[2]) == 1);
    for (const auto& b : bands) CHECK(partition_equal(e[0], e[1], e[2], b[0], b[1], b[2]) == 0);
  }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      uint32_t out[3];
      CHECK(partition_get(bands[i][0], bands[i][1], bands[i][2], out) == 0 && out[0] == bands[i][0] && out[1] == bands[i][1] && out[2] == bands[i][2]);
      CHECK(partition_equal(bands[i][0], bands[i][1], bands[i][2], bands[j][0], bands[j][1], bands[j][2]) == (i == j ? 1 : 0));
    }
}
}  // namespace

int main() {
  changes();
  tallies();
  partitions();
  std::printf("ctx_state: %s\n", bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}
