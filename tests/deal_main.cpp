// deal_main.cpp — a stand-alone program over csrc/pt_deal.hpp for a sanitizer build (tests/test_deal.py compiles it with
// -fsanitize=address,undefined and runs it), through the entries of tests/deal_shim.cpp: the launches of the Python test, with
// the per-item tallies in exactly-sized heap arrays, so that an item number past the queue's end is seen as a write past the
// array.  Exit status 0: every launch ended with every item decoded exactly once.
#include "deal_shim.cpp"

#include <cstdio>
#include <vector>

static int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad++ < 10) std::printf("line %d: %s\n", __LINE__, #c); } } while (0)

static void launch(uint32_t n_items, uint32_t chunk, uint32_t n_waves, uint32_t mode, uint32_t groups, uint32_t seed, uint32_t max_len,
                   uint32_t drop, uint32_t ahead = 1u) {
  std::vector<uint32_t> decoded(n_items, 0u);
  unsigned long long st[6] = {0, 0, 0, 0, 0, 0};
  const unsigned long long bound = 64ull + 8ull * ((unsigned long long)n_items * max_len + (unsigned long long)n_items / chunk + n_waves + 1ull);
  const int rc = deal_simulate(n_items, chunk, n_waves, mode, groups, seed, max_len, drop, ahead, bound, decoded.data(), st);
  if (rc != 0) std::printf("n_items %u chunk %u waves %u mode %u: invariant %d\n", n_items, chunk, n_waves, mode, rc);
  CHECK(rc == 0);
  unsigned long long total = 0;
  for (uint32_t d : decoded) { CHECK(d == 1u); total += d; }
  CHECK(st[2] == total);        // lanes served by the decode = items
  CHECK(st[3] <= total);        // promotions = items that were not dropped
  if (drop == 0u) CHECK(st[3] == total);
}

int main() {
  const uint32_t chunks[3] = {32u, 64u, 512u};
  for (uint32_t mode = 0; mode < 3; mode++)
    for (uint32_t chunk : chunks) {
      const uint32_t counts[8] = {0u, 1u, 63u, 64u, 65u, chunk - 1u, chunk, chunk + 1u};
      for (uint32_t n_items : counts)
        for (uint32_t n_waves : {1u, 3u, 8u})
          for (uint32_t max_len : {1u, 3u, 46u})
            for (uint32_t ahead : {1u, 0u})
              launch(n_items, chunk, n_waves, mode, mode == 2u ? (n_waves >= 4u ? 4u : 1u) : 0u, 17u * chunk + n_items + max_len, max_len,
                     max_len == 3u ? 20u : 0u, ahead);
    }
  launch(20000u, 64u, 12u, 0u, 0u, 5u, 46u, 3u);
  launch(20000u, 64u, 12u, 1u, 0u, 6u, 46u, 3u);
  launch(20000u, 64u, 12u, 2u, 8u, 7u, 46u, 3u);
  launch(20000u, 64u, 12u, 0u, 0u, 8u, 46u, 3u, 0u);
  std::printf("deal: %s\n", bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}
