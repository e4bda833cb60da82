// grid_records_main.cpp — a stand-alone program over csrc/pt_grid_records.hpp for a sanitizer build (tests/test_grid_records.py
// compiles it with -fsanitize=address,undefined and runs it): every count 0 ... 255 at the firsts the Python test uses, encoded,
// decoded, walked round by round the way the kernels do and through the general functions, against the host record's own
// sequence; and the ring layout of small grids, written into exactly-sized heap arrays.  Exit status 0: everything agreed.
#include "../ray_tracer_webgl_amd/csrc/pt_grid_records.hpp"

#include <cstdio>
#include <vector>

static int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad++ < 10) std::printf("line %d: %s\n", __LINE__, #c); } } while (0)

static void rounds(uint32_t first, uint32_t count, uint32_t G, bool fast) {
  uint32_t host = first | (count << 24), rec = ptrec::from_host(host);
  for (;;) {
    const bool has_h = (host >> 24) != 0u, has_d = rec >= ptrec::kNone;
    CHECK(has_h == has_d);
    if (!has_h || !has_d) break;
    const uint32_t base = host & 0xffffffu, left = host >> 24, cand = (1u << G) - 1u;
    const uint32_t want = left >= G ? cand : (1u << left) - 1u;
    host = left > G ? (base + G) | ((left - G) << 24) : 0u;
    uint32_t m, nx;
    if (fast) {
      m = ptrec::short_mask4(rec, cand);
      nx = 0u;
      if (ptrec::is_long(rec)) { m = cand; nx = ptrec::next_long4(rec); }
    } else {
      m = cand & ptrec::round_mask(rec, G);
      nx = ptrec::next(rec, G);
    }
    CHECK(ptrec::first_of(rec) == base && m == want);
    rec = nx;
  }
}

int main() {
  for (uint32_t count = 0; count < 256; count++) {
    const uint32_t firsts[4] = {0u, 1u, 4000003u, ptrec::kEntryLimit - 1u - count};
    for (uint32_t first : firsts) {
      const uint32_t host = first | (count << 24);
      CHECK(ptrec::to_host(ptrec::from_host(host)) == host);
      CHECK(ptrec::count_of(ptrec::encode(first, count)) == count);
      rounds(first, count, 4, true);
      for (uint32_t G = 2; G <= 4; G++) rounds(first, count, G, false);
    }
  }
  CHECK(ptrec::fits(ptrec::kEntryLimit - 1u) && !ptrec::fits(ptrec::kEntryLimit) && !ptrec::fits(1u << 24));
  const uint32_t sizes[4][2] = {{1, 1}, {2, 3}, {16, 16}, {1023, 2}};
  for (const auto& s : sizes) {
    const uint32_t nx = s[0], nz = s[1];
    std::vector<uint32_t> cells((size_t)nx * nz);
    uint32_t first = 0;
    for (size_t k = 0; k < cells.size(); k++) { const uint32_t c = (uint32_t)(k * 7u % 11u); cells[k] = first | (c << 24); first += c; }
    std::vector<uint32_t> ring((size_t)ptrec::ring_cells(nx, nz), 0xdeadbeefu);
    ptrec::ring_layout(cells.data(), nx, nz, ring.data());
    size_t n_out = 0;
    for (uint32_t v : ring) n_out += v == ptrec::kOutside;
    CHECK(n_out == ring.size() - cells.size());
    for (uint32_t cz = 0; cz < nz; cz++)
      for (uint32_t cx = 0; cx < nx; cx++) {
        const uint32_t rec = ring[ptrec::ring_index(nx, cx, cz)], host = cells[(size_t)cz * nx + cx];
        CHECK(rec != ptrec::kOutside && ptrec::count_of(rec) == host >> 24 && ((host >> 24) == 0u || ptrec::to_host(rec) == host));
      }
  }
  std::printf("grid records: %s\n", bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}
