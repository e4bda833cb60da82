// filter_plan_main.cpp — a stand-alone program over csrc/pt_error_plan.hpp's chunk_rows for a sanitizer build
// (tests/test_filter_plan.py compiles it with -fsanitize=address,undefined and runs it): every height up to 40 x band_rows 0 to 9,
// the bounds written into an exactly-sized heap array and held against a chunk index computed row by row, then heights and chunk
// heights at the top of 32 bits, where an unsigned wrap would show.  Exit status 0: everything agreed.
#include "filter_plan_shim.cpp"

#include <cstdio>
#include <vector>

static int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad++ < 10) std::printf("line %d: %s\n", __LINE__, #c); } } while (0)

static void shape(uint32_t rows, uint32_t band_rows) {
  std::vector<uint32_t> chunk(rows);
  for (uint32_t ly = 0; ly < rows; ly++) chunk[ly] = band_rows ? ly / band_rows : 0u;
  for (uint32_t ly = 0; ly < rows; ly++) {
    std::vector<uint32_t> fl(2, 0xdeadbeefu);
    filter_plan_chunk_rows(ly, band_rows, rows, fl.data());
    CHECK(fl[0] <= ly && ly <= fl[1] && fl[1] < rows);
    for (uint32_t q = 0; q < rows; q++) CHECK((chunk[q] == chunk[ly]) == (q >= fl[0] && q <= fl[1]));
  }
}

int main() {
  for (uint32_t rows = 1; rows <= 40; rows++)
    for (uint32_t band_rows = 0; band_rows <= 9; band_rows++) shape(rows, band_rows);
  const uint32_t top = 0xffffffffu;
  uint32_t fl[2];
  filter_plan_chunk_rows(top - 1u, 0u, top, fl);
  CHECK(fl[0] == 0u && fl[1] == top - 1u);
  filter_plan_chunk_rows(top - 1u, top, top, fl);                 // one chunk as high as the image
  CHECK(fl[0] == 0u && fl[1] == top - 1u);
  filter_plan_chunk_rows(top - 1u, 0x80000000u, top, fl);         // the last chunk partial, first + band_rows would wrap
  CHECK(fl[0] == 0x80000000u && fl[1] == top - 1u);
  filter_plan_chunk_rows(7u, 1u, top, fl);
  CHECK(fl[0] == 7u && fl[1] == 7u);
  std::printf("filter plan: %s\n", bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}
