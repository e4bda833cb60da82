// filter_plan_shim.cpp — the chunk-bounds arithmetic of the filtered read-out (csrc/pt_error_plan.hpp chunk_rows: the function
// pt_filter_kernel calls) behind a C entry, for tests/test_filter_plan.py.  Compiled by the tests with g++: the header is host
// code.  first_last receives the first and last local row of local row ly's chunk.
#include "../ray_tracer_webgl_amd/csrc/pt_error_plan.hpp"

extern "C" __attribute__((visibility("default"))) void filter_plan_chunk_rows(uint32_t ly, uint32_t band_rows, uint32_t local_rows,
                                                                              uint32_t* first_last) {
  const pterr::ChunkRows c = pterr::chunk_rows(ly, band_rows, local_rows);
  first_last[0] = c.first;
  first_last[1] = c.last;
}
