// reproject_estimate_main.cpp — a stand-alone program over csrc/pt_reproject.hpp's reproject_pixel_estimate (the per-pixel
// statements pt_reproject_estimate_kernel runs) for a sanitizer build (tests/test_reproject_estimate_ref.py compiles it with
// -fsanitize=address,undefined and runs it on the files it writes).  Every buffer is an exactly-sized std::vector read through at():
// a gather index that leaves the history planes, the accumulation or the STATE throws, a read past an allocation is the address
// sanitizer's.  Per file, one frame:
//     uint32 x 6   width, height, local rows, band_rows, band_index, band_count;  uint32 S (samples per pixel of the folded passes)
//     float  x 2   cap_diffuse, cap_other;  float x 16 the history view's constants
//     then texels of 16 bytes each: rows * width of current ids, current point, history ids, history point, accumulation;
//     2 * rows * width of the state; rows * width of the expected accumulation; 2 * rows * width of the expected state
// Exit status 0: every texel of both outputs agreed bit for bit (NaN with NaN).
#include "reproject_estimate_shim.cpp"

#include <cstdio>
#include <cstring>
#include <vector>

namespace {
int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad++ < 10) std::printf("line %d: %s\n", __LINE__, #c); } } while (0)

template <class T>
bool read_n(std::FILE* fp, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, fp) == n;
}
bool same_float(float a, float b) {
  uint32_t x, y;
  std::memcpy(&x, &a, 4);
  std::memcpy(&y, &b, 4);
  return x == y || (a != a && b != b);
}
bool same_texel(ptrep::F4 a, ptrep::F4 b) {
  return same_float(a.x, b.x) && same_float(a.y, b.y) && same_float(a.z, b.z) && same_float(a.w, b.w);
}

struct CheckedMem {
  const std::vector<ptrep::I4>* h_ids; const std::vector<ptrep::F4>* h_pnt; const std::vector<ptrep::F4>* accum;
  const std::vector<ptrep::F4>* err;
  ptrep::I4 hids(size_t i) const { return h_ids->at(i); }
  ptrep::F4 hpnt(size_t i) const { return h_pnt->at(i); }
  ptrep::F4 acc(size_t i) const { return accum->at(i); }
  ptrep::F4 errA(size_t i) const { return err->at(2 * i); }
  ptrep::F4 errB(size_t i) const { return err->at(2 * i + 1); }
};
struct CheckedCur {
  const std::vector<ptrep::I4>* c_ids; const std::vector<ptrep::F4>* c_pnt;
  ptrep::I4 ids(size_t i) const { return c_ids->at(i); }
  ptrep::F4 pnt(size_t i) const { return c_pnt->at(i); }
};
struct CheckedOut {
  std::vector<ptrep::F4>* o; std::vector<ptrep::F4>* e;
  void put(size_t i, ptrep::F4 v) { o->at(i) = v; }
  void put_state(size_t i, ptrep::F4 a, ptrep::F4 b) { e->at(2 * i) = a; e->at(2 * i + 1) = b; }
};

void one_file(const char* path) {
  std::FILE* fp = std::fopen(path, "rb");
  if (!fp) { std::printf("cannot open %s\n", path); bad++; return; }
  std::vector<uint32_t> frame6, spp;
  std::vector<float> caps, k16;
  bool ok = read_n(fp, frame6, 6) && read_n(fp, spp, 1) && read_n(fp, caps, 2) && read_n(fp, k16, 16);
  std::vector<ptrep::I4> cur_ids, hist_ids;
  std::vector<ptrep::F4> cur_pnt, hist_pnt, accum, state, expect, expect_state;
  const size_t n = ok ? (size_t)frame6.at(0) * frame6.at(2) : 0;
  ok = ok && read_n(fp, cur_ids, n) && read_n(fp, cur_pnt, n) && read_n(fp, hist_ids, n) && read_n(fp, hist_pnt, n) &&
       read_n(fp, accum, n) && read_n(fp, state, 2 * n) && read_n(fp, expect, n) && read_n(fp, expect_state, 2 * n);
  std::fclose(fp);
  if (!ok || spp.at(0) == 0u) { std::printf("%s: short file\n", path); bad++; return; }
  const ptrep::Frame f = {frame6.at(0), frame6.at(1), frame6.at(2), frame6.at(3), frame6.at(4), frame6.at(5)};
  std::vector<ptrep::F4> out(n), out_state(2 * n);
  const CheckedCur cur = {&cur_ids, &cur_pnt};
  const CheckedMem mem = {&hist_ids, &hist_pnt, &accum, &state};
  CheckedOut o = {&out, &out_state};
  run_frame_estimate(consts_of(k16.data(), caps.at(0), caps.at(1)), ptrep::est_consts((int)spp.at(0), caps.at(0), caps.at(1)), f, cur,
                     mem, o);
  for (size_t i = 0; i < n; i++) CHECK(same_texel(out.at(i), expect.at(i)));
  for (size_t i = 0; i < 2 * n; i++) CHECK(same_texel(out_state.at(i), expect_state.at(i)));
}
}  // namespace

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++) one_file(argv[i]);
  CHECK(argc > 1);
  std::printf("reproject estimate: %s (%d files)\n", bad ? "MISMATCH" : "ok", argc - 1);
  return bad ? 1 : 0;
}
