// reproject_main.cpp — a stand-alone program over csrc/pt_reproject.hpp (the per-pixel statements the kernel runs) and
// csrc/pt_reproject_plan.hpp for a sanitizer build (tests/test_reproject_plan.py compiles it with -fsanitize=address,undefined and
// runs it on the files it writes).  Every buffer is an exactly-sized std::vector read through at(): a gather index that leaves the
// history planes or the accumulation throws, a read past an allocation is the address sanitizer's.  Per file, one frame:
//     uint32 x 6   width, height, local rows, band_rows, band_index, band_count
//     float  x 12  the history camera {origin, horizontal, vertical, lower_left_corner};  float tolerance_px, cap_diffuse, cap_other
//     float  x 16  the constants the test expects (all zero with uint32 refused = 1 following: the camera must be refused)
//     uint32       refused
//     then, rows * width texels of 16 bytes each: current ids, current point, history ids, history point, accumulation, expected out
// Exit status 0: every file's constants and every texel of its output agreed bit for bit (NaN with NaN).
#include "reproject_plan_shim.cpp"

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

struct CheckedMem {
  const std::vector<ptrep::I4>* h_ids; const std::vector<ptrep::F4>* h_pnt; const std::vector<ptrep::F4>* accum;
  ptrep::I4 hids(size_t i) const { return h_ids->at(i); }
  ptrep::F4 hpnt(size_t i) const { return h_pnt->at(i); }
  ptrep::F4 acc(size_t i) const { return accum->at(i); }
};
struct CheckedCur {
  const std::vector<ptrep::I4>* c_ids; const std::vector<ptrep::F4>* c_pnt;
  ptrep::I4 ids(size_t i) const { return c_ids->at(i); }
  ptrep::F4 pnt(size_t i) const { return c_pnt->at(i); }
};
struct CheckedOut {
  std::vector<ptrep::F4>* o;
  void put(size_t i, ptrep::F4 v) { o->at(i) = v; }
};

void one_file(const char* path) {
  std::FILE* fp = std::fopen(path, "rb");
  if (!fp) { std::printf("cannot open %s\n", path); bad++; return; }
  std::vector<uint32_t> frame6, refused;
  std::vector<float> cam, opt, k_ref;
  bool ok = read_n(fp, frame6, 6) && read_n(fp, cam, 12) && read_n(fp, opt, 3) && read_n(fp, k_ref, 16) && read_n(fp, refused, 1);
  std::vector<ptrep::I4> cur_ids, hist_ids;
  std::vector<ptrep::F4> cur_pnt, hist_pnt, accum, expect;
  const size_t n = ok ? (size_t)frame6.at(0) * frame6.at(2) : 0;
  ok = ok && read_n(fp, cur_ids, n) && read_n(fp, cur_pnt, n) && read_n(fp, hist_ids, n) && read_n(fp, hist_pnt, n) &&
       read_n(fp, accum, n) && read_n(fp, expect, n);
  std::fclose(fp);
  if (!ok) { std::printf("%s: short file\n", path); bad++; return; }
  std::vector<float> k16(16, -1.0f);
  const int got = reproject_plan_constants(cam.data(), frame6.at(0), opt.at(0), k16.data());
  CHECK(got == (refused.at(0) ? 0 : 1));
  if (!got || refused.at(0)) return;
  for (size_t i = 0; i < 16; i++) CHECK(same_float(k16.at(i), k_ref.at(i)));
  const ptrep::Frame f = {frame6.at(0), frame6.at(1), frame6.at(2), frame6.at(3), frame6.at(4), frame6.at(5)};
  std::vector<ptrep::F4> out(n);
  const CheckedCur cur = {&cur_ids, &cur_pnt};
  const CheckedMem mem = {&hist_ids, &hist_pnt, &accum};
  CheckedOut o = {&out};
  run_frame(consts_of(k16.data(), opt.at(1), opt.at(2)), f, cur, mem, o);
  for (size_t i = 0; i < n; i++) {
    const ptrep::F4 a = out.at(i), b = expect.at(i);
    CHECK(same_float(a.x, b.x) && same_float(a.y, b.y) && same_float(a.z, b.z) && same_float(a.w, b.w));
  }
  // the inverse of pt_band_row: every image row is owned by exactly one band, at the local row pt_band_row counts
  for (uint32_t bc = 1; bc <= 4; bc++)
    for (uint32_t br = 1; br <= 5; br++) {
      std::vector<uint32_t> next(bc, 0u);
      for (uint32_t y = 0; y < f.height; y++) {
        uint32_t owners = 0;
        for (uint32_t bi = 0; bi < bc; bi++) {
          const ptrep::Frame g = {f.width, f.height, f.height, br, bi, bc};
          uint32_t lq = 0xdeadbeefu;
          if (ptrep::local_row_of(g, y, &lq)) { owners++; CHECK(lq == next.at(bi)); next.at(bi)++; }
        }
        CHECK(owners == 1u);
      }
    }
}
}  // namespace

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++) one_file(argv[i]);
  CHECK(argc > 1);
  std::printf("reproject: %s (%d files)\n", bad ? "MISMATCH" : "ok", argc - 1);
  return bad ? 1 : 0;
}
