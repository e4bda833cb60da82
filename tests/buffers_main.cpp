// buffers_main.cpp — a stand-alone program over csrc/pt_buffers.hpp and the stand-in allocator of tests/buffers_shim.cpp for a
// sanitizer build (tests/test_buffers.py compiles it with -fsanitize=address,undefined and runs it as a child).  The walk of
// extents the Python test states, every option on; at every step a refused allocation at every k of every set, then the fit once
// more unrefused; every option's toggle refused at every k; buffers moved, released and destroyed while they hold memory.  The
// stand-in's live count must end at zero, and a double free, a leak or a use after free in the ownership code is the sanitizers'.
// Exit status 0: every check held.
#include "buffers_shim.cpp"

#include <cstdio>
#include <cstring>
#include <memory>
#include <utility>

namespace {
int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad++ < 10) std::printf("line %d: %s\n", __LINE__, #c); } } while (0)

struct E { uint64_t pix, tiles, passes; };
E extent(uint64_t width, uint64_t rows, uint64_t passes) { return {width * rows, ((width + 7) / 8) * ((rows + 7) / 8), passes}; }
const E kWalk[] = {extent(16, 0, 1), extent(8, 8, 1), extent(9, 9, 1), extent(16, 8, 1), extent(16, 8, 3), extent(64, 40, 3),
                   extent(8, 8, 1), extent(9, 9, 1), extent(16, 16, 1)};
const int kSteps = (int)(sizeof kWalk / sizeof kWalk[0]);

ptbuf::Extent ext(const E& e) { return ptbuf::Extent(e.pix, e.tiles, e.passes); }

// every buffer that reports a capacity holds a pointer, and is written over its whole size (the address sanitizer's bounds)
void touch(const Sets& s) {
  uint64_t held[N_BUFFERS], cap[N_BUFFERS];
  all_buffers(&s, held, cap);
  for (int k = 0; k < N_BUFFERS; k++) CHECK((held[k] != 0) == (cap[k] != 0));
  auto fill = [](const auto& b) { if (b.get()) std::memset(static_cast<void*>(b.get()), 0x5a, b.capacity() * sizeof(*b.get())); };
  fill(s.frame.own_accum); fill(s.frame.slab); fill(s.frame.tile_cost); fill(s.frame.tile_order);
  fill(s.frame.tex[0]); fill(s.frame.tex[1]); fill(s.frame.canvas); fill(s.frame.resolve);
  fill(s.est.state); fill(s.est.tiles); fill(s.est.stage); fill(s.feat.planes); fill(s.query.planes); fill(s.query.order);
  fill(s.hist.planes); fill(s.hist.tally);
  CHECK(!s.frame.accum || s.frame.accum == s.frame.own_accum.get());  // never stale
}

bool fit_all(Sets& s, const E& e) {
  for (int set = 0; set < SET_COUNT; set++)
    if (!fit_set(&s, set, ext(e)).ok()) return false;
  return true;
}

std::unique_ptr<Sets> walked_to(int k) {
  std::unique_ptr<Sets> s(new Sets());
  for (int set = SET_ESTIMATE; set < SET_COUNT; set++) CHECK(buf_toggle(s.get(), set, 1, 0, 0, 1) == 0);
  for (int i = 0; i < k; i++) CHECK(fit_all(*s, kWalk[i]));
  return s;
}

void refused_fits() {
  long visited = 0;
  for (int k = 0; k < kSteps; k++)
    for (int set = 0; set < SET_COUNT; set++) {
      long n = 0;
      {
        std::unique_ptr<Sets> s = walked_to(k);
        for (int t = 0; t < set; t++) CHECK(fit_set(s.get(), t, ext(kWalk[k])).ok());
        alloc_reset();
        CHECK(fit_set(s.get(), set, ext(kWalk[k])).ok());
        n = alloc_count();
      }
      long ran = 0;
      for (long fail = 1; fail <= n; fail++, ran++) {
        std::unique_ptr<Sets> s = walked_to(k);
        for (int t = 0; t < set; t++) CHECK(fit_set(s.get(), t, ext(kWalk[k])).ok());
        alloc_fail_at(fail);
        const ptbuf::Fit f = fit_set(s.get(), set, ext(kWalk[k]));
        alloc_reset();
        CHECK(f.err != 0 && !f.capped && !set_in_place(s.get(), set, ext(kWalk[k])));
        touch(*s);
        CHECK(fit_all(*s, kWalk[k]));
        for (int t = 0; t < SET_COUNT; t++) CHECK(set_in_place(s.get(), t, ext(kWalk[k])));
        touch(*s);
      }
      CHECK(ran == n);
      visited += n;
    }
  CHECK(visited > 40);
}

void refused_toggles() {
  const E e = kWalk[3];
  for (int set = SET_ESTIMATE; set < SET_COUNT; set++) {
    Sets s;
    CHECK(fit_all(s, e));
    CHECK(buf_toggle(&s, SET_FEATURES, 1, e.pix, e.tiles, e.passes) == 0);
    if (set == SET_ESTIMATE) CHECK(buf_toggle(&s, SET_HISTORY, 1, e.pix, e.tiles, e.passes) == 0);
    if (set == SET_FEATURES) buf_toggle(&s, SET_FEATURES, 0, e.pix, e.tiles, e.passes);
    alloc_reset();
    CHECK(buf_toggle(&s, set, 1, e.pix, e.tiles, e.passes) == 0);
    const long n = alloc_count();
    buf_toggle(&s, set, 0, e.pix, e.tiles, e.passes);
    for (long fail = 1; fail <= n; fail++) {
      alloc_fail_at(fail);
      CHECK(buf_toggle(&s, set, 1, e.pix, e.tiles, e.passes) == 1);
      alloc_reset();
      CHECK(!*set_flag(&s, set) && !set_in_place(&s, set, ext(e)) && s.frame.in_place(ext(e)));
      touch(s);
    }
    CHECK(n > 0 && buf_toggle(&s, set, 1, e.pix, e.tiles, e.passes) == 0 && set_in_place(&s, set, ext(e)));
    touch(s);
  }
}

// one owner per allocation: a move leaves the source empty, an assignment frees what the target held, a release frees once
void moves() {
  ptbuf::DevBuf<Texel> a, b;
  CHECK(a.reserve(7) == 0 && b.reserve(3) == 0);
  ptbuf::DevBuf<Texel> c(std::move(a));
  CHECK(!a.get() && a.capacity() == 0 && c.holds(7));
  b = std::move(c);
  CHECK(b.holds(7));
  b.release();
  b.release();
  CHECK(!b.get() && b.capacity() == 0);
  alloc_fail_at(1);
  CHECK(b.reserve(5) != 0 && !b.get() && b.capacity() == 0);
  alloc_reset();
  CHECK(b.reserve(5) == 0 && b.holds(5) && b.holds_at_least(4) && !b.holds_at_least(6));
}
}  // namespace

int main() {
  refused_fits();
  refused_toggles();
  moves();
  CHECK(alloc_live() == 0);
  std::printf("buffers: %s\n", bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}
