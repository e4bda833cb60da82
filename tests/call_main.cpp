// call_main.cpp — csrc/pt_call.hpp (the typed kernel call) against a backend that records what a launch would have been given:
// no HIP.  Built and run by tests/test_call.py; with -DBAD=1 .. 5 the file holds one call that the type rule refuses and must
// not compile.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../ray_tracer_webgl_amd/csrc/pt_call.hpp"

namespace {
struct alignas(16) TexelA { float x, y, z, w; };
struct alignas(16) TexelB { int32_t x, y, z, w; };
struct Big { uint32_t v[6]; float f; };  // 28 bytes by value
struct Other { float v[4]; };            // 16 bytes, 4-aligned: no texel
struct Dim { unsigned x, y, z; };
using Stream = const char*;
using Kernel = ptcall::Sig<const TexelA*, uint32_t, Big, float*, int>;

struct Seen {
  const void* kernel;
  Dim grid, block;
  size_t lds;
  Stream stream;
  const TexelA* texels;
  uint32_t n;
  Big big;
  float* out;
  int mode;
} seen;

int record(const void* kernel, Dim grid, Dim block, void** slots, size_t lds, Stream stream) {
  seen.kernel = kernel; seen.grid = grid; seen.block = block; seen.lds = lds; seen.stream = stream;
  std::memcpy(&seen.texels, slots[0], sizeof seen.texels);
  std::memcpy(&seen.n, slots[1], sizeof seen.n);
  std::memcpy(&seen.big, slots[2], sizeof seen.big);
  std::memcpy(&seen.out, slots[3], sizeof seen.out);
  std::memcpy(&seen.mode, slots[4], sizeof seen.mode);
  return 7;
}

void stub(const TexelA*, uint32_t, Big, float*, int) {}
}  // namespace

int main() {
  static TexelB plane[2];
  static const TexelA const_plane[2] = {};
  static float out[4];
  static const float const_out[4] = {};
  static Other other[2];
  const Big big = {{1u, 2u, 3u, 4u, 5u, 6u}, 0.5f};
  const uint32_t n = 0xfffffff0u;
  const Dim grid = {3, 2, 1}, block = {256, 1, 1};
  const void* kernel = ptcall::handle(Kernel{}, stub);
  (void)const_plane; (void)const_out; (void)other;
#if !defined(BAD)
  // a pointer to another texel type, non-const for const; the parameters' own types for the rest
  int rc = ptcall::call(record, Kernel{}, kernel, grid, block, 48, "stream", plane, n, big, out, -2);
  bool ok = rc == 7 && seen.kernel == kernel && seen.grid.x == 3 && seen.grid.y == 2 && seen.block.x == 256 && seen.lds == 48 && !std::strcmp(seen.stream, "stream");
  ok = ok && (const void*)seen.texels == (const void*)plane && seen.n == n && !std::memcmp(&seen.big, &big, sizeof big) && seen.out == out && seen.mode == -2;
  // nullptr for either pointer, the texel type itself
  rc = ptcall::call(record, Kernel{}, kernel, grid, block, 0, "", nullptr, 1u, big, nullptr, 0);
  ok = ok && rc == 7 && seen.texels == nullptr && seen.out == nullptr && seen.n == 1u;
  rc = ptcall::call(record, Kernel{}, kernel, grid, block, 0, "", const_plane, 1u, big, out, 0);
  ok = ok && rc == 7 && seen.texels == const_plane;
  std::printf(ok ? "call: ok\n" : "call: the backend saw other values\n");
  return ok ? 0 : 1;
#elif BAD == 1  // int for uint32_t
  return ptcall::call(record, Kernel{}, kernel, grid, block, 0, "", plane, 1, big, out, 0);
#elif BAD == 2  // float for uint32_t
  return ptcall::call(record, Kernel{}, kernel, grid, block, 0, "", plane, 1.0f, big, out, 0);
#elif BAD == 3  // one argument short
  return ptcall::call(record, Kernel{}, kernel, grid, block, 0, "", plane, n, big, out);
#elif BAD == 4  // const T* for T*
  return ptcall::call(record, Kernel{}, kernel, grid, block, 0, "", plane, n, big, const_out, 0);
#elif BAD == 5  // a foreign pointee
  return ptcall::call(record, Kernel{}, kernel, grid, block, 0, "", other, n, big, out, 0);
#elif BAD == 6  // a kernel of another type than its signature
  return ptcall::handle(ptcall::Sig<const TexelA*, uint32_t, Big, float*, uint32_t>{}, stub) != nullptr;
#endif
}
