// pt_call.hpp — TYPED KERNEL CALLS: a kernel's parameter list as a type, and the one place where an argument list becomes the
// array of pointers a launch takes.  A kernel in a translation unit of its own reaches pt_api.hip as a `const void*` (the
// accessors of pt_extra.h), so nothing compares the host's arguments with the kernel's parameters unless both name one type:
// pt_sigs.h states Sig<P...> per kernel, the kernel's unit makes its handle through handle() — which refuses a kernel of another
// type — and the host launches through call(), which refuses an argument list of another count or other types.  All at compile
// time; no HIP in here (tests/call_main.cpp runs call() against a backend of its own).
//
// THE TYPE RULE of call(): an argument's type is the parameter's type — no arithmetic conversion, not int for uint32_t, not
// double for float.  For a pointer parameter also: nullptr; a pointer to non-const for a pointer to const of the same type; and
// a pointer to one TEXEL type for a pointer to another (16 bytes, 16-aligned, trivially copyable: float4, the F4 and I4 of the
// pure headers, a kernel's private Vec4 — the planes are one memory, viewed by each header through its own struct).  Constness
// is never dropped.
#pragma once
#include <cstddef>
#include <tuple>
#include <type_traits>

namespace ptcall {

template <class... P>
struct Sig {
  using Kernel = void (*)(P...);
};

// the handle of the kernel a unit defines: only of a kernel whose type is the signature's
template <class S, class K>
const void* handle(S, K* kernel) {
  static_assert(std::is_same_v<K*, typename S::Kernel>, "the kernel's parameter list is not the one pt_sigs.h states for it");
  return reinterpret_cast<const void*>(kernel);
}

template <class T>
constexpr bool texel() {
  if constexpr (std::is_void_v<T>) return false;
  else return std::is_trivially_copyable_v<T> && sizeof(T) == 16 && alignof(T) == 16;
}

// may an argument of type A stand for a parameter of type P?
template <class P, class A>
constexpr bool accepts() {
  if constexpr (std::is_same_v<P, A>) return true;
  else if constexpr (!std::is_pointer_v<P>) return false;
  else if constexpr (std::is_null_pointer_v<A>) return true;
  else if constexpr (!std::is_pointer_v<A>) return false;
  else {
    using TP = std::remove_pointer_t<P>;
    using TA = std::remove_pointer_t<A>;
    if constexpr (std::is_const_v<TA> && !std::is_const_v<TP>) return false;
    else return std::is_same_v<std::remove_const_t<TP>, std::remove_const_t<TA>> || (texel<std::remove_const_t<TP>>() && texel<std::remove_const_t<TA>>());
  }
}

template <class P, class A>
P as_param(A a) {
  if constexpr (std::is_pointer_v<P> && std::is_pointer_v<A>) return reinterpret_cast<P>(a);
  else return a;
}

// launch(kernel, grid, block, slots, lds, stream) with slots[i] the address of parameter i's value
template <class Launch, class Dim, class Stream, class... P, class... A>
auto call(Launch&& launch, Sig<P...>, const void* kernel, Dim grid, Dim block, size_t lds, Stream stream, A... args) {
  static_assert(sizeof...(A) == sizeof...(P), "as many arguments as the kernel has parameters");
  if constexpr (sizeof...(A) == sizeof...(P)) {
    static_assert((accepts<P, A>() && ...), "every argument of its parameter's type (the type rule of pt_call.hpp)");
    if constexpr ((accepts<P, A>() && ...)) {
      std::tuple<P...> params{as_param<P>(args)...};
      return std::apply(
          [&](P&... p) {
            void* slots[] = {static_cast<void*>(&p)...};
            return launch(kernel, grid, block, slots, lds, stream);
          },
          params);
    }
  }
}

}  // namespace ptcall
