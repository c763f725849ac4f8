// What the mesh pipeline's entry points share on the host: the item cap, the grid of a 256-thread launch, and the ONE
// description of a scratch buffer - a bump carver that hands out 256-byte aligned planes in the order they are taken.
// The same function sizes a buffer (no base: only the running size counts) and carves it (base given: pointers).
#pragma once
#include <cstddef>

namespace mgs {

constexpr long long kMaxItems = ((1ll << 31) - 1) / 3;    // 3 n < 2^31: 32-bit element indices of [n,3] arrays

inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int grid_of(long long n) { return (int)((n + 255) / 256); }      // workgroups of 256 threads over n items

struct Carver {
  char* base;         // null: sizing only
  size_t bytes = 0;   // of the planes taken so far
  explicit Carver(void* p) : base(static_cast<char*>(p)) {}
  // the next plane, n elements of T padded to 256 bytes (one element: a fixed 256-byte slot)
  template <class T>
  T* take(size_t n = 1) {
    T* p = base ? reinterpret_cast<T*>(base + bytes) : nullptr;
    bytes += pad256(sizeof(T) * n);
    return p;
  }
};

// the size of the buffer that `carve(base, sizes..., &bytes)` describes: what a *_scratch_bytes entry point returns
template <class Carve, class... N>
inline size_t carved_bytes(Carve carve, N... sizes) {
  size_t bytes = 0;
  carve(nullptr, sizes..., &bytes);
  return bytes;
}

}  // namespace mgs
