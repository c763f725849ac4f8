// A hash set of item indices that keeps, per key, the SMALLEST index of the items with that key (mesh_simplify.hip: the
// vertices of a cell, the faces of a label triple).
//
//   table    uint32 [size], size a power of two >= 2 n for n items, filled with kSetEmpty; linear probing, masked wrap
//   insert   item i with home slot h: old = CAS(slot, EMPTY, i); EMPTY: done; same key as old: atomicMin(slot, i), done;
//            else the next slot
//   find     the occupant of the first slot from h on whose key is the item's
//
// A slot's key never changes once it is taken: only an item of the same key replaces its occupant.  So every key ends in
// exactly one slot - the first free one of its probe sequence at the time of its first insert - holding the smallest
// index of its items, whatever the order of arrival; and find() of a later launch meets that slot before any empty one,
// because nothing is ever removed.  With n <= size / 2 items a probe sequence always meets an empty slot; both loops are
// bounded by the table size all the same, so that a caller's mistake ends as a miss and not as a loop.
//
// Visibility.  During the insert launch every access to the table is an agent-scope atomic (workgroups on other XCDs
// write it).  `same(i, j)` - do items i and j have the same key - must read arrays written by an EARLIER launch only.
// find() belongs into a LATER launch than the inserts and reads the table plainly.
#pragma once
#include <hip/hip_runtime.h>

namespace mgs {

constexpr unsigned kSetEmpty = 0xFFFFFFFFu;

// the finaliser of MurmurHash3: what both home slots are mixed with
__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long k) {
  k ^= k >> 33; k *= 0xFF51AFD7ED558CCDull;
  k ^= k >> 33; k *= 0xC4CEB9FE1A85EC53ull;
  k ^= k >> 33;
  return k;
}

// table entries for n items: the smallest power of two >= 2 n (and >= 1)
inline unsigned long long set_table_size(unsigned long long n) {
  unsigned long long s = 1;
  while (s < 2 * n) s <<= 1;
  return s;
}

template <class Same>
__device__ __forceinline__ void set_insert(unsigned* __restrict__ table, unsigned mask, unsigned home, unsigned i, Same same) {
  unsigned slot = home & mask;
  for (unsigned probe = 0; probe <= mask; probe++, slot = (slot + 1) & mask) {
    unsigned cur = __hip_atomic_load(table + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kSetEmpty) {
      cur = atomicCAS(table + slot, kSetEmpty, i);
      if (cur == kSetEmpty) return;
    }
    if (same(cur, i)) {
      // the occupant only falls: one at or below i needs nothing from i (a stale, larger read only costs the atomic)
      if (cur > i) atomicMin(table + slot, i);
      return;
    }
  }
}

// the smallest index of the items with i's key; kSetEmpty when none was inserted
template <class Same>
__device__ __forceinline__ unsigned set_find(const unsigned* __restrict__ table, unsigned mask, unsigned home, unsigned i, Same same) {
  unsigned slot = home & mask;
  for (unsigned probe = 0; probe <= mask; probe++, slot = (slot + 1) & mask) {
    const unsigned cur = table[slot];
    if (cur == kSetEmpty) return kSetEmpty;
    if (same(cur, i)) return cur;
  }
  return kSetEmpty;
}

}  // namespace mgs
