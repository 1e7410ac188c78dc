// sfmx_edge_table.h — the lock-free table of a mesh's undirected edges that smooth.hip and fill.hip
// build: open addressing over uint64 keys lo << 32 | hi (all ones = empty, a power-of-two number of slots >= 4 m), and per slot
// two int32 counters: the uses as lo -> hi (fwd) and as hi -> lo (bwd).  An insert is a 64-bit CAS on an empty slot, or a match on
// the returned occupant, else the next slot of the key's probe sequence; then an atomicAdd on the slot's counter.  Slots are
// never emptied, no thread waits for another, and a probe sequence is bounded by the table size.
#pragma once
#include <hip/hip_runtime.h>

#include "sfmx_mesh_dev.h"

constexpr unsigned long long ET_EMPTY = ~0ull;

__device__ __forceinline__ unsigned long long et_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xFF51AFD7ED558CCDull;
  k ^= k >> 33;
  k *= 0xC4CEB9FE1A85EC53ull;
  k ^= k >> 33;
  return k;
}

// Slot number `probe` of a key's probe sequence.  The first ET_LOCAL probes stay inside a window of ET_WINDOW slots that
// starts where the key's smaller end lies in the table (lo slots / 2^nbits): neighbouring vertices then share cache lines of the
// table, and the slot-ordered sweeps over it walk the vertices nearly in order.  A key that finds its window taken (a vertex
// with many edges) goes on at a hashed place and from there slot by slot.  The sequence depends on the key alone and no slot is
// ever emptied, so every thread that inserts a key meets the slot that holds it.  Against hashed places alone the smooth call
// takes 1 270 instead of 1 510 us at 256^3.
constexpr unsigned long long ET_LOCAL = 32, ET_WINDOW = 32;
__device__ __forceinline__ unsigned long long et_slot(unsigned long long key, unsigned long long hk, unsigned long long probe,
                                                      unsigned long long mask, int nbits) {
#ifndef SFMX_SM_HASHED_ONLY  // diagnostic build for the A/B of DESIGN.md 21 (tools/bench_smooth.py --build-dir): hashed places only
  if (probe < ET_LOCAL) return ((((key >> 32) * (mask + 1)) >> nbits) + ((hk + probe) & (ET_WINDOW - 1))) & mask;
  probe -= ET_LOCAL;
#endif
  return ((hk >> 8) + probe) & mask;
}

// the directed edge a -> b; one with equal ends is ignored
__device__ __forceinline__ void et_insert(int a, int b, unsigned long long* keys, int* uses, unsigned long long mask, int nbits) {
  if (a == b) return;
  const unsigned lo = (unsigned)min(a, b), hi = (unsigned)max(a, b);
  const unsigned long long key = (unsigned long long)lo << 32 | hi;
  const unsigned long long hk = et_hash(key);
  // a bounded number of probes: the table has more slots than there are edges, and no slot is ever emptied
  for (unsigned long long probe = 0; probe <= mask + ET_LOCAL; probe++) {
    const unsigned long long h = et_slot(key, hk, probe, mask, nbits);
    const unsigned long long cur = atomicCAS(&keys[h], ET_EMPTY, key);
    if (cur == ET_EMPTY || cur == key) {
      atomicAdd(&uses[2 * h + (a < b ? 0 : 1)], 1);
      return;
    }
  }
}

// one face's three directed edges; a face with an index outside [0, n) stores 1 to *flag (a plain same-value store: the call
// fails) and is skipped, so that nothing is accessed through the index
__device__ __forceinline__ void et_insert_face(const int* __restrict__ faces, int f, int n, unsigned long long* keys, int* uses,
                                               unsigned long long mask, int nbits, int* __restrict__ flag) {
  int a, b, c;
  if (!mesh_face(faces, f, n, a, b, c)) {
    *flag = 1;
    return;
  }
  et_insert(a, b, keys, uses, mask, nbits);
  et_insert(b, c, keys, uses, mask, nbits);
  et_insert(c, a, keys, uses, mask, nbits);
}

// slots of the table for m faces, and nbits with 2^nbits >= n (et_slot's window start)
static inline size_t et_slots(size_t m) {
  size_t slots = 4;
  while (slots < 4 * m) slots <<= 1;  // at most 2^32
  return slots;
}
static inline int et_nbits(int n) {
  int nbits = 1;
  while ((1ll << nbits) < n) nbits++;
  return nbits;
}
