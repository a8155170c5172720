// A cache policy per ACCESS instead of per kernel: 16-byte loads and stores of a [D][ld] array's row, the policy a template
// argument, so one kernel can keep one array in the XCDs' L2s and pass another by them (profiles/cache_tiles.md, section 8).
//   PLAIN, NT         ordinary pointer accesses (*p, __builtin_nontemporal_load / _store): global_load / _store_dwordx4 [nt]
//   SC1, SC0_SC1,     buffer_load / _store_dwordx4 with the scope bits; on gfx950 a store with sc1 writes through the L2 and
//   SC0_SC1_NT        drops the line, a load with sc1 passes the CU's L1.  The value IS the instruction's aux operand
//                     (bit 0 sc0, bit 1 nt, bit 4 sc1).
// A row is addressed through a buffer resource on its base pointer with a 32-bit byte offset: rows of less than 4 GiB.  The
// resource's size is the row's, so an offset past it loads zeros and stores nothing (the callers guard the column anyway).
// Included from bk_tile_kernels.hpp and tools/cache_tile_bench.hip only -- not from the bk_source_* headers, whose text keys
// every cached from-source library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bkm {

typedef double dvec2 __attribute__((ext_vector_type(2)));  // (the same type as bkt::dvec2)
typedef uint32_t uvec4 __attribute__((ext_vector_type(4)));

enum Policy : int { PLAIN = 0, NT = 2, SC1 = 16, SC0_SC1 = 17, SC0_SC1_NT = 19 };

// one row of an array: `bytes` = the part of it the launch may touch (columns [0, C) of the row: 8 C)
struct Row {
  const double* base;
  uint32_t bytes;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const Row& r) {
  // dword 3 of a gfx9 raw buffer: DATA_FORMAT = 32 bits (0x00020000); stride 0, so the offset is checked against `bytes`
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(r.base), (short)0, (int)r.bytes, 0x00020000);
}

// the two chains at doubles [2 c2, 2 c2 + 2) of the row
template <int P>
__device__ __forceinline__ dvec2 load16(const Row& r, uint32_t c2) {
  static_assert(P == PLAIN || P == NT || P == SC1 || P == SC0_SC1 || P == SC0_SC1_NT, "unknown policy");
  if constexpr (P == PLAIN) {
    return *reinterpret_cast<const dvec2*>(r.base + 2 * (int64_t)c2);
  } else if constexpr (P == NT) {
    return __builtin_nontemporal_load(reinterpret_cast<const dvec2*>(r.base + 2 * (int64_t)c2));
  } else {
    const uvec4 v = __builtin_amdgcn_raw_buffer_load_b128(row_rsrc(r), (int)(16u * c2), 0, P);
    return __builtin_bit_cast(dvec2, v);
  }
}

template <int P>
__device__ __forceinline__ void store16(dvec2 v, const Row& r, uint32_t c2) {
  static_assert(P == PLAIN || P == NT || P == SC1 || P == SC0_SC1 || P == SC0_SC1_NT, "unknown policy");
  if constexpr (P == PLAIN) {
    *reinterpret_cast<dvec2*>(const_cast<double*>(r.base) + 2 * (int64_t)c2) = v;
  } else if constexpr (P == NT) {
    __builtin_nontemporal_store(v, reinterpret_cast<dvec2*>(const_cast<double*>(r.base) + 2 * (int64_t)c2));
  } else {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uvec4, v), row_rsrc(r), (int)(16u * c2), 0, P);
  }
}

}  // namespace bkm
