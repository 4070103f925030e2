// (row, entry) keys for lists that may name a row several times: shared by the summing Adam step (adam_rows.hip) and the run-sum of
// the row gathers' backward (rows_sum.hip).  Entry i of a list naming row r gets the 64-bit key (r << shift) | i with
// shift = bits_for(n - 1); the keys are radix-sorted over the bits in use, so a row's entries form one run in ascending entry order.
// An entry without a row (another node type, an id outside the table) gets NO_KEY, which sorts behind every row.
#pragma once
#include <hipcub/hipcub.hpp>

#include "common.h"

namespace egnn_rows {

constexpr size_t kAlign = 256;
constexpr uint64_t NO_KEY = ~uint64_t(0);
inline size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

static inline int bits_for(uint64_t v) {  // number of bits needed to represent values in [0, v]
  int b = 1;
  while (b < 64 && (v >> b) != 0) ++b;
  return b;
}

// log2 of the lanes that serve one row of `units` 16-byte (or, on a scalar path, 4-byte) pieces: min(64, pow2ceil(units))
static inline int lanes_lg(int64_t units) {
  int lg = 0;
  while (lg < 6 && (int64_t(1) << lg) < units) ++lg;
  return lg;
}

// hipCUB sizes the sort's temporary storage from the current device's configuration: false when that query fails (no device)
static inline bool sort_keys_temp(int64_t n, int end_bit, size_t* bytes) {
  *bytes = 0;
  return hipcub::DeviceRadixSort::SortKeys(nullptr, *bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)n, 0, end_bit) == hipSuccess;
}

static inline bool sort_keys(void* temp, size_t temp_bytes, const uint64_t* keys, uint64_t* sorted, int64_t n, int end_bit, hipStream_t st) {
  return hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, keys, sorted, (int)n, 0, end_bit, st) == hipSuccess;
}

__device__ __forceinline__ uint64_t make_key(int64_t row, int shift, int64_t entry) { return ((uint64_t)row << shift) | (uint64_t)entry; }

}  // namespace egnn_rows
