// Composite sort keys of up to a few 64-bit words, shared by the table's order (wf_order.hip)
// and the search's reporting step (wf_report.hip): every field is stored as an unsigned value
// in exactly the bits the caller proved sufficient, most significant field first, and the
// records are sorted by one stable hipcub radix sort per word, least significant word first,
// over the word's used bits only.  The kernels and key_sort are defined in wf_order.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace wf {

// v (below 2^bits) into bits [off, off + bits) of the key w[0 .. K), w[0] the least significant word
template <int K>
__device__ __forceinline__ void key_put(uint64_t (&w)[K], uint64_t v, int off, int bits) {
  if (bits == 0) return;
  const int word = off >> 6, sh = off & 63;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (k == word) w[k] |= v << sh;
    if (k == word + 1 && sh + bits > 64) w[k] |= v >> (64 - sh);
  }
}

// the bits an unsigned range needs: 0 for 0, else the position of its highest set bit + 1
inline int key_bits(uint64_t range) {
  int bits = 0;
  for (; range; range >>= 1) ++bits;
  return bits;
}

// a[i] = i, i < n; enqueued on s
int key_iota(int32_t* a, int64_t n, hipStream_t s, std::string* err);
// hipcub's scratch for key_sort of n records
int key_sort_scratch(int words, int total_bits, int n, size_t* bytes, hipStream_t s, std::string* err);
// keys: [words][n], word-major, word 0 the least significant; total_bits: the key's used bits.
// *perm holds the starting order (the identity: equal records stay in input order) and, after
// the call, the sorted one; *spare is its double buffer (the two may come back swapped).  kin,
// kout: n words each.  Enqueued on s; allocates nothing.
int key_sort(const uint64_t* keys, int words, int total_bits, int n, uint64_t* kin, uint64_t* kout, int32_t** perm,
             int32_t** spare, void* tmp, size_t tmp_bytes, hipStream_t s, std::string* err);

}  // namespace wf
