// The contig store and S-mer index of the read mapper (wf_map.hip builds them; wf_search.hip
// and wf_search_gap.hip read them): the device buffers kept in a context, the kernels' view of
// them, and the device helpers those files use.  Included by those three translation units
// only; everything here has internal linkage.
#pragma once

#include <string>

#include "wf_internal.h"

namespace wf {

struct MapBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

struct SearchState;

struct MapState {
  // the index (kept between calls)
  MapBuf pk, nm, coff, keys, kpos, bucket;
  int n_contigs = 0, seed_len = 0, max_occ = 0, bshift = 0;
  int64_t total = 0, n_kmers = 0;
  bool have_index = false;
  // the low-complexity mask of the contigs (wf_dust.hip, wf_search_mask): one bit per store
  // position, laid out as nm.  have_mask: the index holds only the S-mers without a masked
  // base; map_index clears it.  n_kmers_plain: the S-mers of the index without a mask.
  MapBuf dm;
  bool have_mask = false;
  int64_t n_kmers_plain = 0;
  // read staging (host-resident calls)
  MapBuf s1, o1, s2, o2, r_contig, r_pos1, r_pos2, r_strand, r_mm1, r_mm2;
  // the gapped pass: its result staging and the list of pairs to rescue
  MapBuf r_d1, r_d2, r_k1, r_k2, r_flags, g_flag, g_slot, g_idx, g_tmp;
  // the homology search's staging (wf_search.hip), made by its first call
  SearchState* search = nullptr;
};

void search_destroy(SearchState* ss);

// (wf_map.hip) The S-mer index of the store the state holds, built anew: flag, scan, emit,
// sort, bucket.  dm null: every S-mer without an N that stays in its contig; else only those
// whose S bases are all unmasked in dm.  Sets keys, kpos, bucket, bshift and n_kmers.
int map_build_index(MapState* st, const uint32_t* dm, hipStream_t s, std::string* err);

namespace {

struct MapIndexView {
  const uint2* pk;            // [words + 2] x: low plane, y: high plane
  const uint32_t* nm;         // [words + 2] N plane
  const int32_t* coff;        // [n_contigs + 1] start of each contig in the store
  const uint64_t* keys;       // [n_kmers] sorted
  const int32_t* kpos;        // [n_kmers] position of each sorted S-mer
  const uint32_t* bucket;     // [2^bits + 1]
  int n_contigs, S, bshift;
  const uint32_t* dm;         // [words + 2] low-complexity mask plane; null: no mask
};

// A0 C1 G2 T3, anything else 4 (N); lower case counts as upper
__device__ __forceinline__ int base_code(unsigned char ch) {
  if (ch >= 'a' && ch <= 'z') ch -= 32;
  return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4;
}

// bits [sh, sh + 32) of the 64-bit value hi:lo
__device__ __forceinline__ uint32_t window32(uint32_t lo, uint32_t hi, int sh) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
}

// the contig that holds store position g (0 <= g < total): the last c with coff[c] <= g, so
// empty contigs (which share their successor's start) are never returned
__device__ __forceinline__ int contig_of(const int32_t* coff, int n, int g) {
  int lo = 0, hi = n;                    // invariant: coff[lo] <= g < coff[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (coff[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void k_map_pack(const unsigned char* seq, int64_t total, int64_t words, uint2* pk, uint32_t* nm) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= words) return;
  uint32_t lo = 0, hi = 0, n = 0;
  for (int b = 0; b < 32; ++b) {
    const int64_t i = w * 32 + b;
    const int code = i < total ? base_code(seq[i]) : 4;      // the padding is N
    lo |= (uint32_t)(code & 1) << b;
    hi |= (uint32_t)((code >> 1) & 1) << b;
    n |= (uint32_t)(code >> 2) << b;
  }
  pk[w] = make_uint2(lo & ~n, hi & ~n);
  nm[w] = n;
}

// the S-mer at store position q: false when it holds an N
__device__ __forceinline__ bool store_kmer(const MapIndexView& ix, int q, uint64_t* key) {
  const int W = q >> 5, sh = q & 31;
  const uint32_t mask = ix.S == 32 ? 0xFFFFFFFFu : (1u << ix.S) - 1u;
  if (window32(ix.nm[W], ix.nm[W + 1], sh) & mask) return false;
  const uint2 a = ix.pk[W], b = ix.pk[W + 1];
  *key = ((uint64_t)(window32(a.y, b.y, sh) & mask) << ix.S) | (window32(a.x, b.x, sh) & mask);
  return true;
}

// mismatches of the read word at `row` (of the planes xlo, xhi, xnn) against the 32 store
// bases from position gg on.  kGuard: gg may be as low as -32; the bases before the store are N
template <bool kGuard>
__device__ __forceinline__ uint32_t map_mis_word(const MapIndexView& ix, const uint32_t* xlo, const uint32_t* xhi,
                                                 const uint32_t* xnn, int row, int gg) {
  const int W = gg >> 5, sh = gg & 31;
  uint2 a = make_uint2(0u, 0u);
  uint32_t na = ~0u;
  if (!kGuard || W >= 0) {
    a = ix.pk[W];
    na = ix.nm[W];
  }
  const uint2 b = ix.pk[W + 1];
  return (xlo[row] ^ window32(a.x, b.x, sh)) | (xhi[row] ^ window32(a.y, b.y, sh)) | xnn[row] |
         window32(na, ix.nm[W + 1], sh);
}

int map_ensure(MapBuf& b, size_t bytes, std::string* err) {
  if (bytes == 0) bytes = 16;
  if (b.bytes >= bytes) return 0;
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.bytes = 0;
  const hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) {
    *err = "hipMalloc(" + std::to_string(bytes) + ") failed: " + hipGetErrorString(e);
    return -2;
  }
  b.bytes = bytes;
  return 0;
}

void map_release(MapBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.bytes = 0;
}

MapIndexView map_view(const MapState* st) {
  MapIndexView ix{};
  ix.pk = static_cast<const uint2*>(st->pk.p);
  ix.nm = static_cast<const uint32_t*>(st->nm.p);
  ix.coff = static_cast<const int32_t*>(st->coff.p);
  ix.keys = static_cast<const uint64_t*>(st->keys.p);
  ix.kpos = static_cast<const int32_t*>(st->kpos.p);
  ix.bucket = static_cast<const uint32_t*>(st->bucket.p);
  ix.n_contigs = st->n_contigs;
  ix.S = st->seed_len;
  ix.bshift = st->bshift;
  ix.dm = st->have_mask ? static_cast<const uint32_t*>(st->dm.p) : nullptr;
  return ix;
}

#define MAP_TRY(x)                                                                      \
  do {                                                                                  \
    hipError_t e_ = (x);                                                                \
    if (e_ != hipSuccess) { *err = std::string(#x) + ": " + hipGetErrorString(e_); rc = -2; goto done; } \
  } while (0)
#define MAP_RC(x)          \
  do {                     \
    if ((rc = (x))) goto done; \
  } while (0)

}  // namespace
}  // namespace wf
