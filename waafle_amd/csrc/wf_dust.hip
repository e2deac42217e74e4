// Low-complexity mask of the contig store on MI355X (gfx950, wave64): the symmetric DUST
// definition of Morgulis et al. 2006, as DESIGN.md §12.6 states it (tests/dust_oracle.py
// restates it on the CPU).  Written from the published definition; agreement with NCBI
// dustmasker is not measured.
//
// A run is a maximal stretch of A/C/G/T inside one contig; triplet i covers bases i..i + 2;
// an interval is l <= Wd - 2 consecutive triplets of one run and scores r / (l - 1), r the sum
// of c (c - 1) / 2 over the 64 triplet kinds.  It is perfect when 10 r > Lv (l - 1) and no
// sub-interval scores strictly more; a base is masked iff a perfect interval covers it.
//
// k_dust_mask: one thread per start position, kDustBlock threads per block, of which the
//   first kDustTile are emitted and the rest are the halo.  By length: M_l(i), the greatest
//   score among the sub-intervals of (i, l), is max(s(i, l), M_{l-1}(i), M_{l-1}(i + 1)), and
//   (i, l) is perfect iff it passes the threshold and s(i, l) is no less than the other two.
//   Step l of thread i needs M_{l-1} of thread i + 1 (a wave shuffle; across waves one LDS
//   word per wave and the step's barrier), so thread t is right up to length l while
//   t + l - 1 < kDustBlock: the emitted threads are right for every l <= 62.
//   The 64 counts of a thread are 16 dwords of 4 byte counters (counts are <= 62), laid out
//   [dword][thread]: a wave's 64 lanes read 64 consecutive dwords whatever their triplets, so
//   the two 32-lane halves of an LDS access each fall on 32 distinct banks.
//   A start keeps its longest perfect length; end = i + l + 2.  The inclusive prefix maximum
//   of `end` over the emitted starts tells every position of the block (halo included: an
//   interval reaches at most 63 bases past its start) whether an interval of this tile covers
//   it; a wave's 64 flags are two words of dm, or-ed in atomically because the halo's words
//   belong to the next tile as well.
// k_dust_count: the masked bases.
// dust_mask then rebuilds the S-mer index without the S-mers that hold a masked base
// (map_build_index, wf_map.hip: k_map_flag with the mask plane as its argument).
#include <algorithm>
#include <string>

#include "wf_internal.h"
#include "wf_mapstore.h"

namespace wf {

namespace {

constexpr int kDustBlock = 512;
constexpr int kDustWaves = kDustBlock / 64;
static_assert(kDustTile == kDustBlock - 64 && kDustTile % 32 == 0,
              "an interval covers at most 64 bases; a wave's flags are whole words of dm");

// M as one word: numerator r <= 1891 (62 equal triplets), denominator l - 1 <= 61
__device__ __forceinline__ int dust_pack(int num, int den) { return num << 8 | den; }

__global__ __launch_bounds__(kDustBlock) void k_dust_mask(const MapIndexView ix, int total, int Wd, int Lv,
                                                          uint32_t* dm) {
  __shared__ uint32_t cnt[16 * kDustBlock];      // [dword of 4 counters][thread]
  __shared__ int xch[2][kDustWaves];             // lane 0's M of each wave, by step parity
  __shared__ int wmax[kDustWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i64 = (int64_t)blockIdx.x * kDustTile + tid;
  const int i = (int)std::min<int64_t>(i64, total);          // total < 2^31 - 1024
  // the bounds, before any load of bases: lmax = the triplets from i on inside its run,
  // at most Wd - 2.  Position i < total reads words W .. W + 2 <= (total - 1) / 32 + 2, the
  // last word of the planes; the padding is N, so a run ends at `total` at the latest.
  int lmax = 0;
  uint64_t lo = 0, hi = 0;
  if (i64 < total) {
    const int W = i >> 5, sh = i & 31;
    const uint32_t n0 = ix.nm[W], n1 = ix.nm[W + 1], n2 = ix.nm[W + 2];
    const uint64_t nn = (uint64_t)window32(n0, n1, sh) | ((uint64_t)window32(n1, n2, sh) << 32);
    const int c = contig_of(ix.coff, ix.n_contigs, i);
    int len = nn ? __ffsll((long long)nn) - 1 : 64;          // bases of the run from i on, <= 64
    len = min(len, ix.coff[c + 1] - i);
    lmax = max(0, min(Wd, len) - 2);
    if (lmax > 0) {
      const uint2 a = ix.pk[W], b = ix.pk[W + 1], d = ix.pk[W + 2];
      lo = (uint64_t)window32(a.x, b.x, sh) | ((uint64_t)window32(b.x, d.x, sh) << 32);
      hi = (uint64_t)window32(a.y, b.y, sh) | ((uint64_t)window32(b.y, d.y, sh) << 32);
    }
  }
  for (int w = 0; w < 16; ++w) cnt[w * kDustBlock + tid] = 0;
  int r = 0, M = dust_pack(0, 1), best = 0;
  if (lmax > 0) {                                            // l = 1: the triplet at i, score 0
    const int t = (int)(lo & 7) | (int)(hi & 7) << 3;
    cnt[(t >> 2) * kDustBlock + tid] = 1u << (8 * (t & 3));
  }
  for (int l = 2; l <= Wd - 2; ++l) {
    if (lane == 0) xch[l & 1][wave] = M;
    __syncthreads();
    int nb = __shfl_down(M, 1);
    if (lane == 63) nb = wave + 1 < kDustWaves ? xch[l & 1][wave + 1] : M;
    if (l <= lmax) {
      const int k = l - 1;                                   // the triplet at i + k joins
      const int t = (int)((lo >> k) & 7) | (int)((hi >> k) & 7) << 3;
      uint32_t* p = &cnt[(t >> 2) * kDustBlock + tid];
      const uint32_t v = *p;
      r += (int)((v >> (8 * (t & 3))) & 0xFFu);
      *p = v + (1u << (8 * (t & 3)));
      // s = r / k against M_{l-1}(i) and M_{l-1}(i + 1), by cross-products (< 2^17)
      const int an = M >> 8, ad = M & 0xFF, bn = nb >> 8, bd = nb & 0xFF;
      const bool ge = r * ad >= an * k && r * bd >= bn * k;
      if (ge && 10 * r > Lv * k) best = l;
      int mn = an, md = ad;
      if (bn * md > mn * bd) { mn = bn; md = bd; }
      if (r * md > mn * k) { mn = r; md = k; }
      M = dust_pack(mn, md);
    }
  }
  // the prefix maximum of `end` over the emitted starts
  int e = (best > 0 && tid < kDustTile) ? i + best + 2 : 0;
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(e, d);
    if (lane >= d) e = max(e, o);
  }
  if (lane == 63) wmax[wave] = e;
  __syncthreads();
  for (int w = 0; w < wave; ++w) e = max(e, wmax[w]);
  const unsigned long long bits = __ballot(e > i);           // e <= total: nothing past the store
  if (lane == 0 && bits) {
    const int W = i >> 5;                                    // i is a multiple of 32 here
    if ((uint32_t)bits) atomicOr(&dm[W], (uint32_t)bits);
    if ((uint32_t)(bits >> 32)) atomicOr(&dm[W + 1], (uint32_t)(bits >> 32));
  }
}

__global__ void k_dust_count(const uint32_t* dm, int64_t words, unsigned long long* n) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int c = w < words ? __popc(dm[w]) : 0;
  for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(n, (unsigned long long)c);
}

}  // namespace

int dust_mask(MapState* st, int window, int level, DustStats* stats, uint32_t* host_mask, hipStream_t s,
              std::string* err) {
  const int64_t total = st->total;
  const int64_t words = (total + 31) / 32 + 2;
  const int Lv = std::min(level, 20000);                     // 10 r <= 18910: nothing passes; no overflow
  DevArr<unsigned long long> d_n;
  const int rc = synced_on_error(s, [&]() -> int {
    unsigned long long masked = 0;
    MAP_RC(st->dm.ensure(words, err));
    MAP_RC(d_n.ensure(1, err));
    MAP_TRY(hipMemsetAsync(st->dm.p, 0, (size_t)words * sizeof(uint32_t), s));
    MAP_TRY(hipMemsetAsync(d_n.p, 0, sizeof(unsigned long long), s));
    if (total > 0) {
      hipLaunchKernelGGL(k_dust_mask, dim3((unsigned)((total + kDustTile - 1) / kDustTile)), dim3(kDustBlock), 0, s,
                         map_view(st), (int)total, window, Lv, st->dm.p);
      MAP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_dust_count, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, st->dm.p, words, d_n.p);
      MAP_TRY(hipGetLastError());
    }
    MAP_TRY(hipMemcpyAsync(&masked, d_n.p, sizeof masked, hipMemcpyDeviceToHost, s));
    if (host_mask && total > 0)
      MAP_TRY(hipMemcpyAsync(host_mask, st->dm.p, (size_t)((total + 31) / 32) * sizeof(uint32_t),
                             hipMemcpyDeviceToHost, s));
    MAP_TRY(hipStreamSynchronize(s));
    st->have_mask = false;                                   // until the index matches the mask
    MAP_RC(map_build_index(st, st->dm.p, s, err));
    st->have_mask = true;
    stats->masked_bases = (int64_t)masked;
    stats->kmers_before = st->n_kmers_plain;
    stats->kmers_after = st->n_kmers;
    return 0;
  });
  if (rc) st->have_index = false;                            // the index may be half built
  return rc;
}

}  // namespace wf
