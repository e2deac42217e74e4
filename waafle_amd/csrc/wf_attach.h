// Hits -> attachments (orgscorer.py:359-392): the one definition of each rule for k_triage,
// k_count, k_wave and k_att_contig.  What a kernel loads and when, and where its attachments
// go, stay with the kernel; the packed hit word (pack_hit_key, key_*) is in wf_internal.h.
#pragma once
#include "wf_device.h"

namespace wf {

constexpr int kXcds = 8;             // MI355X: 8 XCDs of 32 CUs, each with its own L2

// XCD-aware contig order of a persistent grid.  Workgroups are dealt to the XCDs round-robin
// (blockIdx % 8), so under a plain grid stride the record fields of 8 neighbouring contigs
// (1-8 B each) share cache lines that 8 L2s write back partially.  Instead XCD x's j-th
// workgroup takes contig (8 k + x) * B + j at step k (B = grid / 8): runs of B contigs per XCD.
struct XcdOrder {
  bool xmap;
  int xb, xj, xx;
  __device__ __forceinline__ int at(int it) const {
    return xmap ? (it * kXcds + xx) * xb + xj : (int)blockIdx.x + it * (int)gridDim.x;
  }
};
__device__ __forceinline__ XcdOrder xcd_order() {
  return XcdOrder{gridDim.x % kXcds == 0, (int)gridDim.x / kXcds, (int)blockIdx.x / kXcds, (int)blockIdx.x % kXcds};
}

// A locus (:373): first and last site whichever way the GFF row runs, and the strand code.
struct Locus {
  int lo, hi, st;
  __device__ __forceinline__ int len() const { return hi - lo + 1; }
};
__device__ __forceinline__ Locus load_locus(const KArgs& K, int64_t i) {
  const int a = K.lstart[i], e = K.lend[i];
  return Locus{min(a, e), max(a, e), K.lstrand[i]};
}

// Loci ascending and disjoint (the usual GFF): with min_overlap > 0 a hit attaches only to
// loci it overlaps, a run found by binary search and walked in GFF order -- O(H log G), not
// a test of every locus per hit.  The test of one locus against the one before it ...
__device__ __forceinline__ bool locus_out_of_order(int lo, int prev_hi) { return lo <= prev_hi; }
// ... and of a contig's loci, lane g holding locus g < G.
__device__ __forceinline__ bool wave_loci_ordered(int lane, int G, int lo, int hi) {
  const int prev_hi = __shfl_up(hi, 1, 64);
  return __ballot(lane >= 1 && lane < G && locus_out_of_order(lo, prev_hi)) == 0ull;
}

// Ordered loci: the first of the G <= MAXG loci whose last site last(g) is at or after qlo (or
// the last locus).  A select, not a branch per step: the lanes' searches stay in step.
template <int MAXG, class LastSite>
__device__ __forceinline__ int first_locus(int G, int qlo, LastSite last) {
  int g = 0;
#pragma unroll
  for (int k = MAXG / 2; k > 0; k >>= 1) {
    const int gk = g + k;
    g = (gk <= G && last(min(gk, G) - 1) < qlo) ? gk : g;
  }
  return g;
}

// The walk reads a contig's loci through a view V: V.lo(g), V.hi(g), V.st(g), each read only
// when asked.  The kernels stage loci as tables of first site, strand code and last site or
// (BY_LEN) length ...
template <bool BY_LEN>
struct LociTables {
  const int *los, *ends;
  const int8_t* sts;
  __device__ __forceinline__ int lo(int g) const { return los[g]; }
  __device__ __forceinline__ int hi(int g) const { return BY_LEN ? los[g] + ends[g] - 1 : ends[g]; }
  __device__ __forceinline__ int st(int g) const { return sts[g]; }
};
using LociByEnd = LociTables<false>;
using LociByLen = LociTables<true>;
// ... the first n_lds loci there and the others in the batch, for the walk over every locus.
struct LociOrBatch {
  LociByLen V;
  const KArgs& K;
  int64_t l0;                        // the contig's first locus in the batch
  int n_lds;
  __device__ __forceinline__ Locus at(int g) const {
    return g < n_lds ? Locus{V.lo(g), V.hi(g), V.st(g)} : load_locus(K, l0 + g);
  }
  __device__ __forceinline__ int lo(int g) const { return at(g).lo; }
  __device__ __forceinline__ int hi(int g) const { return at(g).hi; }
  __device__ __forceinline__ int st(int g) const { return at(g).st; }
};

// f(g) for the loci g0 <= g < G a hit attaches to, in GFF order (:361-368).  ORDERED: from
// first_locus to the first locus that starts past qhi; else every locus is tried.  hs is the
// hit's strand bit, which attaches() reads only with --stranded.
template <bool ORDERED, class Loci, class F>
__device__ __forceinline__ void each_attached(const DevParams& P, const Loci& V, int g0, int G, int qlo, int qhi,
                                              int hs, F f) {
  for (int g = g0; g < G; ++g) {
    const int lo = V.lo(g);
    if (ORDERED && lo > qhi) break;
    if (attaches(P, qlo, qhi, hs, lo, V.hi(g) - lo + 1, V.st(g))) f(g);
  }
}

// Sites [start, stop) of a hit on a locus: site[h1:h2+1] under python's slice rules (:373-382).
// A negative stop (--min-overlap 0, a hit ending before the locus) wraps once; stop <= start: empty.
struct SiteRange { int start, stop; };
__device__ __forceinline__ SiteRange site_range(int qlo, int qhi, int lo, int len) {
  const int h1s = max(0, qlo - lo);
  const int h2s = min(len - 1, qhi - lo);
  const int start = min(h1s, len);
  int stop = h2s + 1;
  if (stop < 0) { stop += len; if (stop < 0) stop = 0; }
  return SiteRange{start, stop};
}

// numpy leaves of a locus of len sites: whole 8192-site buffers and the rest (the LUT's counts)
__device__ __forceinline__ int numpy_leaves(const SArgs& S, int len) {
  return (len / kNpyBuf) * (S.lut_off[kNpyBuf + 1] - S.lut_off[kNpyBuf]) +
         (S.lut_off[len % kNpyBuf + 1] - S.lut_off[len % kNpyBuf]);
}

// Annotation transfer (:383-392): per (locus, system) the last hit whose score is the best at or
// above the threshold.  Two passes with a barrier between; slot0: the locus's first table slot.
__device__ __forceinline__ bool annotates(const DevParams& P, uint32_t systems, double sc) {
  return systems != 0u && sc >= P.annot_ref;
}
// pass 1: the best score's bits (scores are >= 0, so the bits order as the scores)
template <class T>
__device__ __forceinline__ void annot_best_score(T* best, int slot0, int nsys, uint32_t systems, double sc) {
  for (int s = 0; s < nsys; ++s)
    if ((systems >> s) & 1u) atomicMax(&best[slot0 + s], (T)dbits(sc));
}
// pass 2: the largest hit index at that score
template <class T>
__device__ __forceinline__ void annot_last_hit(const T* best, int* hit, int slot0, int nsys, uint32_t systems,
                                               double sc, int h) {
  for (int s = 0; s < nsys; ++s)
    if (((systems >> s) & 1u) && best[slot0 + s] == (T)dbits(sc)) atomicMax(&hit[slot0 + s], h);
}

}  // namespace wf
