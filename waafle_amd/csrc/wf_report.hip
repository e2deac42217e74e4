// The reporting step of the homology search (DESIGN.md §12.1 "Reporting", §12.5 "Reporting",
// §12.8) on MI355X (gfx950), and its host form.  tests/report_oracle.py restates both rules on
// the CPU twice: as defined, and in the parallel form the kernels below follow.
//
// Ungapped (report_hsps_device): raw HSPs (sm, contig, delta, b, e, score) -> records.
//   k_rep_ukeys   thread per HSP: the composite key (sm, contig, delta, b, greatest e - e)
//   key_sort      (wf_keys.h) stable radix sorts, one per 64-bit word of the key
//   k_rep_umark   thread per sorted position: (head of its (sm, contig, delta) group) << 32 | e
//   inclusive scan with the segmented maximum: the greatest e of the group up to each position
//   k_rep_ukeep   an element equal to its predecessor in (group, b, e) is a duplicate; it is
//                 contained iff it is no head and the scan one position back is >= its e;
//                 containment first, then score >= min_score
//   exclusive sum of the keep flags: the slot of each record, and their number
//   k_rep_uemit   the record and its key (contig, sm, qstart, sstart, length) at its slot
//   key_sort, k_rep_gather: the records in the order of the output
// Gapped (report_alns_device): anchors and their two sides -> alignments.
//   k_rep_gbuild  thread per anchor: the alignment by the closed forms of §12.5 and its key
//                 (sm, contig, greatest score2 - score2, qstart, sstart, qspan, sspan, length,
//                 matches, gaps)
//   key_sort
//   k_rep_gmark   thread per sorted position: equal to its predecessor in every field (a
//                 duplicate); its position if it heads an (sm, contig) group; its two intervals
//   inclusive maximum scan: the first position of each element's group
//   k_rep_gcover  thread per sorted position: walks the earlier elements of its group, whatever
//                 their number, until one covers both intervals (cover is transitive, so "a
//                 kept earlier one" and "any earlier one" are the same test); then
//                 score2 >= 2 min_score
//   exclusive sum of (not a duplicate) << 32 | keep: slots, raw_alignments and the record count
//   k_rep_gemit, key_sort, k_rep_gather as above with the key of §12.5 "Record"
// Every kernel is one thread per element, checks its bound before any load, and follows only
// indices that the sorts and scans made (permutations of [0, n), group starts <= the position).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <tuple>
#include <vector>

#include "wf_keys.h"
#include "wf_mapstore.h"

namespace wf {

// ---- the host form --------------------------------------------------------------------------

void report_hsps_host(std::vector<SearchRaw>* raw_io, int min_score, std::vector<SearchRec>* recs_out) {
  std::vector<SearchRaw>& raw = *raw_io;
  std::vector<SearchRec>& recs = *recs_out;
  recs.clear();
  // per (subject, strand, contig, diagonal): by start ascending, end descending.  After the
  // identical are counted once, an HSP is strictly contained in another exactly when an
  // earlier one of its group ends at or after its end.
  std::sort(raw.begin(), raw.end(), [](const SearchRaw& x, const SearchRaw& y) {
    return std::make_tuple(x.sm, x.contig, x.delta, x.b, -x.e) < std::make_tuple(y.sm, y.contig, y.delta, y.b, -y.e);
  });
  using Rec = SearchRec;
  int reach = 0;                                 // the greatest end seen in the group
  for (size_t i = 0; i < raw.size(); ++i) {
    const SearchRaw& x = raw[i];
    const bool same = i > 0 && raw[i - 1].sm == x.sm && raw[i - 1].contig == x.contig && raw[i - 1].delta == x.delta;
    if (!same) reach = 0;
    if (same && raw[i - 1].b == x.b && raw[i - 1].e == x.e) continue;
    const bool contained = same && reach >= x.e;
    reach = std::max(reach, x.e);
    if (contained || x.score < min_score) continue;
    const int length = x.e - x.b;
    recs.push_back(Rec{x.contig, x.sm >> 1, x.sm & 1, x.b + x.delta, x.b, length, (x.score + 2 * length) / 3});
  }
  std::sort(recs.begin(), recs.end(), [](const Rec& x, const Rec& y) {
    return std::make_tuple(x.contig, x.subject, x.minus, x.qstart, x.sstart, x.length) <
           std::make_tuple(y.contig, y.subject, y.minus, y.qstart, y.sstart, y.length);
  });
}

namespace {

auto aln_key(const GapAln& x) {
  return std::make_tuple(x.sm, x.contig, -x.score2, x.qstart, x.sstart, x.qspan, x.sspan, x.length, x.matches,
                         x.gaps);
}

// the alignment of one anchor from its two sides (§12.5); host and device
__host__ __device__ __forceinline__ GapAln aln_of(const GapAnchor& an, const GapRaw& r) {
  const GapSide &L = r.left, &R = r.right;
  GapAln x;
  x.sm = an.sm;
  x.contig = an.contig;
  x.qstart = an.j0 - L.q;
  x.qspan = L.q + R.q;
  x.sstart = an.i0 - L.p;
  x.sspan = L.p + R.p;
  x.gaps = L.g + R.g;
  x.score2 = (int64_t)L.H + R.H;
  const int64_t pairs = ((int64_t)x.sspan + x.qspan - x.gaps) / 2;
  x.length = (int32_t)(pairs + x.gaps);
  x.matches = (int32_t)((x.score2 + 5 * (int64_t)x.gaps + 4 * pairs) / 6);
  return x;
}

}  // namespace

void report_alns_host(const std::vector<GapAnchor>& anchors, const std::vector<GapRaw>& raw, int min_score,
                      std::vector<GapAln>* kept_out, int64_t* raw_alignments) {
  std::vector<GapAln> alns(raw.size());
  for (size_t i = 0; i < raw.size(); ++i) alns[i] = aln_of(anchors[i], raw[i]);
  std::sort(alns.begin(), alns.end(), [](const GapAln& x, const GapAln& y) { return aln_key(x) < aln_key(y); });
  alns.erase(std::unique(alns.begin(), alns.end(),
                         [](const GapAln& x, const GapAln& y) { return aln_key(x) == aln_key(y); }),
             alns.end());
  *raw_alignments = (int64_t)alns.size();
  // per (subject, strand, contig), in score order: dropped when a kept one covers both intervals
  std::vector<GapAln>& kept = *kept_out;
  kept.clear();
  size_t g0 = 0;                                 // the group's first kept one
  for (size_t i = 0; i < alns.size(); ++i) {
    const GapAln& x = alns[i];
    if (i == 0 || alns[i - 1].sm != x.sm || alns[i - 1].contig != x.contig) g0 = kept.size();
    bool covered = false;
    for (size_t k = g0; k < kept.size() && !covered; ++k) {
      const GapAln& y = kept[k];
      covered = y.qstart <= x.qstart && x.qstart + x.qspan <= y.qstart + y.qspan && y.sstart <= x.sstart &&
                x.sstart + x.sspan <= y.sstart + y.sspan;
    }
    if (!covered) kept.push_back(x);
  }
  kept.erase(std::remove_if(kept.begin(), kept.end(),
                            [&](const GapAln& x) { return x.score2 < 2 * (int64_t)min_score; }),
             kept.end());
  std::sort(kept.begin(), kept.end(), [](const GapAln& x, const GapAln& y) {
    return std::make_tuple(x.contig, x.sm, x.qstart, x.sstart, x.qspan, x.sspan, x.length, x.matches, x.gaps) <
           std::make_tuple(y.contig, y.sm, y.qstart, y.sstart, y.qspan, y.sspan, y.length, y.matches, y.gaps);
  });
}

// ---- the device form ------------------------------------------------------------------------

namespace {

constexpr int kRepNT = 256;
constexpr int kRepWords = 6;       // 10 fields of at most 34 bits (the 64-bit score2 of two int32 sides)
constexpr uint64_t kHeadBit = 1ull << 32;

// One sort key: nf fields, the most significant first.  Field f holds x - base (desc bit clear)
// or base - x (set: descending) in `bits` bits.
struct RepKey {
  int nf, words, total_bits;
  unsigned desc;
  int64_t base[kRepFields];
  int bits[kRepFields];
};

// the key of the fields `field` (indices into B), those in `desc_mask` (bits by position) descending
RepKey make_key(const RepBounds& B, const int* field, int nf, unsigned desc_mask) {
  RepKey K{};
  K.nf = nf;
  K.desc = desc_mask;
  for (int f = 0; f < nf; ++f) {
    const int64_t lo = B.lo[field[f]], hi = B.hi[field[f]];
    K.bits[f] = key_bits((uint64_t)(hi - lo));
    K.base[f] = (desc_mask >> f & 1u) ? hi : lo;
    K.total_bits += K.bits[f];
  }
  K.words = (K.total_bits + 63) / 64;
  return K;
}

inline unsigned grid_of(int64_t n) { return (unsigned)((n + kRepNT - 1) / kRepNT); }

// x[0 .. NF) packed by K into word-major keys[k * stride + i]
template <int NF>
__device__ __forceinline__ void rep_key_store(const RepKey& K, const int64_t (&x)[NF], uint64_t* __restrict__ keys,
                                              int64_t stride, int64_t i) {
  uint64_t w[kRepWords] = {0, 0, 0, 0, 0, 0};
  int off = 0;
#pragma unroll
  for (int f = NF - 1; f >= 0; --f) {            // the last field is the least significant
    const int64_t v = (K.desc >> f & 1u) ? K.base[f] - x[f] : x[f] - K.base[f];
    key_put(w, (uint64_t)v, off, K.bits[f]);
    off += K.bits[f];
  }
#pragma unroll
  for (int k = 0; k < kRepWords; ++k)
    if (k < K.words) keys[(int64_t)k * stride + i] = w[k];
}

__global__ __launch_bounds__(kRepNT) void k_rep_ukeys(const SearchRaw* __restrict__ raw, int64_t n, RepKey K,
                                                      uint64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * kRepNT + threadIdx.x;
  if (i >= n) return;
  const SearchRaw r = raw[i];
  const int64_t x[5] = {r.sm, r.contig, r.delta, r.b, r.e};
  rep_key_store(K, x, keys, n, i);
}

__device__ __forceinline__ bool same_group(const SearchRaw& x, const SearchRaw& y) {
  return x.sm == y.sm && x.contig == y.contig && x.delta == y.delta;
}

__global__ __launch_bounds__(kRepNT) void k_rep_umark(const SearchRaw* __restrict__ raw, const int32_t* __restrict__ perm,
                                                      int64_t n, uint64_t* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * kRepNT + threadIdx.x;
  if (i >= n) return;
  const SearchRaw x = raw[perm[i]];
  const bool head = i == 0 || !same_group(raw[perm[i - 1]], x);
  val[i] = (head ? kHeadBit : 0ull) | (uint32_t)x.e;         // 0 < e < 2^31
}

// (head, e) pairs: the running maximum of e that starts anew at every head
struct SegMaxOp {
  __host__ __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const {
    if (b & kHeadBit) return b;
    const uint32_t ea = (uint32_t)a, eb = (uint32_t)b;
    return (a & kHeadBit) | (ea > eb ? ea : eb);
  }
};

__global__ __launch_bounds__(kRepNT) void k_rep_ukeep(const SearchRaw* __restrict__ raw, const int32_t* __restrict__ perm,
                                                      const uint64_t* __restrict__ run, int64_t n, int min_score,
                                                      int32_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * kRepNT + threadIdx.x;
  if (i >= n) return;
  const SearchRaw x = raw[perm[i]];
  bool drop = false;
  if (i > 0) {
    const SearchRaw p = raw[perm[i - 1]];
    if (same_group(p, x)) drop = (p.b == x.b && p.e == x.e) || (uint32_t)run[i - 1] >= (uint32_t)x.e;
  }
  keep[i] = !drop && x.score >= min_score;
}

__global__ __launch_bounds__(kRepNT) void k_rep_uemit(const SearchRaw* __restrict__ raw, const int32_t* __restrict__ perm,
                                                      const int32_t* __restrict__ keep, const int32_t* __restrict__ slot,
                                                      int64_t n, int64_t n_kept, RepKey K, SearchRec* __restrict__ rec,
                                                      uint64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * kRepNT + threadIdx.x;
  if (i >= n || !keep[i]) return;
  const int64_t k = slot[i];
  if (k >= n_kept) return;                       // the scan's total is n_kept
  const SearchRaw r = raw[perm[i]];
  const int32_t length = r.e - r.b;
  const SearchRec out{r.contig, r.sm >> 1, r.sm & 1, r.b + r.delta, r.b, length, (r.score + 2 * length) / 3};
  rec[k] = out;
  const int64_t x[5] = {r.contig, r.sm, out.qstart, r.b, length};
  rep_key_store(K, x, keys, n_kept, k);
}

template <class T>
__global__ __launch_bounds__(kRepNT) void k_rep_gather(const T* __restrict__ in, const int32_t* __restrict__ perm,
                                                       int64_t n, T* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kRepNT + threadIdx.x;
  if (i < n) out[i] = in[perm[i]];
}

__global__ __launch_bounds__(kRepNT) void k_rep_anchors(const SearchRec* __restrict__ rec, int64_t n,
                                                        GapAnchor* __restrict__ anchor) {
  const int64_t i = (int64_t)blockIdx.x * kRepNT + threadIdx.x;
  if (i >= n) return;
  const SearchRec r = rec[i];
  const int32_t i0 = r.sstart + r.length / 2;
  anchor[i] = GapAnchor{r.subject << 1 | r.minus, r.contig, i0, i0 + (r.qstart - r.sstart)};
}

__global__ __launch_bounds__(kRepNT) void k_rep_gbuild(const GapAnchor* __restrict__ anchor, const GapRaw* __restrict__ graw,
                                                       int64_t n, RepKey K, GapAln* __restrict__ aln,
                                                       uint64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * kRepNT + threadIdx.x;
  if (i >= n) return;
  const GapAln a = aln_of(anchor[i], graw[i]);
  aln[i] = a;
  const int64_t x[10] = {a.sm, a.contig, a.score2, a.qstart, a.sstart, a.qspan, a.sspan, a.length, a.matches, a.gaps};
  rep_key_store(K, x, keys, n, i);
}

__global__ __launch_bounds__(kRepNT) void k_rep_gmark(const GapAln* __restrict__ aln, const int32_t* __restrict__ perm,
                                                      int64_t n, int32_t* __restrict__ dup, int32_t* __restrict__ gstart,
                                                      int64_t* __restrict__ box) {
  const int64_t i = (int64_t)blockIdx.x * kRepNT + threadIdx.x;
  if (i >= n) return;
  const GapAln x = aln[perm[i]];
  bool head = true, same = false;
  if (i > 0) {
    const GapAln p = aln[perm[i - 1]];
    head = p.sm != x.sm || p.contig != x.contig;
    same = !head && p.score2 == x.score2 && p.qstart == x.qstart && p.sstart == x.sstart && p.qspan == x.qspan &&
           p.sspan == x.sspan && p.length == x.length && p.matches == x.matches && p.gaps == x.gaps;
  }
  dup[i] = same;
  gstart[i] = head ? (int32_t)i : 0;
  box[4 * i] = x.qstart;
  box[4 * i + 1] = (int64_t)x.qstart + x.qspan;
  box[4 * i + 2] = x.sstart;
  box[4 * i + 3] = (int64_t)x.sstart + x.sspan;
}

struct MaxOp {
  __host__ __device__ __forceinline__ int32_t operator()(int32_t a, int32_t b) const { return a > b ? a : b; }
};

__global__ __launch_bounds__(kRepNT) void k_rep_gcover(const GapAln* __restrict__ aln, const int32_t* __restrict__ perm,
                                                       const int32_t* __restrict__ dup, const int32_t* __restrict__ gfirst,
                                                       const int64_t* __restrict__ box, int64_t n, int64_t min_score2,
                                                       uint64_t* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * kRepNT + threadIdx.x;
  if (i >= n) return;
  if (dup[i]) {
    val[i] = 0;
    return;
  }
  const int64_t q0 = box[4 * i], q1 = box[4 * i + 1], s0 = box[4 * i + 2], s1 = box[4 * i + 3];
  bool covered = false;
  // gfirst[i] <= i: the running maximum of positions that are heads at or before i
  for (int64_t k = gfirst[i]; k < i && !covered; ++k)
    covered = box[4 * k] <= q0 && q1 <= box[4 * k + 1] && box[4 * k + 2] <= s0 && s1 <= box[4 * k + 3];
  const bool keep = !covered && aln[perm[i]].score2 >= min_score2;
  val[i] = kHeadBit | (keep ? 1ull : 0ull);      // bit 32: a distinct alignment
}

__global__ __launch_bounds__(kRepNT) void k_rep_gemit(const GapAln* __restrict__ aln, const int32_t* __restrict__ perm,
                                                      const uint64_t* __restrict__ val, const uint64_t* __restrict__ sum,
                                                      int64_t n, int64_t n_kept, RepKey K, GapAln* __restrict__ kept,
                                                      uint64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * kRepNT + threadIdx.x;
  if (i >= n || !(val[i] & 1ull)) return;
  const int64_t k = (uint32_t)sum[i];            // kept before i: below 2^31, no carry into bit 32
  if (k >= n_kept) return;
  const GapAln a = aln[perm[i]];
  kept[k] = a;
  const int64_t x[9] = {a.contig, a.sm, a.qstart, a.sstart, a.qspan, a.sspan, a.length, a.matches, a.gaps};
  rep_key_store(K, x, keys, n_kept, k);
}

struct Scratch {                   // the most any hipcub call below asks for
  size_t bytes = 0;
  void take(size_t t) { bytes = std::max(bytes, t); }
};

// the order of K's keys (st->keys, n records) in *perm (R->perm or R->spare)
int rep_sort(ReportState* R, const RepKey& K, int64_t n, int32_t** perm, hipStream_t s, std::string* err) {
  *perm = R->perm.p;
  int32_t* spare = R->spare.p;
  MAP_RC(key_iota(*perm, n, s, err));
  return key_sort(R->keys.p, K.words, K.total_bits, (int)n, R->kin.p, R->kout.p, perm, &spare, R->tmp.p, R->tmp.n, s, err);
}

// what both forms share: room for n elements of the sorts and scans
int rep_reserve(ReportState* R, const RepKey& K1, const RepKey& K2, int64_t n, hipStream_t s, std::string* err) {
  const size_t un = (size_t)n;
  const int ni = (int)n;
  Scratch sc;
  size_t t = 0;
  MAP_RC(key_sort_scratch(K1.words, K1.total_bits, ni, &t, s, err));
  sc.take(t);
  MAP_RC(key_sort_scratch(K2.words, K2.total_bits, ni, &t, s, err));
  sc.take(t);
  t = 0;
  MAP_TRY(hipcub::DeviceScan::InclusiveScan(nullptr, t, (const uint64_t*)nullptr, (uint64_t*)nullptr, SegMaxOp(), ni, s));
  sc.take(t);
  t = 0;
  MAP_TRY(hipcub::DeviceScan::InclusiveScan(nullptr, t, (const int32_t*)nullptr, (int32_t*)nullptr, MaxOp(), ni, s));
  sc.take(t);
  t = 0;
  MAP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, t, (const int32_t*)nullptr, (int32_t*)nullptr, ni, s));
  sc.take(t);
  t = 0;
  MAP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, t, (const uint64_t*)nullptr, (uint64_t*)nullptr, ni, s));
  sc.take(t);
  MAP_RC(R->keys.ensure(un * (size_t)std::max(1, std::max(K1.words, K2.words)), err));
  MAP_RC(R->kin.ensure(un, err));
  MAP_RC(R->kout.ensure(un, err));
  MAP_RC(R->val.ensure(un, err));
  MAP_RC(R->run.ensure(un, err));
  MAP_RC(R->perm.ensure(un, err));
  MAP_RC(R->spare.ensure(un, err));
  MAP_RC(R->flag.ensure(un, err));
  MAP_RC(R->first.ensure(un, err));
  MAP_RC(R->tmp.ensure(sc.bytes, err));
  return 0;
}

}  // namespace

int report_anchors(const SearchRec* rec, int64_t n, GapAnchor* anchor, hipStream_t s, std::string* err) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_rep_anchors, dim3(grid_of(n)), dim3(kRepNT), 0, s, rec, n, anchor);
  MAP_TRY(hipGetLastError());
  return 0;
}

int report_hsps_device(ReportState* R, const SearchRaw* raw, int64_t n, int min_score, const RepBounds& B,
                       int64_t* n_rec, hipStream_t s, std::string* err) {
  *n_rec = 0;
  if (n <= 0) return 0;
  static const int f1[5] = {kRepSm, kRepContig, kRepDelta, kRepB, kRepE};
  static const int f2[5] = {kRepContig, kRepSm, kRepQstartU, kRepB, kRepLengthU};
  const RepKey K1 = make_key(B, f1, 5, 1u << 4), K2 = make_key(B, f2, 5, 0);
  MAP_RC(rep_reserve(R, K1, K2, n, s, err));
  const unsigned grid = grid_of(n);
  const int ni = (int)n;
  if (K1.words > 0) hipLaunchKernelGGL(k_rep_ukeys, dim3(grid), dim3(kRepNT), 0, s, raw, n, K1, R->keys.p);
  MAP_TRY(hipGetLastError());
  int32_t* perm = nullptr;
  MAP_RC(rep_sort(R, K1, n, &perm, s, err));
  hipLaunchKernelGGL(k_rep_umark, dim3(grid), dim3(kRepNT), 0, s, raw, (const int32_t*)perm, n, R->val.p);
  MAP_TRY(hipGetLastError());
  size_t tb = R->tmp.n;
  MAP_TRY(hipcub::DeviceScan::InclusiveScan(R->tmp.p, tb, (const uint64_t*)R->val.p, R->run.p, SegMaxOp(), ni, s));
  int32_t* const keep = R->flag.p;
  int32_t* const slot = R->first.p;
  hipLaunchKernelGGL(k_rep_ukeep, dim3(grid), dim3(kRepNT), 0, s, raw, (const int32_t*)perm, (const uint64_t*)R->run.p, n,
                     min_score, keep);
  MAP_TRY(hipGetLastError());
  tb = R->tmp.n;
  MAP_TRY(hipcub::DeviceScan::ExclusiveSum(R->tmp.p, tb, (const int32_t*)keep, slot, ni, s));
  int32_t last_keep = 0, last_slot = 0;
  MAP_TRY(hipMemcpyAsync(&last_keep, keep + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MAP_TRY(hipMemcpyAsync(&last_slot, slot + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MAP_TRY(hipStreamSynchronize(s));
  const int64_t n_kept = (int64_t)last_keep + last_slot;
  if (n_kept == 0) return 0;
  MAP_RC(R->rec.ensure((size_t)n_kept, err));
  MAP_RC(R->rec_sorted.ensure((size_t)n_kept, err));
  // (the first sort's keys are done with: the second's take their place, n_kept to a word)
  hipLaunchKernelGGL(k_rep_uemit, dim3(grid), dim3(kRepNT), 0, s, raw, (const int32_t*)perm, (const int32_t*)keep,
                     (const int32_t*)slot, n, n_kept, K2, R->rec.p, R->keys.p);
  MAP_TRY(hipGetLastError());
  MAP_RC(rep_sort(R, K2, n_kept, &perm, s, err));
  hipLaunchKernelGGL(k_rep_gather<SearchRec>, dim3(grid_of(n_kept)), dim3(kRepNT), 0, s, (const SearchRec*)R->rec.p,
                     (const int32_t*)perm, n_kept, R->rec_sorted.p);
  MAP_TRY(hipGetLastError());
  MAP_TRY(hipStreamSynchronize(s));
  *n_rec = n_kept;
  return 0;
}

int report_alns_device(ReportState* R, const GapAnchor* anchor, const GapRaw* graw, int64_t n, int min_score,
                       const RepBounds& B, int64_t* n_rec, int64_t* raw_alignments, hipStream_t s, std::string* err) {
  *n_rec = 0;
  *raw_alignments = 0;
  if (n <= 0) return 0;
  static const int f1[10] = {kRepSm, kRepContig, kRepScore2, kRepQstart, kRepSstart, kRepQspan, kRepSspan, kRepLength,
                             kRepMatches, kRepGaps};
  static const int f2[9] = {kRepContig, kRepSm, kRepQstart, kRepSstart, kRepQspan, kRepSspan, kRepLength, kRepMatches,
                            kRepGaps};
  const RepKey K1 = make_key(B, f1, 10, 1u << 2), K2 = make_key(B, f2, 9, 0);
  MAP_RC(rep_reserve(R, K1, K2, n, s, err));
  MAP_RC(R->box.ensure(4 * (size_t)n, err));
  MAP_RC(R->aln.ensure((size_t)n, err));
  const unsigned grid = grid_of(n);
  const int ni = (int)n;
  hipLaunchKernelGGL(k_rep_gbuild, dim3(grid), dim3(kRepNT), 0, s, anchor, graw, n, K1, R->aln.p, R->keys.p);
  MAP_TRY(hipGetLastError());
  int32_t* perm = nullptr;
  MAP_RC(rep_sort(R, K1, n, &perm, s, err));
  int32_t* const dup = R->flag.p;
  int32_t* const gstart = (int32_t*)R->kin.p;    // the sort is over: its key buffers are free
  int32_t* const gfirst = R->first.p;
  hipLaunchKernelGGL(k_rep_gmark, dim3(grid), dim3(kRepNT), 0, s, (const GapAln*)R->aln.p, (const int32_t*)perm, n, dup,
                     gstart, R->box.p);
  MAP_TRY(hipGetLastError());
  size_t tb = R->tmp.n;
  MAP_TRY(hipcub::DeviceScan::InclusiveScan(R->tmp.p, tb, (const int32_t*)gstart, gfirst, MaxOp(), ni, s));
  hipLaunchKernelGGL(k_rep_gcover, dim3(grid), dim3(kRepNT), 0, s, (const GapAln*)R->aln.p, (const int32_t*)perm,
                     (const int32_t*)dup, (const int32_t*)gfirst, (const int64_t*)R->box.p, n, 2 * (int64_t)min_score,
                     R->val.p);
  MAP_TRY(hipGetLastError());
  tb = R->tmp.n;
  MAP_TRY(hipcub::DeviceScan::ExclusiveSum(R->tmp.p, tb, (const uint64_t*)R->val.p, R->run.p, ni, s));
  uint64_t last_val = 0, last_sum = 0;
  MAP_TRY(hipMemcpyAsync(&last_val, R->val.p + (n - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  MAP_TRY(hipMemcpyAsync(&last_sum, R->run.p + (n - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  MAP_TRY(hipStreamSynchronize(s));
  const uint64_t total = last_val + last_sum;
  const int64_t n_kept = (int64_t)(uint32_t)total;
  *raw_alignments = (int64_t)(total >> 32);
  if (n_kept == 0) return 0;
  MAP_RC(R->aln_kept.ensure((size_t)n_kept, err));
  MAP_RC(R->aln_sorted.ensure((size_t)n_kept, err));
  hipLaunchKernelGGL(k_rep_gemit, dim3(grid), dim3(kRepNT), 0, s, (const GapAln*)R->aln.p, (const int32_t*)perm,
                     (const uint64_t*)R->val.p, (const uint64_t*)R->run.p, n, n_kept, K2, R->aln_kept.p, R->keys.p);
  MAP_TRY(hipGetLastError());
  MAP_RC(rep_sort(R, K2, n_kept, &perm, s, err));
  hipLaunchKernelGGL(k_rep_gather<GapAln>, dim3(grid_of(n_kept)), dim3(kRepNT), 0, s, (const GapAln*)R->aln_kept.p,
                     (const int32_t*)perm, n_kept, R->aln_sorted.p);
  MAP_TRY(hipGetLastError());
  MAP_TRY(hipStreamSynchronize(s));
  *n_rec = n_kept;
  return 0;
}

// ---- the stand-alone entries ----------------------------------------------------------------

void search_set_report(MapState* st, int report_on) { st->search.report_on = report_on; }

int report_hsps(MapState* st, bool device, const ReportHsps& in, const RepBounds& B, const SearchOut& out, int64_t* n,
                hipStream_t s, std::string* err) {
  *n = 0;
  std::vector<SearchRaw> raw((size_t)in.n);
  for (size_t i = 0; i < raw.size(); ++i)
    raw[i] = SearchRaw{in.subject[i] << 1 | in.minus[i], in.contig[i], in.delta[i], in.b[i], in.e[i], in.score[i]};
  std::vector<SearchRec> recs;
  if (!device) {
    report_hsps_host(&raw, in.min_score, &recs);
    *n = (int64_t)recs.size();
  } else if (!raw.empty()) {
    SearchState* ss = &st->search;
    MAP_RC(synced_on_error(s, [&]() -> int {
      MAP_RC(ss->raw.ensure(raw.size(), err));
      MAP_TRY(hipMemcpyAsync(ss->raw.p, raw.data(), raw.size() * sizeof(SearchRaw), hipMemcpyHostToDevice, s));
      MAP_RC(report_hsps_device(&ss->rep, ss->raw.p, (int64_t)raw.size(), in.min_score, B, n, s, err));
      recs.resize((size_t)std::min(*n, out.capacity));
      if (!recs.empty())
        MAP_TRY(hipMemcpy(recs.data(), ss->rep.rec_sorted.p, recs.size() * sizeof(SearchRec), hipMemcpyDeviceToHost));
      return 0;
    }));
  }
  const int64_t w = std::min<int64_t>(*n, out.capacity);
  for (int64_t i = 0; i < w; ++i) {
    const SearchRec& r = recs[(size_t)i];
    out.contig[i] = r.contig;
    out.subject[i] = r.subject;
    out.minus[i] = (uint8_t)r.minus;
    out.qstart[i] = r.qstart;
    out.sstart[i] = r.sstart;
    out.length[i] = r.length;
    out.matches[i] = r.matches;
  }
  return 0;
}

int report_alns(MapState* st, bool device, const ReportAnchors& in, const RepBounds& B, const SearchGapOut& out,
                int64_t* n, int64_t* raw_alignments, hipStream_t s, std::string* err) {
  *n = 0;
  *raw_alignments = 0;
  const size_t m = (size_t)in.n;
  std::vector<GapAnchor> anchors(m);
  std::vector<GapRaw> raw(m);
  for (size_t i = 0; i < m; ++i) {
    anchors[i] = GapAnchor{in.subject[i] << 1 | in.minus[i], in.contig[i], in.i0[i], in.j0[i]};
    raw[i].left = GapSide{in.side[0][i], in.side[1][i], in.side[2][i], in.side[3][i]};
    raw[i].right = GapSide{in.side[4][i], in.side[5][i], in.side[6][i], in.side[7][i]};
  }
  std::vector<GapAln> kept;
  if (!device) {
    report_alns_host(anchors, raw, in.min_score, &kept, raw_alignments);
    *n = (int64_t)kept.size();
  } else if (m > 0) {
    SearchState* ss = &st->search;
    MAP_RC(synced_on_error(s, [&]() -> int {
      MAP_RC(ss->g_anchor.ensure(m, err));
      MAP_RC(ss->g_out.ensure(m, err));
      MAP_TRY(hipMemcpyAsync(ss->g_anchor.p, anchors.data(), m * sizeof(GapAnchor), hipMemcpyHostToDevice, s));
      MAP_TRY(hipMemcpyAsync(ss->g_out.p, raw.data(), m * sizeof(GapRaw), hipMemcpyHostToDevice, s));
      MAP_RC(report_alns_device(&ss->rep, ss->g_anchor.p, ss->g_out.p, (int64_t)m, in.min_score, B, n, raw_alignments, s,
                                err));
      kept.resize((size_t)std::min(*n, out.capacity));
      if (!kept.empty())
        MAP_TRY(hipMemcpy(kept.data(), ss->rep.aln_sorted.p, kept.size() * sizeof(GapAln), hipMemcpyDeviceToHost));
      return 0;
    }));
  }
  const int64_t w = std::min<int64_t>(*n, out.capacity);
  for (int64_t i = 0; i < w; ++i) {
    const GapAln& r = kept[(size_t)i];
    out.contig[i] = r.contig;
    out.subject[i] = r.sm >> 1;
    out.minus[i] = (uint8_t)(r.sm & 1);
    out.qstart[i] = r.qstart;
    out.qspan[i] = r.qspan;
    out.sstart[i] = r.sstart;
    out.sspan[i] = r.sspan;
    out.length[i] = r.length;
    out.matches[i] = r.matches;
    out.gaps[i] = r.gaps;
  }
  return 0;
}

}  // namespace wf
