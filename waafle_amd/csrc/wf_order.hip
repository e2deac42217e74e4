// The table's order and --max-target-seqs on the GPU (gfx950 / MI355X), DESIGN.md §13.6: what
// search.order_records computes on the host, index for index.
//
// One composite key per record, most significant field first:
//   contig, max_score - score, subject, minus, qstart, sstart [, qspan, sspan]
// Each field is stored as (value - its least value) in exactly the bits the caller's pass over
// the input proved sufficient (OrderPlan), so the key is as narrow as this call's records allow
// (typically under 128 bits) and never narrower than they need: at most 4 words of 64 bits.
//
//   k_order_keys  one thread per record: the 64-bit score, the key words, word-major
//   k_order_pick  one thread per position: the key word of the record the permutation has there
//   the sort      least significant word first, one stable hipcub radix sort of (word, index)
//                 pairs per word over the word's used bits only; it starts from the identity, so
//                 records equal in every field stay in input order
//   the limit     (only when some contig can hold more than max_target_seqs subjects.)  In the
//                 sorted order the first record of each (contig, subject) pair is its best one,
//                 and within a contig those first records come in the pairs' rank order
//                 (-best, subject).  So a pair's rank is the number of pair heads before its own
//                 head in its contig.  One more stable sort of the positions by (contig, subject)
//                 groups the pairs; the first of each group is the head.
//     k_order_pairkey  the (contig, subject) word of the record at each sorted position, and
//                      the position of each contig's first record
//     k_order_heads    per group-sorted slot: the group's first slot; marks the head positions
//     k_order_keep     per group-sorted slot: rank of its group's head -> keep flag of its position
//                 with two running maxima (group start, contig start) and two sums (heads
//                 before a position, kept before a position) from hipcub::DeviceScan
//   k_order_emit  order[slot] = index, for the kept positions
//   k_order_gather  the nine wf_hit_records columns in that order (those asked for)
//
// Every kernel is one thread per element with its bound checked before any load; the indices it
// follows are permutations of [0, n) made by the sorts and scans above.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "wf_keys.h"
#include "wf_mapstore.h"

namespace wf {

struct OrderState {
  DevArr<int32_t> col;            // the int32 input columns, n each: see kCol*
  DevArr<uint8_t> minus;
  DevArr<uint64_t> keys;          // [words][n]
  DevArr<uint64_t> kin, kout;     // one sort's keys
  DevArr<int32_t> work;           // kWork arrays of n
  DevArr<int64_t> order;
  DevArr<int32_t> out_col;        // the gathered int32 columns, n each
  DevArr<uint8_t> out_minus;
  DevArr<unsigned char> tmp;      // hipcub's scratch
};

OrderState* order_create() { return new OrderState(); }
void order_destroy(OrderState* st) { delete st; }

namespace {

constexpr int kOrderNT = 256;
constexpr int kWork = 11;         // int32 work arrays
enum { kColContig, kColSubject, kColQstart, kColSstart, kColLength, kColMatches, kColQspan, kColSspan, kColGaps, kCols };

struct OrderCols {                // device pointers; qspan, sspan, gaps null: ungapped records
  const int32_t* contig; const int32_t* subject; const uint8_t* minus; const int32_t* qstart; const int32_t* sstart;
  const int32_t* length; const int32_t* matches; const int32_t* qspan; const int32_t* sspan; const int32_t* gaps;
};

inline unsigned grid_of(int64_t n) { return (unsigned)((n + kOrderNT - 1) / kOrderNT); }

__device__ __forceinline__ int64_t order_score(const OrderCols& C, int64_t i) {
  const int64_t m = C.matches[i], len = C.length[i];
  return C.gaps ? 6 * m - 4 * len - (int64_t)C.gaps[i] : 3 * m - 2 * len;
}

__global__ __launch_bounds__(kOrderNT) void k_order_keys(OrderCols C, OrderPlan P, int64_t n, int words,
                                                         uint64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * kOrderNT + threadIdx.x;
  if (i >= n) return;
  int64_t v[kOrderFields];
  v[0] = (int64_t)C.contig[i] - P.base[0];
  v[1] = P.base[1] - order_score(C, i);                    // base[1]: the greatest score
  v[2] = (int64_t)C.subject[i] - P.base[2];
  v[3] = (int64_t)C.minus[i] - P.base[3];
  v[4] = (int64_t)C.qstart[i] - P.base[4];
  v[5] = (int64_t)C.sstart[i] - P.base[5];
  v[6] = C.qspan ? (int64_t)C.qspan[i] - P.base[6] : 0;
  v[7] = C.sspan ? (int64_t)C.sspan[i] - P.base[7] : 0;
  uint64_t w[4] = {0, 0, 0, 0};
  int off = 0;
#pragma unroll
  for (int f = kOrderFields - 1; f >= 0; --f) {            // the last field is the least significant
    key_put(w, (uint64_t)v[f], off, P.bits[f]);
    off += P.bits[f];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < words) keys[(int64_t)k * n + i] = w[k];
}

__global__ __launch_bounds__(kOrderNT) void k_order_iota(int32_t* __restrict__ a, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kOrderNT + threadIdx.x;
  if (i < n) a[i] = (int32_t)i;
}

__global__ __launch_bounds__(kOrderNT) void k_order_pick(const uint64_t* __restrict__ word, const int32_t* __restrict__ perm,
                                                         int64_t n, uint64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kOrderNT + threadIdx.x;
  if (i < n) out[i] = word[perm[i]];
}

// position i of the sorted order: the (contig, subject) word of its record, and i where a contig begins (else 0)
__global__ __launch_bounds__(kOrderNT) void k_order_pairkey(OrderCols C, OrderPlan P, const int32_t* __restrict__ perm,
                                                            int64_t n, uint64_t* __restrict__ pk,
                                                            int32_t* __restrict__ cstart) {
  const int64_t i = (int64_t)blockIdx.x * kOrderNT + threadIdx.x;
  if (i >= n) return;
  const int32_t r = perm[i];
  const int32_t c = C.contig[r];
  pk[i] = ((uint64_t)((int64_t)c - P.base[0]) << P.bits[2]) | (uint64_t)((int64_t)C.subject[r] - P.base[2]);
  cstart[i] = (i > 0 && C.contig[perm[i - 1]] != c) ? (int32_t)i : 0;
}

// slot j of the positions grouped by pair: j where a group begins (else 0); head[position] = begins
__global__ __launch_bounds__(kOrderNT) void k_order_heads(const uint64_t* __restrict__ pk_sorted,
                                                          const int32_t* __restrict__ pos, int64_t n,
                                                          int32_t* __restrict__ gstart, int32_t* __restrict__ head) {
  const int64_t j = (int64_t)blockIdx.x * kOrderNT + threadIdx.x;
  if (j >= n) return;
  const bool begins = j == 0 || pk_sorted[j] != pk_sorted[j - 1];
  gstart[j] = begins ? (int32_t)j : 0;
  head[pos[j]] = begins ? 1 : 0;
}

// slot j: its group's head position h; the pair's rank is the heads in [contig start, h)
__global__ __launch_bounds__(kOrderNT) void k_order_keep(const int32_t* __restrict__ pos, const int32_t* __restrict__ gfirst,
                                                         const int32_t* __restrict__ heads_before,
                                                         const int32_t* __restrict__ cfirst, int64_t limit, int64_t n,
                                                         int32_t* __restrict__ keep) {
  const int64_t j = (int64_t)blockIdx.x * kOrderNT + threadIdx.x;
  if (j >= n) return;
  const int32_t h = pos[gfirst[j]];
  const int64_t rank = (int64_t)heads_before[h] - (int64_t)heads_before[cfirst[h]];
  keep[pos[j]] = rank < limit ? 1 : 0;
}

// keep null: every position is kept
__global__ __launch_bounds__(kOrderNT) void k_order_emit(const int32_t* __restrict__ perm, const int32_t* __restrict__ keep,
                                                         const int32_t* __restrict__ slot, int64_t n,
                                                         int64_t* __restrict__ order) {
  const int64_t i = (int64_t)blockIdx.x * kOrderNT + threadIdx.x;
  if (i >= n) return;
  if (!keep) order[i] = perm[i];
  else if (keep[i]) order[slot[i]] = perm[i];
}

struct OrderGather {              // device pointers, null: not wanted
  int32_t* contig; int32_t* subject; uint8_t* minus; int32_t* qstart; int32_t* qspan; int32_t* sstart; int32_t* sspan;
  int32_t* length; int32_t* matches;
};

__global__ __launch_bounds__(kOrderNT) void k_order_gather(OrderCols C, OrderGather G, const int64_t* __restrict__ order,
                                                           int64_t n_kept) {
  const int64_t k = (int64_t)blockIdx.x * kOrderNT + threadIdx.x;
  if (k >= n_kept) return;
  const int64_t i = order[k];
  const int32_t len = C.length[i];
  if (G.contig) G.contig[k] = C.contig[i];
  if (G.subject) G.subject[k] = C.subject[i];
  if (G.minus) G.minus[k] = C.minus[i];
  if (G.qstart) G.qstart[k] = C.qstart[i];
  if (G.qspan) G.qspan[k] = C.qspan ? C.qspan[i] : len;
  if (G.sstart) G.sstart[k] = C.sstart[i];
  if (G.sspan) G.sspan[k] = C.sspan ? C.sspan[i] : len;
  if (G.length) G.length[k] = len;
  if (G.matches) G.matches[k] = C.matches[i];
}

struct MaxOp {
  __host__ __device__ __forceinline__ int32_t operator()(int32_t a, int32_t b) const { return a > b ? a : b; }
};

template <class T>
int to_device(T* dst, const T* src, int64_t n, hipStream_t s, std::string* err) {
  MAP_TRY(hipMemcpyAsync(dst, src, sizeof(T) * (size_t)n, hipMemcpyHostToDevice, s));
  return 0;
}
template <class T>
int to_host(T* dst, const T* src, int64_t n, hipStream_t s, std::string* err) {
  if (dst && n > 0) MAP_TRY(hipMemcpyAsync(dst, src, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, s));
  return 0;
}

}  // namespace

int key_iota(int32_t* a, int64_t n, hipStream_t s, std::string* err) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_order_iota, dim3(grid_of(n)), dim3(kOrderNT), 0, s, a, n);
  MAP_TRY(hipGetLastError());
  return 0;
}

int key_sort_scratch(int words, int total_bits, int n, size_t* bytes, hipStream_t s, std::string* err) {
  *bytes = 0;
  for (int w = 0; w < words; ++w) {
    size_t t = 0;
    MAP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, t, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                               (const int32_t*)nullptr, (int32_t*)nullptr, n, 0,
                                               std::min(64, total_bits - 64 * w), s));
    *bytes = std::max(*bytes, t);
  }
  return 0;
}

int key_sort(const uint64_t* keys, int words, int total_bits, int n, uint64_t* kin_buf, uint64_t* kout, int32_t** perm,
             int32_t** spare, void* tmp, size_t tmp_bytes, hipStream_t s, std::string* err) {
  for (int w = 0; w < words; ++w) {
    const uint64_t* word = keys + (size_t)w * (size_t)n;
    const uint64_t* kin = word;                              // the first permutation is the identity
    if (w > 0) {
      hipLaunchKernelGGL(k_order_pick, dim3(grid_of(n)), dim3(kOrderNT), 0, s, word, (const int32_t*)*perm, (int64_t)n,
                         kin_buf);
      MAP_TRY(hipGetLastError());
      kin = kin_buf;
    }
    size_t tb = tmp_bytes;
    MAP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, tb, kin, kout, (const int32_t*)*perm, *spare, n, 0,
                                               std::min(64, total_bits - 64 * w), s));
    std::swap(*perm, *spare);
  }
  return 0;
}

int order_run(OrderState* st, const OrderIn& in, const OrderPlan& plan, const OrderOut& out, hipStream_t s,
              std::string* err) {
  const int64_t n = in.n;                                   // 0 < n < 2^31, checked by the caller
  const int ni = (int)n;
  const bool gapped = in.qspan != nullptr;
  int total_bits = 0;
  for (int f = 0; f < kOrderFields; ++f) total_bits += plan.bits[f];
  const int words = (total_bits + 63) / 64;
  const bool want = out.contig || out.subject || out.minus || out.qstart || out.qspan || out.sstart || out.sspan ||
                    out.length || out.matches;

  // every allocation before any copy or launch: a refusal for memory leaves nothing written
  size_t t_sort = 0, t_sum = 0, t_max = 0;
  const int pair_bits = plan.bits[0] + plan.bits[2];
  for (int w = 0; w <= words; ++w) {                         // the words' sorts, then the pairs'
    const int end_bit = w < words ? std::min(64, total_bits - 64 * w) : pair_bits;
    size_t t = 0;
    if (end_bit > 0)
      MAP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, t, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                 (const int32_t*)nullptr, (int32_t*)nullptr, ni, 0, end_bit, s));
    t_sort = std::max(t_sort, t);
  }
  MAP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, t_sum, (const int32_t*)nullptr, (int32_t*)nullptr, ni, s));
  MAP_TRY(hipcub::DeviceScan::InclusiveScan(nullptr, t_max, (const int32_t*)nullptr, (int32_t*)nullptr, MaxOp(), ni, s));
  std::string why;
  const size_t un = (size_t)n;
  if (st->col.ensure(un * (gapped ? kCols : kColQspan), &why) || st->minus.ensure(un, &why) ||
      st->keys.ensure(un * (size_t)std::max(words, 1), &why) || st->kin.ensure(un, &why) || st->kout.ensure(un, &why) ||
      st->work.ensure(un * kWork, &why) || st->order.ensure(un, &why) ||
      (want && (st->out_col.ensure(un * 8, &why) || st->out_minus.ensure(un, &why))) ||
      st->tmp.ensure(std::max(t_sort, std::max(t_sum, t_max)), &why)) {
    *err = "no device memory to order " + std::to_string(n) + " records: " + why;
    return -4;
  }

  int32_t* const col = st->col.p;
  auto column = [&](int k) { return col + (size_t)k * un; };
  MAP_RC(to_device(column(kColContig), in.contig, n, s, err));
  MAP_RC(to_device(column(kColSubject), in.subject, n, s, err));
  MAP_RC(to_device(column(kColQstart), in.qstart, n, s, err));
  MAP_RC(to_device(column(kColSstart), in.sstart, n, s, err));
  MAP_RC(to_device(column(kColLength), in.length, n, s, err));
  MAP_RC(to_device(column(kColMatches), in.matches, n, s, err));
  MAP_RC(to_device(st->minus.p, in.minus, n, s, err));
  if (gapped) {
    MAP_RC(to_device(column(kColQspan), in.qspan, n, s, err));
    MAP_RC(to_device(column(kColSspan), in.sspan, n, s, err));
    MAP_RC(to_device(column(kColGaps), in.gaps, n, s, err));
  }
  const OrderCols C{column(kColContig), column(kColSubject), st->minus.p, column(kColQstart), column(kColSstart),
                    column(kColLength), column(kColMatches), gapped ? column(kColQspan) : nullptr,
                    gapped ? column(kColSspan) : nullptr, gapped ? column(kColGaps) : nullptr};

  int32_t* const work = st->work.p;
  auto arr = [&](int k) { return work + (size_t)k * un; };
  const unsigned grid = grid_of(n);
  size_t tb = st->tmp.n;

  // the sort: least significant word first
  int32_t* perm = arr(0);
  int32_t* spare = arr(1);
  MAP_RC(key_iota(perm, n, s, err));
  if (words > 0) hipLaunchKernelGGL(k_order_keys, dim3(grid), dim3(kOrderNT), 0, s, C, plan, n, words, st->keys.p);
  MAP_TRY(hipGetLastError());
  MAP_RC(key_sort(st->keys.p, words, total_bits, ni, st->kin.p, st->kout.p, &perm, &spare, st->tmp.p, st->tmp.n, s, err));

  // the limit
  int64_t n_kept = n;
  const int32_t* keep = nullptr;
  const int32_t* slot = nullptr;
  if (plan.rank) {
    int32_t* const iota = spare;                             // arr(0) or arr(1), whichever perm is not
    int32_t* const pos = arr(2);
    int32_t* const cstart = arr(3);
    int32_t* const cfirst = arr(4);
    int32_t* const gstart = arr(5);
    int32_t* const gfirst = arr(6);
    int32_t* const head = arr(7);
    int32_t* const heads_before = arr(8);
    int32_t* const keep_w = arr(9);
    int32_t* const slot_w = arr(10);
    hipLaunchKernelGGL(k_order_iota, dim3(grid), dim3(kOrderNT), 0, s, iota, n);
    hipLaunchKernelGGL(k_order_pairkey, dim3(grid), dim3(kOrderNT), 0, s, C, plan, (const int32_t*)perm, n, st->kin.p,
                       cstart);
    MAP_TRY(hipGetLastError());
    if (pair_bits > 0) {
      tb = st->tmp.n;
      MAP_TRY(hipcub::DeviceRadixSort::SortPairs(st->tmp.p, tb, (const uint64_t*)st->kin.p, st->kout.p,
                                                 (const int32_t*)iota, pos, ni, 0, pair_bits, s));
    } else {                                                 // one pair holds every record
      MAP_TRY(hipMemcpyAsync(st->kout.p, st->kin.p, sizeof(uint64_t) * un, hipMemcpyDeviceToDevice, s));
      MAP_TRY(hipMemcpyAsync(pos, iota, sizeof(int32_t) * un, hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(k_order_heads, dim3(grid), dim3(kOrderNT), 0, s, (const uint64_t*)st->kout.p,
                       (const int32_t*)pos, n, gstart, head);
    MAP_TRY(hipGetLastError());
    tb = st->tmp.n;
    MAP_TRY(hipcub::DeviceScan::InclusiveScan(st->tmp.p, tb, (const int32_t*)gstart, gfirst, MaxOp(), ni, s));
    tb = st->tmp.n;
    MAP_TRY(hipcub::DeviceScan::InclusiveScan(st->tmp.p, tb, (const int32_t*)cstart, cfirst, MaxOp(), ni, s));
    tb = st->tmp.n;
    MAP_TRY(hipcub::DeviceScan::ExclusiveSum(st->tmp.p, tb, (const int32_t*)head, heads_before, ni, s));
    hipLaunchKernelGGL(k_order_keep, dim3(grid), dim3(kOrderNT), 0, s, (const int32_t*)pos, (const int32_t*)gfirst,
                       (const int32_t*)heads_before, (const int32_t*)cfirst, plan.limit, n, keep_w);
    MAP_TRY(hipGetLastError());
    tb = st->tmp.n;
    MAP_TRY(hipcub::DeviceScan::ExclusiveSum(st->tmp.p, tb, (const int32_t*)keep_w, slot_w, ni, s));
    int32_t last_keep = 0, last_slot = 0;
    MAP_TRY(hipMemcpyAsync(&last_keep, keep_w + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MAP_TRY(hipMemcpyAsync(&last_slot, slot_w + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MAP_TRY(hipStreamSynchronize(s));
    n_kept = (int64_t)last_keep + last_slot;
    keep = keep_w;
    slot = slot_w;
  }
  hipLaunchKernelGGL(k_order_emit, dim3(grid), dim3(kOrderNT), 0, s, (const int32_t*)perm, keep, slot, n, st->order.p);
  MAP_TRY(hipGetLastError());

  int32_t* const oc = st->out_col.p;
  auto ocol = [&](int k, const void* wanted) { return wanted ? oc + (size_t)k * un : nullptr; };
  const OrderGather G{ocol(0, out.contig), ocol(1, out.subject), out.minus ? st->out_minus.p : nullptr,
                      ocol(2, out.qstart), ocol(3, out.qspan), ocol(4, out.sstart), ocol(5, out.sspan),
                      ocol(6, out.length), ocol(7, out.matches)};
  if (want && n_kept > 0) {
    hipLaunchKernelGGL(k_order_gather, dim3(grid_of(n_kept)), dim3(kOrderNT), 0, s, C, G, (const int64_t*)st->order.p,
                       n_kept);
    MAP_TRY(hipGetLastError());
  }
  MAP_RC(to_host(out.order, (const int64_t*)st->order.p, n_kept, s, err));
  MAP_RC(to_host(out.contig, (const int32_t*)G.contig, n_kept, s, err));
  MAP_RC(to_host(out.subject, (const int32_t*)G.subject, n_kept, s, err));
  MAP_RC(to_host(out.minus, (const uint8_t*)G.minus, n_kept, s, err));
  MAP_RC(to_host(out.qstart, (const int32_t*)G.qstart, n_kept, s, err));
  MAP_RC(to_host(out.qspan, (const int32_t*)G.qspan, n_kept, s, err));
  MAP_RC(to_host(out.sstart, (const int32_t*)G.sstart, n_kept, s, err));
  MAP_RC(to_host(out.sspan, (const int32_t*)G.sspan, n_kept, s, err));
  MAP_RC(to_host(out.length, (const int32_t*)G.length, n_kept, s, err));
  MAP_RC(to_host(out.matches, (const int32_t*)G.matches, n_kept, s, err));
  MAP_TRY(hipStreamSynchronize(s));
  *out.n_kept = n_kept;
  return 0;
}

}  // namespace wf
