// Search records -> the scorer's hit arrays on the GPU (gfx950 / MI355X), DESIGN.md §13: what
// the text round trip (search.format_rows, then inputs.derive_hit_values on the parsed table)
// gives, bit for bit, without the table.
//
//   k_hits     one thread per record: the record's columns are read coalesced, the four small
//              tables (contig length; subject length, taxon, systems) are gathered.  Every index
//              and every divisor was checked on the host (wf_hits_from_records) before the launch.
//   k_hit_off  one thread per contig boundary c in [0, n_contigs]: the number of records with
//              contig < c, a lower bound on the sorted contig column.
//
// pident is the double a reader gets from the text "%.3f" % (100.0 * matches / length): the
// integer nearest to the exact product of the double x = 100 matches / length and 1000, ties to
// even, over 1000.  The product's rounding error comes from one written-out fma; the library is
// built with -ffp-contract=off, so nothing else is fused.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wf_internal.h"

namespace wf {

namespace {

constexpr int kHitsNT = 256;

__device__ inline double pident_of(int32_t matches, int32_t length) {
  const double x = (100.0 * (double)matches) / (double)length;
  const double p = x * 1000.0;
  const double f = floor(p);
  const double d = p - f;                          // exact
  bool up;
  if (d > 0.5) {
    up = true;
  } else if (d < 0.5) {
    up = false;
  } else {
    const double e = fma(x, 1000.0, -p);           // the product's exact error
    if (e > 0.0) up = true;
    else if (e < 0.0) up = false;
    else up = ((int64_t)f & 1) != 0;               // the even one of f and f + 1
  }
  return (up ? f + 1.0 : f) / 1000.0;
}

__global__ __launch_bounds__(kHitsNT) void k_hits(HitsArgs A) {
  const int64_t i = (int64_t)blockIdx.x * kHitsNT + threadIdx.x;
  if (i >= A.n) return;
  const int32_t g = A.subject[i];
  const int64_t qlen = A.qlen[A.contig[i]], slen = A.slen[g];
  const int64_t q1 = (int64_t)A.qstart[i] + 1, qhi = (int64_t)A.qstart[i] + A.qspan[i];
  const int64_t s0 = (int64_t)A.sstart[i] + 1, s1 = (int64_t)A.sstart[i] + A.sspan[i];
  const int64_t lt = s0 - q1, rt = slen - s0 - qlen + q1;
  const int64_t ltrim = lt > 0 ? lt : 0, rtrim = rt > 0 ? rt : 0;
  const int64_t denom = slen - ltrim - rtrim;
  const double scov = (double)(s1 - s0 + 1) / (double)denom;
  const double pident = pident_of(A.matches[i], A.length[i]);
  const int32_t taxon = A.subject_taxon[g];
  const uint32_t sysmask = A.subject_sysmask[g];
  const bool minus = A.minus[i] != 0;
  A.hit_qlo[i] = (int32_t)q1;
  A.hit_qhi[i] = (int32_t)qhi;
  A.hit_taxon[i] = taxon;
  A.hit_strand[i] = minus ? 1 : 0;
  A.hit_score[i] = scov * pident / 100.0;          // two roundings, in this order
  A.hit_scov[i] = scov;
  A.hit_sysmask[i] = sysmask;
  A.hit_key[i] = pack_hit_key(taxon, scov >= A.min_scov, minus, sysmask);
}

__global__ __launch_bounds__(kHitsNT) void k_hit_off(HitsArgs A) {
  const int64_t c = (int64_t)blockIdx.x * kHitsNT + threadIdx.x;
  if (c > A.n_contigs) return;
  int64_t lo = 0, hi = A.n;                        // first record with contig >= c
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (A.contig[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  A.hit_off[c] = lo;
}

}  // namespace

hipError_t launch_hits(const HitsArgs& a, hipStream_t s) {
  if (a.n > 0)
    hipLaunchKernelGGL(k_hits, dim3((unsigned)((a.n + kHitsNT - 1) / kHitsNT)), dim3(kHitsNT), 0, s, a);
  hipLaunchKernelGGL(k_hit_off, dim3((unsigned)(((int64_t)a.n_contigs + 1 + kHitsNT - 1) / kHitsNT)), dim3(kHitsNT), 0,
                     s, a);
  return hipGetLastError();
}

}  // namespace wf
