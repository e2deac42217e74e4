// Gapped extension of the homology search on MI355X (gfx950): every ungapped record of a chunk
// (wf_search.hip) is an anchor, extended to either side by a banded x-drop
// alignment with linear gap cost.  DESIGN.md §12.5 states the rule; tests/search_gap_oracle.py
// restates it on the CPU twice.  Scores in half units: match +2, mismatch -4, gap column -5.
//
// k_search_gapped: one wavefront per anchor, first the right side, then the left.
//   lane l <-> band diagonal d = q - p = l - W (2 W + 1 <= 63 lanes), one anti-diagonal
//   k = p + q per step; the lanes with k - d even hold a cell (p, q) = ((k - d) / 2, (k + d) / 2).
//   Every lane keeps one (H, g): its cell of step k - 2 when it is active at step k (the
//   diagonal predecessor), and for its neighbours their cells of step k - 1 (the two gap
//   predecessors, fetched with __shfl_down / __shfl_up).  best(k) is a wave-wide max of the
//   step before (wf_lanes.h butterfly, DPP and permlane swaps, no LDS).
//   Bases: per tile of 64 steps a lane takes 32 consecutive columns of its own diagonal, so it
//   loads one 32-column mismatch word from the bit planes (chunk_mis, wf_mapstore.h: the chunk's
//   planes of the anchor's strand, the index's store) and shifts a bit out of it per active step.  The left side
//   reads the words below the anchor, bit-reversed.
//   Loads: a lane loads a word only when one of its 32 columns lies inside the subject and
//   inside the contig, so the word starts at most 31 positions before such a column: its first
//   store word is W >= -1 (guarded, reads as N) and its second lies inside the padding.
// Host (search_gapped_run): the ungapped records are uploaded as anchors, extended in launches
// of at most kGapLaunch with a synchronisation each, and the reporting step of §12.5 runs in
// C++ (report_alns_host, wf_report.hip): identical alignments once, then per (subject, strand,
// contig) in score order, those covered by a kept one dropped.  With the reporting step on the
// device (SearchState::report_on) the anchors are made from the device's
// records, the launches follow one another with nothing between them (gapped_launches), and
// only the final records come back.
#include <algorithm>
#include <climits>
#include <string>
#include <tuple>
#include <vector>

#include "wf_internal.h"
#include "wf_lanes.h"
#include "wf_mapstore.h"

namespace wf {
namespace {

constexpr int kGapLaunch = 1 << 16;             // anchors per k_search_gapped launch
constexpr int kGapDead = INT_MIN / 2;

struct GapArgs {
  MapIndexView ix;            // the contigs
  ChunkView ch;               // the chunk
  int W, X2;                  // band half-width; 2 Xg (half units)
  const GapAnchor* anchor;    // [n]
  int n;
  GapRaw* out;                // [n]
};

__device__ __forceinline__ int wave_max(int x) {
  return wave_butterfly(x, [](int a, int b) { return a > b ? a : b; });
}
__device__ __forceinline__ int wave_min(int x) {
  return wave_butterfly(x, [](int a, int b) { return a < b ? a : b; });
}

// One side of one anchor, by the whole wave (every lane runs every step; the loop's trip
// count is wave-uniform).  u: nu bases of the variant, v: nv bases of the contig, walked away
// from the anchor; vpos, gpos: the store positions of u[0] and v[0].
template <bool kLeft>
__device__ __forceinline__ GapSide gap_side(const GapArgs& A, int strand, int vpos, int gpos, int nu, int nv,
                                            int lane) {
  const int W = A.W, d = lane - W;
  const bool inband = lane <= 2 * W;
  // the columns t (u[t] against v[t + d]) a diagonal move of this lane may read
  const int tlo = max(0, -d), thi = min(nu, nv - d);
  int H = lane == W ? 0 : kGapDead, g = 0;       // the lane's latest cell
  int topH = H, topK = 0, topG = 0;              // the lane's best live cell, the first of equal ones
  int best = 0;                                  // over the anti-diagonals before k
  bool prev_live = true;
  uint32_t mis = ~0u;
  int t0 = 0;                                    // the column of bit 0 of mis
  // the last anti-diagonal with a cell in the band; nu < 2^30 (an anchor lies inside its HSP)
  const int kmax = (int)min((int64_t)nu + nv, 2 * (int64_t)min(nu, nv) + W);
  for (int k = 1; k <= kmax; ++k) {
    if (k == 1 || (k & 63) == 0) {               // a tile of steps [k0, k0 + 64), k0 = k & ~63
      const int k0 = k & ~63;
      const int kf = k0 + (d & 1);               // the lane's first active step of the tile
      t0 = ((kf - d) >> 1) - 1;
      mis = ~0u;
      if (inband && max(t0, tlo) < min(t0 + 32, thi)) {
        if (kLeft) mis = __brev(chunk_mis(A.ix, A.ch, strand, vpos - t0 - 31, gpos - d - t0 - 31));
        else mis = chunk_mis(A.ix, A.ch, strand, vpos + t0, gpos + d + t0);
      }
    }
    const bool active = inband && ((k - d) & 1) == 0;
    const int p = (k - d) >> 1, q = k - p;
    int Hu = __shfl_down(H, 1), gu = __shfl_down(g, 1);    // (p - 1, q): diagonal d + 1
    int Hl = __shfl_up(H, 1), gl = __shfl_up(g, 1);        // (p, q - 1): diagonal d - 1
    if (lane == 63) Hu = kGapDead;
    if (lane == 0) Hl = kGapDead;
    int nh = kGapDead, ng = 0;
    if (H > kGapDead) {                          // (p - 1, q - 1): column p - 1
      nh = H + (((mis >> ((p - 1 - t0) & 31)) & 1u) ? -4 : 2);
      ng = g;
    }
    if (Hu > kGapDead && Hu - 5 > nh) { nh = Hu - 5; ng = gu + 1; }
    if (Hl > kGapDead && Hl - 5 > nh) { nh = Hl - 5; ng = gl + 1; }
    const bool live = active && p >= 0 && q >= 0 && p <= nu && q <= nv && nh > kGapDead && best - nh <= A.X2;
    if (active) {
      H = live ? nh : kGapDead;
      g = ng;
    }
    if (live && nh > topH) { topH = nh; topK = k; topG = ng; }
    const int m = wave_max(active ? H : kGapDead);
    if (m == kGapDead) {
      if (!prev_live) break;
      prev_live = false;
    } else {
      prev_live = true;
      best = max(best, m);
    }
  }
  // the greatest H; of equal ones the smallest k, then the smallest p
  const int Hm = wave_max(topH);
  const int km = wave_min(topH == Hm ? topK : INT_MAX);
  const int mine = (km - d) >> 1;
  const int pm = wave_min(topH == Hm && topK == km ? mine : INT_MAX);
  const int gm = wave_max(topH == Hm && topK == km && mine == pm ? topG : INT_MIN);
  return GapSide{Hm, pm, km - pm, gm};
}

__global__ __launch_bounds__(256) void k_search_gapped(const GapArgs A) {
  const int a = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (a >= A.n) return;                          // the whole wave
  const int lane = threadIdx.x & 63;
  const GapAnchor an = A.anchor[a];
  const int gsub = an.sm >> 1, strand = an.sm & 1;
  int M, vbase;
  chunk_place(A.ch, gsub, strand, &M, &vbase);
  const int c0 = A.ix.coff[an.contig], Lc = A.ix.coff[an.contig + 1] - c0;
  // bounds before any load; an anchor outside them (never made by the host) extends nowhere
  const int i0 = min(max(an.i0, 0), M), j0 = min(max(an.j0, 0), Lc);
  GapRaw out;
  out.right = gap_side<false>(A, strand, vbase + i0, c0 + j0, M - i0, Lc - j0, lane);
  out.left = gap_side<true>(A, strand, vbase + i0 - 1, c0 + j0 - 1, i0, j0, lane);
  if (lane == 0) A.out[a] = out;
}

int gapped_device(MapState* st, const std::vector<GapAnchor>& anchors, int band, int xdrop_gap, int64_t total,
                  std::vector<GapRaw>* raw, hipStream_t s, std::string* err) {
  SearchState* ss = &st->search;                 // search_records left the chunk in it: there are anchors
  MAP_RC(ss->g_anchor.ensure(kGapLaunch, err));
  MAP_RC(ss->g_out.ensure(kGapLaunch, err));
  GapArgs A{};
  A.ix = map_view(st);
  A.ch = chunk_view(*ss, total);
  A.W = band;
  A.X2 = 2 * xdrop_gap;
  A.anchor = ss->g_anchor.p;
  A.out = ss->g_out.p;
  raw->resize(anchors.size());
  for (size_t a0 = 0; a0 < anchors.size(); a0 += kGapLaunch) {
    A.n = (int)std::min<size_t>(kGapLaunch, anchors.size() - a0);
    MAP_TRY(hipMemcpyAsync(ss->g_anchor.p, anchors.data() + a0, sizeof(GapAnchor) * A.n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_search_gapped, dim3((unsigned)((A.n + 3) / 4)), dim3(256), 0, s, A);
    MAP_TRY(hipGetLastError());
    MAP_TRY(hipMemcpyAsync(raw->data() + a0, ss->g_out.p, sizeof(GapRaw) * A.n, hipMemcpyDeviceToHost, s));
    MAP_TRY(hipStreamSynchronize(s));
  }
  return 0;
}

}  // namespace

int gapped_launches(MapState* st, const GapAnchor* anchor, int64_t n, int band, int xdrop_gap, int64_t total,
                    GapRaw* out, hipStream_t s, std::string* err) {
  GapArgs A{};
  A.ix = map_view(st);
  A.ch = chunk_view(st->search, total);
  A.W = band;
  A.X2 = 2 * xdrop_gap;
  for (int64_t a0 = 0; a0 < n; a0 += kGapLaunch) {
    A.anchor = anchor + a0;
    A.out = out + a0;
    A.n = (int)std::min<int64_t>(kGapLaunch, n - a0);
    hipLaunchKernelGGL(k_search_gapped, dim3((unsigned)((A.n + 3) / 4)), dim3(256), 0, s, A);
    MAP_TRY(hipGetLastError());
  }
  return 0;
}

namespace {

// search_gapped_run with the reporting step on the device: the kept alignments, sorted, in *kept
// (the first `capacity` of *n)
int gapped_on_device(MapState* st, const ChunkSource& src, const int64_t* off, int64_t n_subjects,
                     const SearchRule& rule, int band, int xdrop_gap, int64_t capacity, std::vector<GapAln>* kept,
                     int64_t* n, SearchStats* stats, SearchGapStats* gstats, hipStream_t s, std::string* err) {
  SearchState* ss = &st->search;
  int64_t n_recs = 0;
  MAP_RC(search_records_device(st, src, off, n_subjects, rule, &n_recs, stats, s, err));
  gstats->anchors = n_recs;
  if (n_recs == 0) return 0;
  return synced_on_error(s, [&]() -> int {
    MAP_RC(ss->g_anchor.ensure((size_t)n_recs, err));
    MAP_RC(ss->g_out.ensure((size_t)n_recs, err));
    MAP_RC(report_anchors(ss->rep.rec_sorted.p, n_recs, ss->g_anchor.p, s, err));
    MAP_RC(gapped_launches(st, ss->g_anchor.p, n_recs, band, xdrop_gap, off[n_subjects], ss->g_out.p, s, err));
    int64_t longest = 0;
    for (int64_t g = 0; g < n_subjects; ++g) longest = std::max(longest, off[g + 1] - off[g]);
    // a side's p <= its part of the subject, q <= its part of the contig, 0 <= H <= 2 p, g <= p + q
    const int64_t span = longest + st->total;
    RepBounds B{};
    B.hi[kRepSm] = 2 * n_subjects - 1;
    B.hi[kRepContig] = std::max(st->n_contigs - 1, 0);
    B.hi[kRepScore2] = 4 * longest;
    B.hi[kRepQstart] = B.hi[kRepQspan] = st->total;
    B.hi[kRepSstart] = B.hi[kRepSspan] = longest;
    B.hi[kRepLength] = B.hi[kRepMatches] = B.hi[kRepGaps] = 2 * span;
    MAP_RC(report_alns_device(&ss->rep, ss->g_anchor.p, ss->g_out.p, n_recs, rule.min_score, B, n,
                              &gstats->raw_alignments, s, err));
    kept->resize((size_t)std::min<int64_t>(*n, capacity));
    if (!kept->empty())
      MAP_TRY(hipMemcpy(kept->data(), ss->rep.aln_sorted.p, kept->size() * sizeof(GapAln), hipMemcpyDeviceToHost));
    return 0;
  });
}

}  // namespace

int search_gapped_run(MapState* st, const ChunkSource& src, const int64_t* off, int64_t n_subjects, const SearchRule& rule,
                      int band, int xdrop_gap, const SearchGapOut& out, int64_t* n, SearchStats* stats,
                      SearchGapStats* gstats, hipStream_t s, std::string* err) {
  *n = 0;
  *gstats = SearchGapStats{0, 0};
  std::vector<GapAln> kept;
  if (st->search.report_on) {
    MAP_RC(gapped_on_device(st, src, off, n_subjects, rule, band, xdrop_gap, out.capacity, &kept, n, stats, gstats, s,
                            err));
  } else {
    std::vector<SearchRec> recs;
    MAP_RC(search_records(st, src, off, n_subjects, rule, &recs, stats, s, err));
    gstats->anchors = (int64_t)recs.size();
    if (recs.empty()) return 0;
    std::vector<GapAnchor> anchors(recs.size());
    for (size_t i = 0; i < recs.size(); ++i) {
      const SearchRec& r = recs[i];
      const int32_t i0 = r.sstart + r.length / 2;
      anchors[i] = GapAnchor{r.subject << 1 | r.minus, r.contig, i0, i0 + (r.qstart - r.sstart)};
    }
    std::vector<GapRaw> raw;
    const int rc = gapped_device(st, anchors, band, xdrop_gap, off[n_subjects], &raw, s, err);
    if (rc) {
      (void)hipStreamSynchronize(s);
      return rc;
    }
    report_alns_host(anchors, raw, rule.min_score, &kept, &gstats->raw_alignments);
    *n = (int64_t)kept.size();
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
