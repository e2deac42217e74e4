// Homology search on MI355X (gfx950): ungapped seed-and-extend of database genes (the
// subjects, streamed in chunks) against the contigs the mapper's index holds (wf_map_index).
// DESIGN.md §12 states the rule; tests/search_oracle.py restates it on the CPU.  Not a blastn
// clone: ungapped HSPs only, no composition statistics; masking only after wf_search_mask
// (wf_dust.hip), which takes the low-complexity S-mers out of the index.
//
// One chunk (search_run):
//   k_map_pack / k_search_pack_rc  the chunk as bit planes (wf_mapstore.h) in both orientations:
//                    the minus store is the reverse complement of the whole chunk, so subject
//                    [o, o') lies at [total - o', total - o) in it, reverse-complemented
//   then, per tile of at most kSearchTile seed slots (slot = strand, subject, offset a = kT):
//   k_search_count   thread per slot: the S-mer of the variant, its bucket, the first of its
//                    occurrences in the sorted index and their number (0 when the seed holds
//                    an N, is absent or occurs more than max_occ times)
//   device exclusive scan of the counts: every seed hit of the tile gets a number
//   k_search_extend  thread per seed hit, in launches of at most kSearchLaunch hits: the hit's
//                    slot by a search in the scanned counts, its contig, the bounds of its
//                    diagonal from coff[c], coff[c + 1] and the subject's ends (before any
//                    load), then the x-drop walk to the right and to the left over 32-column
//                    mismatch words, a run of matches at a time.  A hit whose predecessor
//                    (a - T, same diagonal) is a seed hit too gives the same HSP and is skipped.
//   The HSPs go to the host, which sorts them per (subject, strand, contig, diagonal), counts
//   identical ones once, drops the strictly contained and those below min_score.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <tuple>
#include <vector>

#include "wf_internal.h"
#include "wf_mapstore.h"
#include "wf_searchstate.h"

namespace wf {

struct SearchRaw {            // one extended seed hit
  int32_t sm;                 // subject << 1 | minus
  int32_t contig;
  int32_t delta;              // contig position - variant position
  int32_t b, e;               // [b, e) on the variant
  int32_t score;
};

void search_destroy(SearchState* ss) {
  if (!ss) return;
  MapBuf* bufs[] = {&ss->seq, &ss->off, &ss->soff, &ss->pk[0], &ss->pk[1], &ss->nm[0], &ss->nm[1],
                    &ss->cnt, &ss->first, &ss->start, &ss->tmp, &ss->raw, &ss->ctr, &ss->g_anchor, &ss->g_out};
  for (MapBuf* b : bufs) map_release(*b);
  delete ss;
}

namespace {

constexpr int kSearchLaunch = 1 << 20;          // seed hits per k_search_extend launch
constexpr int kSearchTile = 1 << 24;            // seed slots per tile, and
constexpr int64_t kSearchTileHits = 1 << 30;    //   slots * max_occ: the scan stays in int32

struct SearchArgs {
  MapIndexView ix;            // the contigs
  const uint2* vpk[2];        // the chunk: plus store, minus store
  const uint32_t* vnm[2];
  const int64_t* off;         // [n + 1] the subjects' starts in the chunk
  const int64_t* soff;        // [n + 1] first seed slot of each subject (of one strand)
  int n_subjects;
  int T, max_occ, X;
  int64_t NS, total;          // seed slots of one strand; bases of the chunk
  int64_t t0;                 // the tile: slots [t0, t0 + nt) of the 2 NS
  int nt;
  int32_t* cnt;               // [nt]
  int32_t* first;             // [nt]
  const int32_t* start;       // [nt] exclusive scan of cnt
  int h0, nh;                 // the launch: seed hits [h0, h0 + nh) of the tile
  SearchRaw* raw;             // [kSearchLaunch]
  unsigned long long* ctr;    // [0] HSPs written, [1] seed hits skipped
};

struct SearchSeed {
  int g, strand, a, M, vbase; // subject, strand, seed offset, subject length, its start in the store
};

__device__ __forceinline__ SearchSeed search_seed(const SearchArgs& A, int64_t t) {
  SearchSeed sd;
  sd.strand = t >= A.NS;
  const int64_t s = t - (sd.strand ? A.NS : 0);
  int lo = 0, hi = A.n_subjects;                 // invariant: soff[lo] <= s < soff[hi]
  while (hi - lo > 1) {
    const int mid = (int)(((int64_t)lo + hi) >> 1);
    if (A.soff[mid] <= s) lo = mid; else hi = mid;
  }
  sd.g = lo;
  sd.a = (int)(s - A.soff[lo]) * A.T;
  const int64_t o0 = A.off[lo], o1 = A.off[lo + 1];
  sd.M = (int)(o1 - o0);
  sd.vbase = (int)(sd.strand ? A.total - o1 : o0);
  return sd;
}

__global__ void k_search_pack_rc(const unsigned char* seq, int64_t total, int64_t words, uint2* pk, uint32_t* nm) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= words) return;
  uint32_t lo = 0, hi = 0, n = 0;
  for (int b = 0; b < 32; ++b) {
    const int64_t i = w * 32 + b;
    int code = i < total ? base_code(seq[total - 1 - i]) : 4;   // the padding is N
    if (code < 4) code = 3 - code;
    lo |= (uint32_t)(code & 1) << b;
    hi |= (uint32_t)((code >> 1) & 1) << b;
    n |= (uint32_t)(code >> 2) << b;
  }
  pk[w] = make_uint2(lo & ~n, hi & ~n);
  nm[w] = n;
}

__global__ __launch_bounds__(256) void k_search_count(const SearchArgs A) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.nt) return;
  const SearchSeed sd = search_seed(A, A.t0 + j);
  MapIndexView v = A.ix;                         // store_kmer on the chunk's planes
  v.pk = A.vpk[sd.strand];
  v.nm = A.vnm[sd.strand];
  uint64_t key = 0;
  int cnt = 0, first = 0;
  if (store_kmer(v, sd.vbase + sd.a, &key)) {    // a + S <= M: words W, W + 1 are in the store
    const uint32_t b = (uint32_t)(key >> A.ix.bshift);
    int lo = (int)A.ix.bucket[b];
    const int end = (int)A.ix.bucket[b + 1];
    int hi = end;
    while (lo < hi) {                            // lower bound within the bucket
      const int mid = (lo + hi) >> 1;
      if (A.ix.keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    first = lo;
    hi = end;
    while (lo < hi) {                            // upper bound
      const int mid = (lo + hi) >> 1;
      if (A.ix.keys[mid] <= key) lo = mid + 1; else hi = mid;
    }
    cnt = lo - first;
    if (cnt > A.max_occ) cnt = 0;
  }
  A.cnt[j] = cnt;
  A.first[j] = first;
}

// mismatch bits of the 32 columns whose first lies at position vp of the variant store and gp
// of the contig store; either may be as low as -32 (the bases before a store are N)
__device__ __forceinline__ uint32_t search_mis(const SearchArgs& A, int strand, int vp, int gp) {
  const uint2* pk = A.vpk[strand];
  const uint32_t* nm = A.vnm[strand];
  const int W = vp >> 5, sh = vp & 31;
  uint2 a = make_uint2(0u, 0u);
  uint32_t na = ~0u;
  if (W >= 0) {
    a = pk[W];
    na = nm[W];
  }
  const uint2 b = pk[W + 1];
  const uint32_t vlo = window32(a.x, b.x, sh), vhi = window32(a.y, b.y, sh), vn = window32(na, nm[W + 1], sh);
  return map_mis_word<true>(A.ix, &vlo, &vhi, &vn, 0, gp);
}

// The x-drop walk over the n columns of one word, bit k of m: the k-th column walked is a
// mismatch.  cols: the columns walked before this word; ext: the columns up to the best.
// false: the drop exceeded X.
__device__ __forceinline__ bool search_walk(uint32_t m, int n, int X, int cols, int& r, int& best, int& ext) {
  int b = 0;
  while (b < n) {
    const uint32_t rest = m >> b;
    int run = rest ? __ffs((int)rest) - 1 : 32;  // matches before the next mismatch
    run = min(run, n - b);
    if (run > 0) {
      r += run;
      b += run;
      if (r > best) { best = r; ext = cols + b; }
    }
    if (b < n) {
      r -= 2;
      ++b;
      if (best - r > X) return false;
    }
  }
  return true;
}

// Loads: a column i is read only with ibeg <= i < iend, that is inside the subject and inside
// contig c.  A word starts at most 31 columns before such a column, so its first store word
// is W >= -1 (guarded) and its second W + 1 <= (total - 1) / 32 + 1, inside the padding.
__global__ __launch_bounds__(256) void k_search_extend(const SearchArgs A) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= A.nh) return;
  const int h = A.h0 + idx;
  const MapIndexView& ix = A.ix;
  int lo = 0, hi = A.nt;                         // the last slot with start <= h: the hit's own
  while (hi - lo > 1) {
    const int mid = (int)(((int64_t)lo + hi) >> 1);
    if (A.start[mid] <= h) lo = mid; else hi = mid;
  }
  const int j = lo;
  const SearchSeed sd = search_seed(A, A.t0 + j);
  const int q = ix.kpos[A.first[j] + (h - A.start[j])];
  const int c = contig_of(ix.coff, ix.n_contigs, q);
  const int c0 = ix.coff[c], c1 = ix.coff[c + 1];
  const int D = q - sd.a;                        // store position of variant column 0
  const int S = ix.S, T = A.T;
  // the predecessor a - T on this diagonal is a seed hit when its seed is usable and the T
  // columns before this seed match inside the contig: it yields the same HSP.  With a
  // low-complexity mask the index lacks the occurrences that hold a masked base, so the
  // occurrence at q - T counts only when its S bases are unmasked.
  if (sd.a >= T && j > 0 && A.cnt[j - 1] > 0 && q - T >= c0) {
    uint32_t mis = search_mis(A, sd.strand, sd.vbase + sd.a - T, q - T);
    if (T < 32) mis &= (1u << T) - 1u;
    if (ix.dm) {                                 // q - T >= 0; words W, W + 1 are in the plane
      const int W = (q - T) >> 5, sh = (q - T) & 31;
      const uint32_t smask = S == 32 ? 0xFFFFFFFFu : (1u << S) - 1u;
      mis |= window32(ix.dm[W], ix.dm[W + 1], sh) & smask;
    }
    if (mis == 0) {
      atomicAdd(&A.ctr[1], 1ull);
      return;
    }
  }
  const int ibeg = max(0, c0 - D), iend = min(sd.M, c1 - D);
  int r = 0, best_r = 0, ext_r = 0;
  for (int i = sd.a + S, cols = 0; i < iend;) {
    const int n = min(32, iend - i);
    const uint32_t mis = search_mis(A, sd.strand, sd.vbase + i, D + i);
    if (!search_walk(mis, n, A.X, cols, r, best_r, ext_r)) break;
    i += n;
    cols += n;
  }
  int best_l = 0, ext_l = 0;
  r = 0;
  for (int i = sd.a - 1, cols = 0; i >= ibeg;) {
    const int n = min(32, i - ibeg + 1);
    const uint32_t mis = __brev(search_mis(A, sd.strand, sd.vbase + i - 31, D + i - 31));
    if (!search_walk(mis, n, A.X, cols, r, best_l, ext_l)) break;
    i -= n;
    cols += n;
  }
  SearchRaw out;
  out.sm = sd.g << 1 | sd.strand;
  out.contig = c;
  out.delta = D - c0;
  out.b = sd.a - ext_l;
  out.e = sd.a + S + ext_r;
  out.score = S + best_r + best_l;
  A.raw[atomicAdd(&A.ctr[0], 1ull)] = out;       // at most nh <= kSearchLaunch per launch
}

#define SEARCH_TRY(x)                                                                     \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) { *err = std::string(#x) + ": " + hipGetErrorString(e_); return -2; } \
  } while (0)
#define SEARCH_RC(x)                 \
  do {                               \
    const int rc_ = (x);             \
    if (rc_) return rc_;             \
  } while (0)

// the seed hits of the chunk, extended: appended to *raw
int search_device(MapState* st, const char* seq, const int64_t* off, int64_t n, const SearchRule& rule,
                  std::vector<SearchRaw>* raw, SearchStats* stats, hipStream_t s, std::string* err) {
  if (!st->search) st->search = new SearchState();
  SearchState* ss = st->search;
  const int64_t total = off[n];
  const int S = st->seed_len;
  std::vector<int64_t> soff((size_t)n + 1, 0);
  for (int64_t g = 0; g < n; ++g) {
    const int64_t M = off[g + 1] - off[g];
    soff[g + 1] = soff[g] + (M >= S ? (M - S) / rule.stride + 1 : 0);
  }
  const int64_t NS = soff[n];
  if (NS == 0) return 0;
  const int64_t words = (total + 31) / 32 + 2;
  SEARCH_RC(map_ensure(ss->seq, (size_t)total, err));
  SEARCH_RC(map_ensure(ss->off, sizeof(int64_t) * (n + 1), err));
  SEARCH_RC(map_ensure(ss->soff, sizeof(int64_t) * (n + 1), err));
  for (int v = 0; v < 2; ++v) {
    SEARCH_RC(map_ensure(ss->pk[v], (size_t)words * sizeof(uint2), err));
    SEARCH_RC(map_ensure(ss->nm[v], (size_t)words * sizeof(uint32_t), err));
  }
  const int tile = (int)std::min<int64_t>(kSearchTile, kSearchTileHits / rule.max_occ);
  const int64_t tile_cap = std::min<int64_t>(tile, 2 * NS);
  SEARCH_RC(map_ensure(ss->cnt, sizeof(int32_t) * tile_cap, err));
  SEARCH_RC(map_ensure(ss->first, sizeof(int32_t) * tile_cap, err));
  SEARCH_RC(map_ensure(ss->start, sizeof(int32_t) * tile_cap, err));
  SEARCH_RC(map_ensure(ss->raw, sizeof(SearchRaw) * kSearchLaunch, err));
  SEARCH_RC(map_ensure(ss->ctr, 2 * sizeof(unsigned long long), err));
  SEARCH_TRY(hipMemcpyAsync(ss->seq.p, seq, (size_t)total, hipMemcpyHostToDevice, s));
  SEARCH_TRY(hipMemcpyAsync(ss->off.p, off, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, s));
  SEARCH_TRY(hipMemcpyAsync(ss->soff.p, soff.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, s));
  const unsigned pack_blocks = (unsigned)((words + 255) / 256);
  hipLaunchKernelGGL(k_map_pack, dim3(pack_blocks), dim3(256), 0, s, static_cast<const unsigned char*>(ss->seq.p),
                     total, words, static_cast<uint2*>(ss->pk[0].p), static_cast<uint32_t*>(ss->nm[0].p));
  SEARCH_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_search_pack_rc, dim3(pack_blocks), dim3(256), 0, s,
                     static_cast<const unsigned char*>(ss->seq.p), total, words, static_cast<uint2*>(ss->pk[1].p),
                     static_cast<uint32_t*>(ss->nm[1].p));
  SEARCH_TRY(hipGetLastError());

  SearchArgs A{};
  A.ix = map_view(st);
  for (int v = 0; v < 2; ++v) {
    A.vpk[v] = static_cast<const uint2*>(ss->pk[v].p);
    A.vnm[v] = static_cast<const uint32_t*>(ss->nm[v].p);
  }
  A.off = static_cast<const int64_t*>(ss->off.p);
  A.soff = static_cast<const int64_t*>(ss->soff.p);
  A.n_subjects = (int)n;
  A.T = rule.stride;
  A.max_occ = rule.max_occ;
  A.X = rule.xdrop;
  A.NS = NS;
  A.total = total;
  A.cnt = static_cast<int32_t*>(ss->cnt.p);
  A.first = static_cast<int32_t*>(ss->first.p);
  A.start = static_cast<const int32_t*>(ss->start.p);
  A.raw = static_cast<SearchRaw*>(ss->raw.p);
  A.ctr = static_cast<unsigned long long*>(ss->ctr.p);
  size_t tmp_bytes = 0;
  SEARCH_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, A.cnt, static_cast<int32_t*>(ss->start.p),
                                              (int)tile_cap, s));
  SEARCH_RC(map_ensure(ss->tmp, tmp_bytes, err));
  for (int64_t t0 = 0; t0 < 2 * NS; t0 += tile) {
    A.t0 = t0;
    A.nt = (int)std::min<int64_t>(tile, 2 * NS - t0);
    hipLaunchKernelGGL(k_search_count, dim3((unsigned)((A.nt + 255) / 256)), dim3(256), 0, s, A);
    SEARCH_TRY(hipGetLastError());
    size_t tb = ss->tmp.bytes;
    SEARCH_TRY(hipcub::DeviceScan::ExclusiveSum(ss->tmp.p, tb, A.cnt, static_cast<int32_t*>(ss->start.p), A.nt, s));
    int32_t last_cnt = 0, last_start = 0;
    SEARCH_TRY(hipMemcpyAsync(&last_cnt, A.cnt + (A.nt - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SEARCH_TRY(hipMemcpyAsync(&last_start, A.start + (A.nt - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SEARCH_TRY(hipStreamSynchronize(s));
    const int64_t hits = (int64_t)last_cnt + last_start;
    stats->seed_hits += hits;
    if (stats->seed_hits > 0x7FFFFFFFll) {
      *err = "more than 2^31 - 1 seed hits in one chunk";
      return -7;
    }
    for (int64_t h0 = 0; h0 < hits; h0 += kSearchLaunch) {
      A.h0 = (int)h0;
      A.nh = (int)std::min<int64_t>(kSearchLaunch, hits - h0);
      unsigned long long ctr[2] = {0, 0};
      SEARCH_TRY(hipMemsetAsync(ss->ctr.p, 0, sizeof ctr, s));
      hipLaunchKernelGGL(k_search_extend, dim3((unsigned)((A.nh + 255) / 256)), dim3(256), 0, s, A);
      SEARCH_TRY(hipGetLastError());
      SEARCH_TRY(hipMemcpyAsync(ctr, ss->ctr.p, sizeof ctr, hipMemcpyDeviceToHost, s));
      SEARCH_TRY(hipStreamSynchronize(s));
      stats->skipped += (int64_t)ctr[1];
      const size_t had = raw->size(), got = (size_t)std::min<unsigned long long>(ctr[0], kSearchLaunch);
      raw->resize(had + got);
      if (got) SEARCH_TRY(hipMemcpy(raw->data() + had, ss->raw.p, got * sizeof(SearchRaw), hipMemcpyDeviceToHost));
    }
  }
  return 0;
}

}  // namespace

int search_records(MapState* st, const char* seq, const int64_t* off, int64_t n_subjects, const SearchRule& rule,
                   std::vector<SearchRec>* recs_out, SearchStats* stats, hipStream_t s, std::string* err) {
  std::vector<SearchRec>& recs = *recs_out;
  recs.clear();
  *stats = SearchStats{0, 0, 0};
  if (n_subjects == 0 || st->n_kmers == 0) return 0;
  std::vector<SearchRaw> raw;
  const int rc = search_device(st, seq, off, n_subjects, rule, &raw, stats, s, err);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  stats->raw_hsps = (int64_t)raw.size();
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
    if (contained || x.score < rule.min_score) continue;
    const int length = x.e - x.b;
    recs.push_back(Rec{x.contig, x.sm >> 1, x.sm & 1, x.b + x.delta, x.b, length, (x.score + 2 * length) / 3});
  }
  std::sort(recs.begin(), recs.end(), [](const Rec& x, const Rec& y) {
    return std::make_tuple(x.contig, x.subject, x.minus, x.qstart, x.sstart, x.length) <
           std::make_tuple(y.contig, y.subject, y.minus, y.qstart, y.sstart, y.length);
  });
  return 0;
}

int search_run(MapState* st, const char* seq, const int64_t* off, int64_t n_subjects, const SearchRule& rule,
               const SearchOut& out, int64_t* n, SearchStats* stats, hipStream_t s, std::string* err) {
  *n = 0;
  std::vector<SearchRec> recs;
  const int rc = search_records(st, seq, off, n_subjects, rule, &recs, stats, s, err);
  if (rc) return rc;
  *n = (int64_t)recs.size();
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

}  // namespace wf
