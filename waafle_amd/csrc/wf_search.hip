// Homology search on MI355X (gfx950): ungapped seed-and-extend of database genes (the
// subjects, streamed in chunks) against the contigs the mapper's index holds (wf_map_index).
// DESIGN.md §12 states the rule; tests/search_oracle.py restates it on the CPU.  Not a blastn
// clone: ungapped HSPs only, no composition statistics; masking only after wf_search_mask
// (wf_dust.hip), which takes the low-complexity S-mers out of the index.
//
// One chunk (search_run):
//   map_pack twice   (k_map_pack, wf_map.hip) the chunk as bit planes in both orientations:
//                    the minus store is the reverse complement of the whole chunk, so subject
//                    [o, o') lies at [total - o', total - o) in it, reverse-complemented
//   or, for a chunk given as the bit planes of a packed database (ChunkSource):
//   k_search_unpack  thread per store word: the same two stores from the three planes as they
//                    lie in the file, at any bit offset; no ASCII on the device
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
//   The reporting step (wf_report.hip) sorts the HSPs per (subject, strand, contig, diagonal),
//   counts identical ones once, drops the strictly contained and those below min_score: on the
//   host, to which every launch's HSPs are copied, or (SearchState::report_on)
//   on the device, where the launches append to one array with nothing between them.
#include <algorithm>
#include <string>
#include <tuple>
#include <vector>

#include "wf_internal.h"
#include "wf_mapstore.h"

namespace wf {

namespace {

constexpr int kSearchLaunch = 1 << 20;          // seed hits per k_search_extend launch
constexpr int kSearchTile = 1 << 24;            // seed slots per tile, and
constexpr int64_t kSearchTileHits = 1 << 30;    //   slots * max_occ: the scan stays in int32

struct SearchArgs {
  MapIndexView ix;            // the contigs
  ChunkView ch;               // the chunk
  const int64_t* soff;        // [n + 1] first seed slot of each subject (of one strand)
  int n_subjects;
  int T, max_occ, X;
  int64_t NS;                 // seed slots of one strand
  int64_t t0;                 // the tile: slots [t0, t0 + nt) of the 2 NS
  int nt;
  int32_t* cnt;               // [nt]
  int32_t* first;             // [nt]
  const int32_t* start;       // [nt] exclusive scan of cnt
  int h0, nh;                 // the launch: seed hits [h0, h0 + nh) of the tile
  SearchRaw* raw;             // [kSearchLaunch]; the device form: room for every seed hit so far
  unsigned long long* ctr;    // [0] HSPs written, [1] seed hits skipped (the device form: of the chunk)
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
  chunk_place(A.ch, lo, sd.strand, &sd.M, &sd.vbase);
  return sd;
}

__global__ __launch_bounds__(256) void k_search_count(const SearchArgs A) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.nt) return;
  const SearchSeed sd = search_seed(A, A.t0 + j);
  uint64_t key = 0;
  int cnt = 0, first = 0;
  // a + S <= M: words W, W + 1 are in the chunk's store
  if (planes_kmer(A.ch.vpk[sd.strand], A.ch.vnm[sd.strand], A.ix.S, sd.vbase + sd.a, &key)) {
    int hi;
    int lo = first = index_lower_bound(A.ix, key, &hi);
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
    uint32_t mis = chunk_mis(ix, A.ch, sd.strand, sd.vbase + sd.a - T, q - T);
    if (T < 32) mis &= (1u << T) - 1u;
    if (ix.dm) mis |= plane_window(ix.dm, q - T) & smer_mask(S);   // q - T >= 0: inside the plane
    if (mis == 0) {
      atomicAdd(&A.ctr[1], 1ull);
      return;
    }
  }
  const int ibeg = max(0, c0 - D), iend = min(sd.M, c1 - D);
  int r = 0, best_r = 0, ext_r = 0;
  for (int i = sd.a + S, cols = 0; i < iend;) {
    const int n = min(32, iend - i);
    const uint32_t mis = chunk_mis(ix, A.ch, sd.strand, sd.vbase + i, D + i);
    if (!search_walk(mis, n, A.X, cols, r, best_r, ext_r)) break;
    i += n;
    cols += n;
  }
  int best_l = 0, ext_l = 0;
  r = 0;
  for (int i = sd.a - 1, cols = 0; i >= ibeg;) {
    const int n = min(32, i - ibeg + 1);
    const uint32_t mis = __brev(chunk_mis(ix, A.ch, sd.strand, sd.vbase + i - 31, D + i - 31));
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
  // at most nh <= kSearchLaunch per launch; the device form counts on: at most the seed hits so far
  A.raw[atomicAdd(&A.ctr[0], 1ull)] = out;
}

struct UnpackArgs {
  const uint32_t* in[3];      // lo, hi, nn as uploaded: [n_words] each
  int64_t n_words;
  int64_t total;              // bases of the chunk; base i is bit bit0 + i of the planes
  int64_t words;              // (total + 31) / 32 + 2 store words per strand
  int bit0;
  uint2* pk[2];
  uint32_t* nm[2];
};

// bits [b, b + 32) of plane p, b >= -31; the words outside [0, n_words) are not loaded and
// read as 0 (the caller makes those positions N)
__device__ __forceinline__ uint32_t unpack_window(const uint32_t* p, int64_t n_words, int64_t b) {
  const int64_t W = b >> 5;                      // floor: -1 for a negative b
  const int sh = (int)(b & 31);
  const uint32_t x = W >= 0 && W < n_words ? p[W] : 0u;
  const uint32_t y = sh && W + 1 < n_words ? p[W + 1] : 0u;
  return window32(x, y, sh);
}

// Store word w of both strands from the file's planes.  Plus: chunk positions [32 w, 32 w + 32),
// the window at bit bit0 + 32 w.  Minus: positions total - 1 - 32 w downwards, complemented: the
// window at bit0 + total - 32 (w + 1) (negative by up to 31 bits in the last word with bases),
// bit-reversed, both base planes flipped.  Either way bit k is a base of the chunk exactly when
// k < total - 32 w, so one mask serves both; every other bit is N, and lo, hi are cleared under
// N here, whatever the file holds.  A word without bases loads nothing.
__global__ __launch_bounds__(256) void k_search_unpack(const UnpackArgs A) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= A.words) return;
  const int64_t left = A.total - 32 * w;
  uint32_t plo = 0, phi = 0, pn = ~0u, mlo = 0, mhi = 0, mn = ~0u;
  if (left > 0) {
    const uint32_t pad = left < 32 ? ~0u << (int)left : 0u;
    const int64_t bp = A.bit0 + 32 * w, bm = A.bit0 + left - 32;
    pn = unpack_window(A.in[2], A.n_words, bp) | pad;
    plo = unpack_window(A.in[0], A.n_words, bp) & ~pn;
    phi = unpack_window(A.in[1], A.n_words, bp) & ~pn;
    mn = __brev(unpack_window(A.in[2], A.n_words, bm)) | pad;
    mlo = ~__brev(unpack_window(A.in[0], A.n_words, bm)) & ~mn;
    mhi = ~__brev(unpack_window(A.in[1], A.n_words, bm)) & ~mn;
  }
  A.pk[0][w] = make_uint2(plo, phi);
  A.nm[0][w] = pn;
  A.pk[1][w] = make_uint2(mlo, mhi);
  A.nm[1][w] = mn;
}

// the chunk's stores pk, nm of both strands from src, enqueued on s; search_device has made
// room in ss->seq or ss->planes
int search_store(SearchState* ss, const ChunkSource& src, int64_t total, hipStream_t s, std::string* err) {
  if (src.seq) {
    MAP_TRY(hipMemcpyAsync(ss->seq.p, src.seq, (size_t)total, hipMemcpyHostToDevice, s));
    for (int v = 0; v < 2; ++v) MAP_RC(map_pack(ss->seq.p, total, v == 1, ss->pk[v].p, ss->nm[v].p, s, err));
    return 0;
  }
  UnpackArgs U{};
  U.n_words = src.n_words;
  U.total = total;
  U.words = (total + 31) / 32 + 2;
  U.bit0 = src.bit0;
  const uint32_t* from[3] = {src.lo, src.hi, src.nn};
  for (int k = 0; k < 3; ++k) {
    uint32_t* to = ss->planes.p + (size_t)k * src.n_words;
    MAP_TRY(hipMemcpyAsync(to, from[k], sizeof(uint32_t) * (size_t)src.n_words, hipMemcpyHostToDevice, s));
    U.in[k] = to;
  }
  for (int v = 0; v < 2; ++v) {
    U.pk[v] = ss->pk[v].p;
    U.nm[v] = ss->nm[v].p;
  }
  hipLaunchKernelGGL(k_search_unpack, dim3((unsigned)((U.words + 255) / 256)), dim3(256), 0, s, U);
  MAP_TRY(hipGetLastError());
  return 0;
}

// the seed hits of the chunk, extended: appended to *raw; or, with raw null (the device form of
// the reporting step), left in ss->raw, *n_raw of them
int search_device(MapState* st, const ChunkSource& src, const int64_t* off, int64_t n, const SearchRule& rule,
                  std::vector<SearchRaw>* raw, int64_t* n_raw, SearchStats* stats, hipStream_t s, std::string* err) {
  SearchState* ss = &st->search;
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
  const int tile = (int)std::min<int64_t>(kSearchTile, kSearchTileHits / rule.max_occ);
  const int64_t tile_cap = std::min<int64_t>(tile, 2 * NS);
  if (src.seq) MAP_RC(ss->seq.ensure(total, err));           // ss->seq is not touched by a packed chunk
  else MAP_RC(ss->planes.ensure(3 * (size_t)src.n_words, err));
  MAP_RC(ss->off.ensure(n + 1, err));
  MAP_RC(ss->soff.ensure(n + 1, err));
  for (int v = 0; v < 2; ++v) {
    MAP_RC(ss->pk[v].ensure(words, err));
    MAP_RC(ss->nm[v].ensure(words, err));
  }
  MAP_RC(ss->cnt.ensure(tile_cap, err));
  MAP_RC(ss->first.ensure(tile_cap, err));
  MAP_RC(ss->start.ensure(tile_cap, err));
  if (raw) MAP_RC(ss->raw.ensure(kSearchLaunch, err));
  MAP_RC(ss->ctr.ensure(2, err));
  if (!raw) MAP_TRY(hipMemsetAsync(ss->ctr.p, 0, 2 * sizeof(unsigned long long), s));
  MAP_RC(scan_reserve(ss->tmp, (int)tile_cap, s, err));      // the largest tile: the loop allocates nothing
  MAP_TRY(hipMemcpyAsync(ss->off.p, off, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, s));
  MAP_TRY(hipMemcpyAsync(ss->soff.p, soff.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, s));
  MAP_RC(search_store(ss, src, total, s, err));
  ss->resident = total;

  SearchArgs A{};
  A.ix = map_view(st);
  A.ch = chunk_view(*ss, total);
  A.soff = ss->soff.p;
  A.n_subjects = (int)n;
  A.T = rule.stride;
  A.max_occ = rule.max_occ;
  A.X = rule.xdrop;
  A.NS = NS;
  A.cnt = ss->cnt.p;
  A.first = ss->first.p;
  A.start = ss->start.p;
  A.ctr = ss->ctr.p;
  for (int64_t t0 = 0; t0 < 2 * NS; t0 += tile) {
    A.t0 = t0;
    A.nt = (int)std::min<int64_t>(tile, 2 * NS - t0);
    hipLaunchKernelGGL(k_search_count, dim3((unsigned)((A.nt + 255) / 256)), dim3(256), 0, s, A);
    MAP_TRY(hipGetLastError());
    int64_t hits = 0;
    MAP_RC(scan_total(ss->cnt.p, ss->start.p, A.nt, ss->tmp, &hits, s, err));
    stats->seed_hits += hits;
    if (stats->seed_hits > 0x7FFFFFFFll) {
      *err = "more than 2^31 - 1 seed hits in one chunk";
      return -7;
    }
    // the device form: every seed hit so far may have left an HSP (the scan's total has just
    // synchronised, so the array can grow with its contents kept)
    if (!raw) MAP_RC(grow_keep(ss->raw, (size_t)stats->seed_hits, (size_t)(stats->seed_hits - hits), s, err));
    A.raw = ss->raw.p;
    for (int64_t h0 = 0; h0 < hits; h0 += kSearchLaunch) {
      A.h0 = (int)h0;
      A.nh = (int)std::min<int64_t>(kSearchLaunch, hits - h0);
      if (!raw) {
        hipLaunchKernelGGL(k_search_extend, dim3((unsigned)((A.nh + 255) / 256)), dim3(256), 0, s, A);
        MAP_TRY(hipGetLastError());
        continue;
      }
      unsigned long long ctr[2] = {0, 0};
      MAP_TRY(hipMemsetAsync(ss->ctr.p, 0, sizeof ctr, s));
      hipLaunchKernelGGL(k_search_extend, dim3((unsigned)((A.nh + 255) / 256)), dim3(256), 0, s, A);
      MAP_TRY(hipGetLastError());
      MAP_TRY(hipMemcpyAsync(ctr, ss->ctr.p, sizeof ctr, hipMemcpyDeviceToHost, s));
      MAP_TRY(hipStreamSynchronize(s));
      stats->skipped += (int64_t)ctr[1];
      const size_t had = raw->size(), got = (size_t)std::min<unsigned long long>(ctr[0], kSearchLaunch);
      raw->resize(had + got);
      if (got) MAP_TRY(hipMemcpy(raw->data() + had, ss->raw.p, got * sizeof(SearchRaw), hipMemcpyDeviceToHost));
    }
  }
  if (!raw) {
    unsigned long long ctr[2] = {0, 0};
    MAP_TRY(hipMemcpyAsync(ctr, ss->ctr.p, sizeof ctr, hipMemcpyDeviceToHost, s));
    MAP_TRY(hipStreamSynchronize(s));
    stats->skipped = (int64_t)ctr[1];
    *n_raw = (int64_t)std::min<unsigned long long>(ctr[0], (unsigned long long)stats->seed_hits);
  }
  return 0;
}

}  // namespace

ChunkView chunk_view(const SearchState& ss, int64_t total) {
  return ChunkView{{ss.pk[0].p, ss.pk[1].p}, {ss.nm[0].p, ss.nm[1].p}, ss.off.p, total};
}

int search_records(MapState* st, const ChunkSource& src, const int64_t* off, int64_t n_subjects, const SearchRule& rule,
                   std::vector<SearchRec>* recs_out, SearchStats* stats, hipStream_t s, std::string* err) {
  std::vector<SearchRec>& recs = *recs_out;
  recs.clear();
  *stats = SearchStats{0, 0, 0};
  st->search.resident = -1;
  if (n_subjects == 0 || st->n_kmers == 0) return 0;
  std::vector<SearchRaw> raw;
  const int rc = search_device(st, src, off, n_subjects, rule, &raw, nullptr, stats, s, err);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  stats->raw_hsps = (int64_t)raw.size();
  report_hsps_host(&raw, rule.min_score, &recs);
  return 0;
}

int search_records_device(MapState* st, const ChunkSource& src, const int64_t* off, int64_t n_subjects,
                          const SearchRule& rule, int64_t* n_recs, SearchStats* stats, hipStream_t s, std::string* err) {
  *n_recs = 0;
  *stats = SearchStats{0, 0, 0};
  st->search.resident = -1;
  if (n_subjects == 0 || st->n_kmers == 0) return 0;
  return synced_on_error(s, [&]() -> int {
    int64_t n_raw = 0;
    MAP_RC(search_device(st, src, off, n_subjects, rule, nullptr, &n_raw, stats, s, err));
    stats->raw_hsps = n_raw;
    // the bounds the host has: 2 x the chunk's subjects, the contigs, the store's and the chunk's
    // bases for the diagonal and the contig position, the longest subject
    int64_t longest = 0;
    for (int64_t g = 0; g < n_subjects; ++g) longest = std::max(longest, off[g + 1] - off[g]);
    RepBounds B{};
    B.hi[kRepSm] = 2 * n_subjects - 1;
    B.hi[kRepContig] = std::max(st->n_contigs - 1, 0);
    B.lo[kRepDelta] = -off[n_subjects];
    B.hi[kRepDelta] = st->total;
    B.hi[kRepB] = B.hi[kRepE] = B.hi[kRepLengthU] = longest;
    B.hi[kRepQstartU] = st->total;
    return report_hsps_device(&st->search.rep, st->search.raw.p, n_raw, rule.min_score, B, n_recs, s, err);
  });
}

int search_run(MapState* st, const ChunkSource& src, const int64_t* off, int64_t n_subjects, const SearchRule& rule,
               const SearchOut& out, int64_t* n, SearchStats* stats, hipStream_t s, std::string* err) {
  *n = 0;
  std::vector<SearchRec> recs;
  if (st->search.report_on) {                    // only the first `capacity` final records come back
    MAP_RC(search_records_device(st, src, off, n_subjects, rule, n, stats, s, err));
    recs.resize((size_t)std::min<int64_t>(*n, out.capacity));
    if (!recs.empty())
      MAP_TRY(hipMemcpy(recs.data(), st->search.rep.rec_sorted.p, recs.size() * sizeof(SearchRec), hipMemcpyDeviceToHost));
  } else {
    MAP_RC(search_records(st, src, off, n_subjects, rule, &recs, stats, s, err));
    *n = (int64_t)recs.size();
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

int64_t search_chunk_words(const MapState* st) {
  return !st || st->search.resident < 0 ? 0 : (st->search.resident + 31) / 32 + 2;
}

int search_chunk_planes(MapState* st, int strand, uint32_t* lo, uint32_t* hi, uint32_t* nn, hipStream_t s,
                        std::string* err) {
  const size_t words = (size_t)search_chunk_words(st);
  std::vector<uint2> pk(words);
  MAP_TRY(hipStreamSynchronize(s));
  MAP_TRY(hipMemcpy(pk.data(), st->search.pk[strand].p, sizeof(uint2) * words, hipMemcpyDeviceToHost));
  MAP_TRY(hipMemcpy(nn, st->search.nm[strand].p, sizeof(uint32_t) * words, hipMemcpyDeviceToHost));
  for (size_t w = 0; w < words; ++w) {
    lo[w] = pk[w].x;
    hi[w] = pk[w].y;
  }
  return 0;
}

}  // namespace wf
