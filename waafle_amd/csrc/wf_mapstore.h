// What the read mapper and the homology search share (wf_map.hip, wf_search.hip,
// wf_search_gap.hip, wf_dust.hip): the typed device array, the state a context keeps, the
// kernels' views of the contig store with its S-mer index and of a chunk of subjects, and the
// device helpers over them.  Declarations, structs and forced-inline device helpers only: each
// kernel and host function is defined in the one file named at its declaration.
#pragma once

#include <algorithm>
#include <string>
#include <vector>

#include "wf_internal.h"

namespace wf {

// Early return on a HIP error (-2, the call's text and HIP's message in *err) or on a non-zero
// code.  For use where `std::string* err` is in scope and the enclosing function returns int;
// inside a lambda (synced_on_error below) they return from the lambda, not from its function.
#define MAP_TRY(x)                                                                       \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) { *err = std::string(#x) + ": " + hipGetErrorString(e_); return -2; } \
  } while (0)
#define MAP_RC(x)                    \
  do {                               \
    const int rc_ = (x);             \
    if (rc_) return rc_;             \
  } while (0)

// An owning device array of T: grow-only (ensure keeps what is large enough and does not keep
// the contents otherwise), freed with its owner.
template <class T>
struct DevArr {
  T* p = nullptr;
  size_t n = 0;                // elements allocated
  DevArr() = default;
  DevArr(const DevArr&) = delete;
  DevArr& operator=(const DevArr&) = delete;
  ~DevArr() { if (p) (void)hipFree(p); }
  int ensure(size_t count, std::string* err) {
    if (p && n >= count) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);      // a count of 0 allocates too
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) {
      *err = "hipMalloc(" + std::to_string(bytes) + ") failed: " + hipGetErrorString(e);
      return -2;
    }
    p = static_cast<T*>(q);
    n = count;
    return 0;
  }
};

// f's return code; when it is an error, after the stream is idle.  A function whose local
// DevArrs kernels may still touch runs its body as f, so that an early return frees nothing
// under a kernel in flight.
template <class F>
int synced_on_error(hipStream_t s, F&& f) {
  const int rc = f();
  if (rc) (void)hipStreamSynchronize(s);
  return rc;
}

// ---- the homology search's records and staging (wf_search.hip, wf_search_gap.hip) --------

struct SearchRaw {            // one extended seed hit
  int32_t sm;                 // subject << 1 | minus
  int32_t contig;
  int32_t delta;              // contig position - variant position
  int32_t b, e;               // [b, e) on the variant
  int32_t score;
};
struct GapAnchor { int32_t sm, contig, i0, j0; };   // subject << 1 | minus; i0 on the variant, j0 contig-local
struct GapSide { int32_t H, p, q, g; };
struct GapRaw { GapSide left, right; };

struct SearchRec { int32_t contig, subject, minus, qstart, sstart, length, matches; };
struct GapAln {               // one gapped alignment
  int32_t sm, contig, qstart, qspan, sstart, sspan, length, matches, gaps;
  int64_t score2;
};

// the device form of the reporting step (wf_report.hip): grow-only
struct ReportState {
  DevArr<uint64_t> keys;       // [words][n] the composite sort keys
  DevArr<uint64_t> kin, kout;  // one sort's keys
  DevArr<uint64_t> val, run;   // a scan's input and output
  DevArr<int32_t> perm, spare; // the sorted order and its double buffer
  DevArr<int32_t> flag, first; // per sorted position: a flag; its group's first position
  DevArr<int64_t> box;         // [n][4] gapped: the two intervals of the alignment at a sorted position
  DevArr<SearchRec> rec, rec_sorted;
  DevArr<GapAln> aln, aln_kept, aln_sorted;
  DevArr<unsigned char> tmp;   // hipcub's scratch
};

struct SearchState {
  DevArr<unsigned char> seq, tmp;
  DevArr<int64_t> off, soff;
  DevArr<uint2> pk[2];
  DevArr<uint32_t> nm[2];
  DevArr<int32_t> cnt, first, start;
  DevArr<SearchRaw> raw;
  DevArr<unsigned long long> ctr;
  DevArr<GapAnchor> g_anchor;  // the gapped extension's anchors and results of one launch
  DevArr<GapRaw> g_out;
  DevArr<uint32_t> planes;     // a packed chunk as uploaded: lo, hi, nn, n_words each (k_search_unpack reads it)
  int64_t resident = -1;       // bases of the chunk whose planes pk, nm hold; -1: none
  int report_on = 0;           // WF_OPT_SEARCH_REPORT: 0 the reporting step on the host, 1 on the device
  ReportState rep;
};

struct MapState {
  // the index (kept between calls)
  DevArr<uint2> pk;
  DevArr<uint32_t> nm, bucket;
  DevArr<int32_t> coff, kpos;
  DevArr<uint64_t> keys;
  int n_contigs = 0, seed_len = 0, max_occ = 0, bshift = 0;
  int64_t total = 0, n_kmers = 0;
  bool have_index = false;
  // the low-complexity mask of the contigs (wf_dust.hip, wf_search_mask): one bit per store
  // position, laid out as nm.  have_mask: the index holds only the S-mers without a masked
  // base; map_index clears it.  n_kmers_plain: the S-mers of the index without a mask.
  DevArr<uint32_t> dm;
  bool have_mask = false;
  int64_t n_kmers_plain = 0;
  // read staging (host-resident calls)
  DevArr<char> s1, s2;
  DevArr<int64_t> o1, o2;
  DevArr<int32_t> r_contig, r_pos1, r_pos2;
  DevArr<uint8_t> r_strand, r_mm1, r_mm2;
  // the gapped pass: its result staging and the list of pairs to rescue
  DevArr<int8_t> r_d1, r_d2;
  DevArr<int16_t> r_k1, r_k2;
  DevArr<uint8_t> r_flags;
  DevArr<int32_t> g_flag, g_slot, g_idx;
  DevArr<unsigned char> g_tmp;
  // the homology search's staging, filled by its first call
  SearchState search;
};

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

// one chunk of subjects, resident in SearchState after search_records
struct ChunkView {
  const uint2* vpk[2];        // plus store, minus store (the reverse complement of the whole chunk)
  const uint32_t* vnm[2];
  const int64_t* off;         // [n_subjects + 1] the subjects' starts in the chunk
  int64_t total;              // bases of the chunk
};

// (wf_map.hip)
MapIndexView map_view(const MapState* st);
// seq[0, total) as bit planes of (total + 31) / 32 + 2 words, the padding N; rc: the reverse
// complement of the whole of seq.  Enqueued on s.
int map_pack(const unsigned char* seq, int64_t total, bool rc, uint2* pk, uint32_t* nm, hipStream_t s,
             std::string* err);
// scan_reserve: tmp (bytes) becomes the scratch of scan_total for up to n flags.  scan_total:
// slot = exclusive scan of flag[0, n), n > 0, with a tmp reserved for an n no smaller; *sum =
// the flags' total, after a synchronisation.  It allocates nothing.
int scan_reserve(DevArr<unsigned char>& tmp, int n, hipStream_t s, std::string* err);
int scan_total(const int32_t* flag, int32_t* slot, int n, const DevArr<unsigned char>& tmp, int64_t* sum,
               hipStream_t s, std::string* err);
// The S-mer index of the store the state holds, built anew: flag, scan, emit, sort, bucket.
// dm null: every S-mer without an N that stays in its contig; else only those whose S bases
// are all unmasked in dm.  Sets keys, kpos, bucket, bshift and n_kmers.
int map_build_index(MapState* st, const uint32_t* dm, hipStream_t s, std::string* err);

// (wf_search.hip)
ChunkView chunk_view(const SearchState& ss, int64_t total);
// The ungapped records of the chunk, sorted by (contig, subject, minus,
// qstart, sstart, length).  When any seed slot exists, the chunk's bit planes (pk, nm of both
// strands) and `off` stay resident in st->search afterwards (SearchState::resident), whichever
// form src gave the bases in.
int search_records(MapState* st, const ChunkSource& src, const int64_t* off, int64_t n_subjects, const SearchRule& rule,
                   std::vector<SearchRec>* recs, SearchStats* stats, hipStream_t s, std::string* err);

// ... with the reporting step on the device: the same records, *n_recs of
// them, in st->search.rep.rec_sorted; the raw HSPs never leave the device.
int search_records_device(MapState* st, const ChunkSource& src, const int64_t* off, int64_t n_subjects,
                          const SearchRule& rule, int64_t* n_recs, SearchStats* stats, hipStream_t s, std::string* err);

// (wf_search_gap.hip) the anchors [0, n) on the device extended into out[0, n), in launches of at
// most 2^16 with nothing between them; the chunk of `total` bases is resident.  Enqueued on s.
int gapped_launches(MapState* st, const GapAnchor* anchor, int64_t n, int band, int xdrop_gap, int64_t total,
                    GapRaw* out, hipStream_t s, std::string* err);

// ---- the reporting step (wf_report.hip) ---------------------
// host forms: what search_records and search_gapped_run always did.  raw is sorted in place.
void report_hsps_host(std::vector<SearchRaw>* raw, int min_score, std::vector<SearchRec>* recs);
void report_alns_host(const std::vector<GapAnchor>& anchors, const std::vector<GapRaw>& raw, int min_score,
                      std::vector<GapAln>* kept, int64_t* raw_alignments);
// device forms.  raw / anchor, graw: device arrays of n >= 0 elements.  The records come sorted
// in st->rep.rec_sorted / aln_sorted, *n_rec of them.  Returns after a synchronisation.
int report_hsps_device(ReportState* R, const SearchRaw* raw, int64_t n, int min_score, const RepBounds& B,
                       int64_t* n_rec, hipStream_t s, std::string* err);
int report_alns_device(ReportState* R, const GapAnchor* anchor, const GapRaw* graw, int64_t n, int min_score,
                       const RepBounds& B, int64_t* n_rec, int64_t* raw_alignments, hipStream_t s, std::string* err);
// anchor[i] of the record rec[i], i < n (device arrays); enqueued on s
int report_anchors(const SearchRec* rec, int64_t n, GapAnchor* anchor, hipStream_t s, std::string* err);
// a (device) holds `have` elements worth keeping: room for `count`, the contents kept
template <class T>
int grow_keep(DevArr<T>& a, size_t count, size_t have, hipStream_t s, std::string* err) {
  if (a.p && a.n >= count) return 0;
  DevArr<T> b;
  MAP_RC(b.ensure(std::max(count, 2 * a.n), err));
  if (have) {
    MAP_TRY(hipMemcpyAsync(b.p, a.p, have * sizeof(T), hipMemcpyDeviceToDevice, s));
    MAP_TRY(hipStreamSynchronize(s));                // the old array is freed below
  }
  std::swap(a.p, b.p);
  std::swap(a.n, b.n);
  return 0;
}
// ---- device helpers -----------------------------------------------------------------------

// A0 C1 G2 T3, anything else 4 (N); lower case counts as upper
__device__ __forceinline__ int base_code(unsigned char ch) {
  if (ch >= 'a' && ch <= 'z') ch -= 32;
  return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4;
}

// The bases src[0], src[step], ..., `count` <= 32 of them, as bit b of three planes, each
// complemented when comp: lo and hi are 0 where n (the base is an N) is set, all three past count.
struct Planes32 { uint32_t lo, hi, n; };
__device__ __forceinline__ Planes32 pack32(const unsigned char* src, int step, int count, bool comp) {
  uint32_t lo = 0, hi = 0, n = 0;
  for (int b = 0; b < count; ++b) {
    int code = base_code(src[b * step]);
    if (comp && code < 4) code = 3 - code;
    lo |= (uint32_t)(code & 1) << b;
    hi |= (uint32_t)((code >> 1) & 1) << b;
    n |= (uint32_t)(code >> 2) << b;
  }
  return Planes32{lo & ~n, hi & ~n, n};
}

__device__ __forceinline__ uint32_t smer_mask(int S) { return S == 32 ? 0xFFFFFFFFu : (1u << S) - 1u; }

// bits [sh, sh + 32) of the 64-bit value hi:lo
__device__ __forceinline__ uint32_t window32(uint32_t lo, uint32_t hi, int sh) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
}
// the 32 bits of plane p from position q >= 0 on (words q / 32 and q / 32 + 1)
__device__ __forceinline__ uint32_t plane_window(const uint32_t* p, int q) {
  return window32(p[q >> 5], p[(q >> 5) + 1], q & 31);
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

// the S-mer at position q >= 0 of the planes pk, nm: false when it holds an N
__device__ __forceinline__ bool planes_kmer(const uint2* pk, const uint32_t* nm, int S, int q, uint64_t* key) {
  const int W = q >> 5, sh = q & 31;
  const uint32_t mask = smer_mask(S);
  if (plane_window(nm, q) & mask) return false;
  const uint2 a = pk[W], b = pk[W + 1];
  *key = ((uint64_t)(window32(a.y, b.y, sh) & mask) << S) | (window32(a.x, b.x, sh) & mask);
  return true;
}

// the first entry of the sorted index whose key is >= key, within key's bucket [.., *end)
__device__ __forceinline__ int index_lower_bound(const MapIndexView& ix, uint64_t key, int* end) {
  const uint32_t b = (uint32_t)(key >> ix.bshift);
  int lo = (int)ix.bucket[b], hi = (int)ix.bucket[b + 1];
  *end = hi;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ix.keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
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

// subject g of the chunk on `strand`: its length and its start in that strand's store
__device__ __forceinline__ void chunk_place(const ChunkView& C, int g, int strand, int* M, int* vbase) {
  const int64_t o0 = C.off[g], o1 = C.off[g + 1];
  *M = (int)(o1 - o0);
  *vbase = (int)(strand ? C.total - o1 : o0);
}

// mismatch bits of the 32 columns whose first lies at position vp of the chunk's store of
// `strand` and gp of the contig store; either may be as low as -32 (the bases before a store
// are N)
__device__ __forceinline__ uint32_t chunk_mis(const MapIndexView& ix, const ChunkView& C, int strand, int vp,
                                              int gp) {
  const uint2* pk = C.vpk[strand];
  const uint32_t* nm = C.vnm[strand];
  const int W = vp >> 5, sh = vp & 31;
  uint2 a = make_uint2(0u, 0u);
  uint32_t na = ~0u;
  if (W >= 0) {
    a = pk[W];
    na = nm[W];
  }
  const uint2 b = pk[W + 1];
  const uint32_t vlo = window32(a.x, b.x, sh), vhi = window32(a.y, b.y, sh), vn = window32(na, nm[W + 1], sh);
  return map_mis_word<true>(ix, &vlo, &vhi, &vn, 0, gp);
}

}  // namespace wf
