// Paired-read mapper on MI355X (gfx950, wave64): a deterministic seed-and-verify ungapped
// mapper for waafle_junctions' read input (DESIGN.md §11 states the rule; tests/map_oracle.py
// restates it on the CPU).  Not a bowtie2 clone: no gaps, no clipping, no MAPQ.
//
// Index (map_index):
//   k_map_pack    thread per 32 bases: the contig store as two bit planes in one 64-bit word
//                 (x: low bit, y: high bit of the base code A0 C1 G2 T3) and a 1-bit N plane;
//                 the store is padded so the window read of words w and w + 1 stays in bounds
//                 (map_pack; the homology search packs its chunks with it, in both orientations)
//   k_map_flag    thread per position: 1 when the S-mer there has no N and stays in its contig
//                 and, given the low-complexity mask (wf_dust.hip), holds no masked base
//   k_map_emit    (device scan of the flags) -> compact (key, position) pairs, position order;
//                 key = high-plane bits << S | low-plane bits
//   device radix sort on the 2S key bits (stable: equal keys keep ascending positions)
//   k_map_bucket  direct-address table over the key's top bits: bucket[b] = first sorted
//                 entry whose prefix is >= b, so a lookup is one table read plus a search
//                 among the few entries that share the prefix
// Mapping (k_map_pairs): one wave per read pair, one wave per workgroup.
//   lanes = 2 mates x 2 strands x 16 words: pack the four read variants into LDS
//   lanes = 2 mates x 2 strands x 16 seed slots: look the seed up, expand its occurrences
//     into the candidate list (global start = occurrence - seed offset); a lane owns max_occ
//     slots, so the list holds 64 * max_occ entries and cannot overflow
//   candidates are de-duplicated per variant; a start whose read would leave its contig is
//     dropped before anything is loaded from the store
//   (candidate, 32-base word) tasks over the lanes: window of the store by a funnel shift,
//     mismatches = popcount((x ^ r) low | (x ^ r) high | N), summed per candidate in LDS
//   (mate-1 hit, mate-2 hit) tasks over the lanes: the concordant pair of least key, by a
//     wave-wide minimum of the two key words
// Single-gap rescue (map_pairs_gapped, max_gap > 0; DESIGN.md §11.1 "gapped pass"):
//   k_map_gap_flag / scan / k_map_gap_list  the pairs k_map_pairs left unaligned whose mates
//     are both at least S long, compacted on the device
//   k_map_gap     one wave per listed pair, in launches of at most kMapGapLaunch pairs: the
//     same planes and seed look-ups; the candidates are now diagonals (start, contig of the
//     seed occurrence, the set of seed slots that hit it), kept even where the ungapped read
//     would leave its contig; one (diagonal, d, side) task per lane forms the mismatch words of
//     the left and the right diagonal and walks the split point k over prefix + suffix
//     popcounts; the hits (at most 256 per mate) are collected in LDS and the concordant
//     pair of least key is again a wave-wide minimum
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "wf_internal.h"
#include "wf_lanes.h"
#include "wf_mapstore.h"   // the shared layer: DevArr, MapState, MapIndexView, the device helpers

namespace wf {

namespace {

constexpr int kMapMaxRead = 512;        // bases per mate
constexpr int kMapSlots = 16;           // seed slots per (mate, strand)
constexpr int kMapWords = kMapMaxRead / 32;
constexpr int kMapRow = kMapWords + 1;  // + a zero word: the seed window reads word w + 1
constexpr int kMapFixedLds = (3 * 4 * kMapRow + 8) * 4 + 2 * kMapMaxRead;

struct MapPairArgs {
  MapIndexView ix;
  int max_occ, max_mm;
  int64_t min_ins, max_ins, n_pairs;
  const char* s1; const int64_t* o1; const char* s2; const int64_t* o2;
  int32_t* contig; int32_t* pos1; int32_t* pos2; uint8_t* strand1; uint8_t* mm1; uint8_t* mm2;
};

// thread per word of the planes; rc: word w holds seq[total - 1 - 32 w] downwards, complemented
__global__ void k_map_pack(const unsigned char* seq, int64_t total, int64_t words, bool rc, uint2* pk, uint32_t* nm) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= words) return;
  const int count = (int)std::min<int64_t>(std::max<int64_t>(total - w * 32, 0), 32);
  const Planes32 v = pack32(rc ? seq + (total - 1 - w * 32) : seq + w * 32, rc ? -1 : 1, count, rc);
  pk[w] = make_uint2(v.lo, v.hi);
  nm[w] = v.n | (count < 32 ? ~0u << count : 0u);            // the padding is N
}

// dm null: the flags of the plain index; else the S bases must be unmasked in dm too.  The
// windows are read before the contig is known (q < n_pos: inside the planes either way), so
// that neither the loads nor the test of dm wait for the search of coff.
__global__ void k_map_flag(const MapIndexView ix, const uint32_t* dm, int n_pos, int32_t* flag) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_pos) return;
  uint32_t bad = plane_window(ix.nm, q);                     // an N among the 32 bases from q on,
  if (dm) bad |= plane_window(dm, q);                        //   or a masked base
  const int c = contig_of(ix.coff, ix.n_contigs, q);
  flag[q] = (int64_t)q + ix.S <= ix.coff[c + 1] && (bad & smer_mask(ix.S)) == 0;
}

__global__ void k_map_emit(const MapIndexView ix, int n_pos, const int32_t* flag, const int32_t* slot,
                           uint64_t* keys, int32_t* kpos) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_pos || !flag[q]) return;
  uint64_t key = 0;
  planes_kmer(ix.pk, ix.nm, ix.S, q, &key);
  keys[slot[q]] = key;
  kpos[slot[q]] = q;
}

// thread i <= n: the buckets in (prefix of entry i - 1, prefix of entry i] start at i; thread
// n closes the table, so each of the n_buckets + 1 entries is written exactly once
__global__ void k_map_bucket(const uint64_t* keys, int n, int shift, uint32_t n_buckets, uint32_t* bucket) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  const int64_t cur = i < n ? (int64_t)(keys[i] >> shift) : (int64_t)n_buckets;
  const int64_t prev = i > 0 ? (int64_t)(keys[i - 1] >> shift) : -1;
  for (int64_t b = prev + 1; b <= cur; ++b) bucket[b] = (uint32_t)i;
}

__device__ __forceinline__ void map_unaligned(const MapPairArgs& A, int64_t pr) {
  A.contig[pr] = -1;
  A.pos1[pr] = 0;
  A.pos2[pr] = 0;
  A.strand1[pr] = 0;
  A.mm1[pr] = 0;
  A.mm2[pr] = 0;
}

// lane = variant * 16 + word: the read as given (strand 0) and reverse-complemented (1) as
// bit planes in LDS, each row closed by a zero word; asc holds the two mates' ASCII bases
__device__ __forceinline__ void map_pack_variants(const unsigned char* asc, int L1, int L2, int lane,
                                                  uint32_t* xlo, uint32_t* xhi, uint32_t* xnn) {
  const int v = lane >> 4, slot = lane & 15;
  const int Lv = (v >> 1) ? L2 : L1;
  const unsigned char* src = asc + (v >> 1) * kMapMaxRead;
  const bool rc = v & 1;
  const Planes32 x = pack32(rc ? src + (Lv - 1 - slot * 32) : src + slot * 32, rc ? -1 : 1,
                            min(max(Lv - slot * 32, 0), 32), rc);
  xlo[v * kMapRow + slot] = x.lo;
  xhi[v * kMapRow + slot] = x.hi;
  xnn[v * kMapRow + slot] = x.n;
  if (slot == 0) {
    xlo[v * kMapRow + kMapWords] = 0;
    xhi[v * kMapRow + kMapWords] = 0;
    xnn[v * kMapRow + kMapWords] = 0;
  }
}

// seed slot `slot` of variant v: the number of its occurrences and the first of them in the
// sorted index (none when the slot is past the read, the seed holds an N, is absent, or
// occurs more than max_occ times)
__device__ __forceinline__ int map_seed_lookup(const MapIndexView& ix, int max_occ, const uint32_t* xlo,
                                               const uint32_t* xhi, const uint32_t* xnn, int v, int slot,
                                               int Lv, int* first) {
  const int S = ix.S;
  const int off = slot * S;
  int cnt = 0;
  if (slot < min(Lv / S, kMapSlots)) {
    const uint32_t mask = smer_mask(S);
    if ((plane_window(xnn + v * kMapRow, off) & mask) == 0) {
      const uint64_t key = ((uint64_t)(plane_window(xhi + v * kMapRow, off) & mask) << S) |
                           (plane_window(xlo + v * kMapRow, off) & mask);
      int end;
      const int lo = index_lower_bound(ix, key, &end);
      *first = lo;
      while (cnt <= max_occ && lo + cnt < end && ix.keys[lo + cnt] == key) ++cnt;
      if (cnt > max_occ) cnt = 0;
    }
  }
  return cnt;
}

__global__ __launch_bounds__(64) void k_map_pairs(const MapPairArgs A) {
  extern __shared__ __align__(16) unsigned char map_lds[];
  const int lane = threadIdx.x;
  const int64_t pr = blockIdx.x;
  const MapIndexView& ix = A.ix;
  const int S = ix.S;
  const int cap = 64 * A.max_occ;
  uint32_t* xlo = reinterpret_cast<uint32_t*>(map_lds);      // [4][kMapRow] variant m * 2 + s
  uint32_t* xhi = xlo + 4 * kMapRow;
  uint32_t* xnn = xhi + 4 * kMapRow;
  int* vst = reinterpret_cast<int*>(xnn + 4 * kMapRow);      // [4] first candidate of a variant
  int* ctr = vst + 4;                                        // [0] surviving candidates
  int* list = ctr + 4;                                       // [cap] candidate starts
  int* ug = list + cap;                                      // [cap] survivors: start,
  int* uc = ug + cap;                                        //   contig,
  uint32_t* um = reinterpret_cast<uint32_t*>(uc + cap);      //   variant << 16 | mismatches
  unsigned char* asc = reinterpret_cast<unsigned char*>(um + cap);   // [2][kMapMaxRead]

  const int64_t b1 = A.o1[pr], b2 = A.o2[pr];
  const int64_t l1 = A.o1[pr + 1] - b1, l2 = A.o2[pr + 1] - b2;
  if (l1 < S || l2 < S || l1 > kMapMaxRead || l2 > kMapMaxRead) {   // (the host refuses > 512)
    if (lane == 0) map_unaligned(A, pr);
    return;
  }
  const int L1 = (int)l1, L2 = (int)l2;
  for (int i = lane; i < L1; i += 64) asc[i] = (unsigned char)A.s1[b1 + i];
  for (int i = lane; i < L2; i += 64) asc[kMapMaxRead + i] = (unsigned char)A.s2[b2 + i];
  if (lane == 0) ctr[0] = 0;
  __syncthreads();

  // lane = variant * 16 + word: the read as given (strand 0) and reverse-complemented (1)
  const int v = lane >> 4, slot = lane & 15;
  const int Lv = (v >> 1) ? L2 : L1;
  map_pack_variants(asc, L1, L2, lane, xlo, xhi, xnn);
  __syncthreads();

  // lane = variant * 16 + seed slot: the seed's occurrences (none when it holds an N, is
  // absent, or occurs more than max_occ times)
  int first = 0;
  const int off = slot * S;
  const int cnt = map_seed_lookup(ix, A.max_occ, xlo, xhi, xnn, v, slot, Lv, &first);
  int n_cand;
  const int start = wave_excl_scan_dpp(cnt, &n_cand);
  if (slot == 0) vst[v] = start;
  for (int k = 0; k < cnt; ++k) list[start + k] = ix.kpos[first + k] - off;
  __syncthreads();

  // de-duplicate per variant (the first copy stays) and drop what leaves its contig
  for (int e = lane; e < n_cand; e += 64) {
    const int g = list[e];
    const int ev = (e >= vst[1]) + (e >= vst[2]) + (e >= vst[3]);
    bool dup = false;
    for (int k = vst[ev]; k < e && !dup; ++k) dup = list[k] == g;
    if (dup || g < 0) continue;
    const int c = contig_of(ix.coff, ix.n_contigs, g);
    if ((int64_t)g + ((ev >> 1) ? L2 : L1) > ix.coff[c + 1]) continue;
    const int u = atomicAdd(&ctr[0], 1);
    ug[u] = g;
    uc[u] = c;
    um[u] = (uint32_t)ev << 16;
  }
  __syncthreads();
  const int U = ctr[0];

  // mismatches: one (candidate, word) task per lane and turn
  const int nw = (max(L1, L2) + 31) >> 5;
  for (int t = lane; t < U * nw; t += 64) {
    const int u = t / nw, w = t - u * nw;
    const int uv = (int)(um[u] >> 16);
    const int rem = ((uv >> 1) ? L2 : L1) - 32 * w;
    if (rem <= 0) continue;
    const int gg = ug[u] + 32 * w;                           // < the contig's end <= total
    uint32_t mis = map_mis_word<false>(ix, xlo, xhi, xnn, uv * kMapRow + w, gg);
    if (rem < 32) mis &= (1u << rem) - 1u;
    if (mis) atomicAdd(&um[u], (uint32_t)__popc(mis));
  }
  __syncthreads();

  // the concordant pair of least (mm1 + mm2, contig, f.p, fragment, strand of mate 1): contig
  // and f.p order as the + mate's store position does
  uint64_t khi = ~0ull, klo = ~0ull;
  int wa = 0, wb = 0;
  for (int t = lane; t < U * U; t += 64) {
    const int a = t / U, b = t - a * U;
    const uint32_t ma = um[a], mb = um[b];
    const int va = (int)(ma >> 16), vb = (int)(mb >> 16);
    if ((va >> 1) != 0 || (vb >> 1) != 1 || ((va ^ vb) & 1) == 0) continue;
    const int mma = (int)(ma & 0xFFFFu), mmb = (int)(mb & 0xFFFFu);
    if (mma > A.max_mm || mmb > A.max_mm || uc[a] != uc[b]) continue;
    const bool afirst = (va & 1) == 0;                       // mate 1 is the + mate
    const int64_t gf = afirst ? ug[a] : ug[b], gr = afirst ? ug[b] : ug[a];
    const int64_t ef = gf + (afirst ? L1 : L2), er = gr + (afirst ? L2 : L1);
    if (gf > gr || ef > er) continue;                        // dovetail
    const int64_t frag = er - gf;
    if (frag < A.min_ins || frag > A.max_ins) continue;
    const uint64_t h = ((uint64_t)(mma + mmb) << 32) | (uint64_t)gf;
    const uint64_t l = ((uint64_t)frag << 1) | (uint64_t)(va & 1);
    if (h < khi || (h == khi && l < klo)) { khi = h; klo = l; wa = a; wb = b; }
  }
  const uint64_t bhi = wave_butterfly(khi, [](uint64_t x, uint64_t y) { return x < y ? x : y; });
  const uint64_t mlo = khi == bhi ? klo : ~0ull;
  const uint64_t blo = wave_butterfly(mlo, [](uint64_t x, uint64_t y) { return x < y ? x : y; });
  if (bhi == ~0ull) {
    if (lane == 0) map_unaligned(A, pr);
    return;
  }
  if (khi == bhi && klo == blo) {                            // the key is unique: one lane
    const int c = uc[wa];
    A.contig[pr] = c;
    A.pos1[pr] = ug[wa] - ix.coff[c] + 1;
    A.pos2[pr] = ug[wb] - ix.coff[c] + 1;
    A.strand1[pr] = (uint8_t)((um[wa] >> 16) & 1);
    A.mm1[pr] = (uint8_t)(um[wa] & 0xFFFFu);
    A.mm2[pr] = (uint8_t)(um[wb] & 0xFFFFu);
  }
}

// ---- the single-gap rescue ------------------------------------------------------------

constexpr int kMapGapMax = 8;           // max_gap
constexpr int kMapGapHits = 256;        // hits per mate
constexpr int kMapGapLaunch = 1 << 16;  // pairs per k_map_gap launch
// LDS: planes, counters, the two hit lists and the ASCII reads, plus 21 bytes per entry of
// the candidate list (64 * max_occ entries)
constexpr int kMapGapFixedLds = (3 * 4 * kMapRow + 16) * 4 + 2 * kMapGapHits * 12 + 2 * kMapMaxRead;
constexpr int kMapGapEntryLds = 21;
static_assert(kMapGapMax + 8 < 32 && kMapGapMax < 32, "d + 8 is packed in 5 bits; loads reach max_gap past a contig");

struct MapGapArgs {
  MapPairArgs P;              // the index, the rule, the reads and the six result arrays
  int max_gap, n;             // n: pairs of this launch
  const int32_t* idx;         // [n] their pair numbers
  int8_t* d1; int8_t* d2; int16_t* k1; int16_t* k2; uint8_t* flags;
};

__global__ void k_map_gap_flag(const MapPairArgs A, int32_t* flag) {
  const int64_t pr = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pr >= A.n_pairs) return;
  flag[pr] = A.contig[pr] < 0 && A.o1[pr + 1] - A.o1[pr] >= A.ix.S && A.o2[pr + 1] - A.o2[pr] >= A.ix.S;
}

__global__ void k_map_gap_list(int64_t n, const int32_t* flag, const int32_t* slot, int32_t* idx) {
  const int64_t pr = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pr < n && flag[pr]) idx[slot[pr]] = (int32_t)pr;
}

// one diagonal of one variant: read index i against store position g0 + i
struct MapDiag {
  const MapIndexView& ix;
  const uint32_t *xlo, *xhi, *xnn;
  int row, L, g0;
  // mismatch bits of read word w (bits at and past L are 0)
  __device__ __forceinline__ uint32_t word(int w) const {
    uint32_t mis = map_mis_word<true>(ix, xlo, xhi, xnn, row + w, g0 + 32 * w);
    const int rem = L - 32 * w;
    if (rem < 32) mis &= (1u << rem) - 1u;
    return mis;
  }
  // mismatches among read indices [0, j), j <= L
  __device__ __forceinline__ int prefix(int j) const {
    int n = 0;
    for (int w = 0; w < (j >> 5); ++w) n += __popc(word(w));
    if (j & 31) n += __popc(word(j >> 5) & ((1u << (j & 31)) - 1u));
    return n;
  }
};

// One wave per listed pair.  Every store load is a word W or W + 1 of a position in
// [p - max_gap, p + L + max_gap) with coff[c] <= p and p + L + d <= coff[c + 1]: W >= -1
// (guarded) and W + 1 <= ceil(total / 32) + 1, the last padded word, since max_gap < 32.
__global__ __launch_bounds__(64) void k_map_gap(const MapGapArgs G) {
  extern __shared__ __align__(16) unsigned char map_lds[];
  const MapPairArgs& A = G.P;
  const int lane = threadIdx.x;
  const int64_t pr = G.idx[blockIdx.x];
  const MapIndexView& ix = A.ix;
  const int S = ix.S;
  const int cap = 64 * A.max_occ;
  uint32_t* xlo = reinterpret_cast<uint32_t*>(map_lds);      // [4][kMapRow] variant m * 2 + s
  uint32_t* xhi = xlo + 4 * kMapRow;
  uint32_t* xnn = xhi + 4 * kMapRow;
  int* vst = reinterpret_cast<int*>(xnn + 4 * kMapRow);      // [5] first entry of a variant, end
  int* ctr = vst + 8;                                        // [0] diagonals, [1 + m] hits of mate m
  int* hg = ctr + 8;                                         // [2][kMapGapHits] hits: start,
  int* hc = hg + 2 * kMapGapHits;                            //   contig,
  uint32_t* hw = reinterpret_cast<uint32_t*>(hc + 2 * kMapGapHits);  // strand, d + 8, k, mm
  int* list = reinterpret_cast<int*>(hw + 2 * kMapGapHits);  // [cap] seed hits: diagonal,
  int* lcon = list + cap;                                    //   contig of the occurrence
  int* ug = lcon + cap;                                      // [cap] distinct diagonals: start,
  int* uc = ug + cap;                                        //   contig,
  uint32_t* um = reinterpret_cast<uint32_t*>(uc + cap);      //   variant << 16 | seed slots
  unsigned char* asc = reinterpret_cast<unsigned char*>(um + cap);   // [2][kMapMaxRead]
  unsigned char* lln = asc + 2 * kMapMaxRead;                // [cap] seed hits: the lane

  const int64_t b1 = A.o1[pr], b2 = A.o2[pr];
  const int L1 = (int)(A.o1[pr + 1] - b1), L2 = (int)(A.o2[pr + 1] - b2);   // S..512: listed
  for (int i = lane; i < L1; i += 64) asc[i] = (unsigned char)A.s1[b1 + i];
  for (int i = lane; i < L2; i += 64) asc[kMapMaxRead + i] = (unsigned char)A.s2[b2 + i];
  if (lane < 3) ctr[lane] = 0;
  __syncthreads();
  const int v = lane >> 4, slot = lane & 15;
  const int Lv = (v >> 1) ? L2 : L1;
  map_pack_variants(asc, L1, L2, lane, xlo, xhi, xnn);
  __syncthreads();

  // lane = variant * 16 + seed slot: every occurrence with its diagonal and its own contig
  int first = 0;
  const int off = slot * S;
  const int cnt = map_seed_lookup(ix, A.max_occ, xlo, xhi, xnn, v, slot, Lv, &first);
  int n_cand;
  const int start = wave_excl_scan_dpp(cnt, &n_cand);
  if (slot == 0) vst[v] = start;
  if (lane == 0) vst[4] = n_cand;
  for (int k = 0; k < cnt; ++k) {
    const int q = ix.kpos[first + k];
    list[start + k] = q - off;
    lcon[start + k] = contig_of(ix.coff, ix.n_contigs, q);
    lln[start + k] = (unsigned char)lane;
  }
  __syncthreads();

  // distinct (variant, diagonal, contig), each with the seed slots that hit it; nothing is
  // dropped here: a diagonal that leaves its contig can still be one side of a gap
  for (int e = lane; e < n_cand; e += 64) {
    const int g = list[e], c = lcon[e];
    const int ev = lln[e] >> 4;
    bool dup = false;
    uint32_t slots = 0;
    for (int k = vst[ev]; k < vst[ev + 1] && !dup; ++k) {
      if (list[k] != g || lcon[k] != c) continue;
      dup = k < e;
      slots |= 1u << (lln[k] & 15);
    }
    if (dup) continue;
    const int u = atomicAdd(&ctr[0], 1);
    ug[u] = g;
    uc[u] = c;
    um[u] = (uint32_t)ev << 16 | slots;
  }
  __syncthreads();
  const int U = ctr[0];

  // one (diagonal u, d, side) task per lane and turn.  Side 0: u is the left diagonal, the
  // alignment starts at p = ug[u]; side 1: u is the right diagonal, p = ug[u] - d, and the
  // task is left to side 0 of the diagonal at p when that one is listed (counted once).
  const int nd = 2 * G.max_gap + 1;
  for (int t = lane; t < U * 2 * nd; t += 64) {
    const int u = t / (2 * nd), r = t - u * 2 * nd;
    const int side = r >= nd;
    const int d = r - side * nd - G.max_gap;
    if (d == 0 && side) continue;
    const uint32_t mu = um[u];
    const int uv = (int)(mu >> 16), c = uc[u];
    const int L = (uv >> 1) ? L2 : L1;
    const int gap = d < 0 ? -d : 0;
    const int klo = S, khi = L - S - gap;                    // both segments >= S
    if (d != 0 && khi < klo) continue;
    const int p = side ? ug[u] - d : ug[u];
    if (p < ix.coff[c] || p + L + d > ix.coff[c + 1]) continue;
    uint32_t sl = side ? 0u : (mu & 0xFFFFu), sr = side ? (mu & 0xFFFFu) : 0u;
    if (d != 0) {                                            // the other diagonal's seed slots
      const int og = side ? p : p + d;
      uint32_t other = 0;
      bool found = false;
      for (int j = 0; j < U && !found; ++j)
        if (ug[j] == og && uc[j] == c && (int)(um[j] >> 16) == uv) { found = true; other = um[j] & 0xFFFFu; }
      if (side && found) continue;
      if (!side) sr = other;
    }
    const MapDiag dl{ix, xlo, xhi, xnn, uv * kMapRow, L, p};
    int best = 1 << 20, bk = 0;
    if (d == 0) {
      best = dl.prefix(L);
    } else {
      // seeded k: a left seed slot j needs (j + 1) S <= k, a right one j S >= k + gap, so
      // the seeded k are [kl, khi] united with [klo, kr]
      const int kl = sl ? (__ffs((int)sl) - 1) * S + S : (1 << 20);
      const int kr = sr ? (31 - __clz((int)sr)) * S - gap : -1;
      if (kl > khi && kr < klo) continue;
      const MapDiag dr{ix, xlo, xhi, xnn, uv * kMapRow, L, p + d};
      const int tr = dr.prefix(L);
      int pl = dl.prefix(klo), pj = dr.prefix(klo + gap);
      uint32_t wl = dl.word(klo >> 5), wr = dr.word((klo + gap) >> 5);
      for (int k = klo;; ++k) {
        const int mm = pl + tr - pj;
        if ((k >= kl || k <= kr) && mm < best) { best = mm; bk = k; }   // the least k stays
        if (k == khi) break;
        const int j = k + gap;
        pl += (int)((wl >> (k & 31)) & 1u);
        pj += (int)((wr >> (j & 31)) & 1u);
        if (((k + 1) & 31) == 0) wl = dl.word((k + 1) >> 5);
        if (((j + 1) & 31) == 0) wr = dr.word((j + 1) >> 5);
      }
    }
    if (best > A.max_mm) continue;
    const int m = uv >> 1;
    const int h = atomicAdd(&ctr[1 + m], 1);
    if (h >= kMapGapHits) continue;
    hg[m * kMapGapHits + h] = p;
    hc[m * kMapGapHits + h] = c;
    hw[m * kMapGapHits + h] = (uint32_t)(uv & 1) << 24 | (uint32_t)(d + 8) << 16 | (uint32_t)bk << 6 | (uint32_t)best;
  }
  __syncthreads();
  const int n1 = ctr[1], n2 = ctr[2];
  if (n1 > kMapGapHits || n2 > kMapGapHits) {                // the pair stays unaligned
    if (lane == 0) G.flags[pr] = 2;
    return;
  }

  // the concordant pair of least (nm1 + nm2, |d1| + |d2|, contig, f.p, fragment, strand of
  // mate 1, d1, d2)
  uint64_t khi = ~0ull, klo = ~0ull;
  int wa = 0, wb = 0;
  for (int t = lane; t < n1 * n2; t += 64) {
    const int a = t / n2, b = kMapGapHits + t - a * n2;
    const uint32_t ha = hw[a], hb = hw[b];
    if (((ha ^ hb) >> 24) == 0 || hc[a] != hc[b]) continue;
    const int da = (int)((ha >> 16) & 31u) - 8, db = (int)((hb >> 16) & 31u) - 8;
    const bool afirst = (ha >> 24) == 0;                     // mate 1 is the + mate
    const int64_t gf = afirst ? hg[a] : hg[b], gr = afirst ? hg[b] : hg[a];
    const int64_t ef = gf + (afirst ? L1 + da : L2 + db), er = gr + (afirst ? L2 + db : L1 + da);
    if (gf > gr || ef > er) continue;                        // dovetail
    const int64_t frag = er - gf;
    if (frag < A.min_ins || frag > A.max_ins) continue;
    const int ad = (da < 0 ? -da : da) + (db < 0 ? -db : db);
    const int nm = (int)(ha & 63u) + (int)(hb & 63u) + ad;
    const uint64_t h = ((uint64_t)nm << 40) | ((uint64_t)ad << 32) | (uint64_t)gf;
    const uint64_t l = ((uint64_t)frag << 11) | (uint64_t)(ha >> 24) << 10 | (uint64_t)(da + 8) << 5 |
                       (uint64_t)(db + 8);
    if (h < khi || (h == khi && l < klo)) { khi = h; klo = l; wa = a; wb = b; }
  }
  const uint64_t bhi = wave_butterfly(khi, [](uint64_t x, uint64_t y) { return x < y ? x : y; });
  const uint64_t mlo = khi == bhi ? klo : ~0ull;
  const uint64_t blo = wave_butterfly(mlo, [](uint64_t x, uint64_t y) { return x < y ? x : y; });
  if (bhi == ~0ull) return;                                  // unaligned, as k_map_pairs left it
  if (khi == bhi && klo == blo) {                            // the key is unique: one lane
    const int c = hc[wa];
    const uint32_t ha = hw[wa], hb = hw[wb];
    A.contig[pr] = c;
    A.pos1[pr] = hg[wa] - ix.coff[c] + 1;
    A.pos2[pr] = hg[wb] - ix.coff[c] + 1;
    A.strand1[pr] = (uint8_t)(ha >> 24);
    A.mm1[pr] = (uint8_t)(ha & 63u);
    A.mm2[pr] = (uint8_t)(hb & 63u);
    G.d1[pr] = (int8_t)((int)((ha >> 16) & 31u) - 8);
    G.d2[pr] = (int8_t)((int)((hb >> 16) & 31u) - 8);
    G.k1[pr] = (int16_t)((ha >> 6) & 1023u);
    G.k2[pr] = (int16_t)((hb >> 6) & 1023u);
    G.flags[pr] = 1;
  }
}

// The gapped pass over the results k_map_pairs has written: list the pairs to rescue on the
// device, then k_map_gap in launches of at most kMapGapLaunch pairs.
int map_rescue(MapState* st, MapGapArgs GA, hipStream_t s, std::string* err) {
  const int64_t NP = GA.P.n_pairs;
  const unsigned blocks = (unsigned)((NP + 255) / 256);
  const size_t lds = (size_t)kMapGapFixedLds + (size_t)kMapGapEntryLds * 64 * (size_t)GA.P.max_occ;
  MAP_RC(st->g_flag.ensure(NP, err));
  MAP_RC(st->g_slot.ensure(NP, err));
  MAP_RC(st->g_idx.ensure(NP, err));
  hipLaunchKernelGGL(k_map_gap_flag, dim3(blocks), dim3(256), 0, s, GA.P, st->g_flag.p);
  MAP_TRY(hipGetLastError());
  int64_t n = 0;
  MAP_RC(scan_reserve(st->g_tmp, (int)NP, s, err));
  MAP_RC(scan_total(st->g_flag.p, st->g_slot.p, (int)NP, st->g_tmp, &n, s, err));
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_map_gap_list, dim3(blocks), dim3(256), 0, s, NP, st->g_flag.p, st->g_slot.p, st->g_idx.p);
  MAP_TRY(hipGetLastError());
  MAP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_map_gap),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (int64_t lo = 0; lo < n; lo += kMapGapLaunch) {
    GA.n = (int)std::min<int64_t>(kMapGapLaunch, n - lo);
    GA.idx = st->g_idx.p + lo;
    hipLaunchKernelGGL(k_map_gap, dim3((unsigned)GA.n), dim3(64), lds, s, GA);
    MAP_TRY(hipGetLastError());
  }
  return 0;
}

}  // namespace

MapState* map_create() { return new MapState(); }

void map_destroy(MapState* st) { delete st; }

int map_index_params(const MapState* st, int* seed_len, int* max_occ) {
  if (!st || !st->have_index) return 0;
  *seed_len = st->seed_len;
  *max_occ = st->max_occ;
  return 1;
}

MapIndexView map_view(const MapState* st) {
  return MapIndexView{st->pk.p, st->nm.p, st->coff.p, st->keys.p, st->kpos.p, st->bucket.p,
                      st->n_contigs, st->seed_len, st->bshift, st->have_mask ? st->dm.p : nullptr};
}

int map_pack(const unsigned char* seq, int64_t total, bool rc, uint2* pk, uint32_t* nm, hipStream_t s,
             std::string* err) {
  const int64_t words = (total + 31) / 32 + 2;
  hipLaunchKernelGGL(k_map_pack, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, seq, total, words, rc, pk, nm);
  MAP_TRY(hipGetLastError());
  return 0;
}

int scan_reserve(DevArr<unsigned char>& tmp, int n, hipStream_t s, std::string* err) {
  size_t bytes = 0;
  MAP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const int32_t*)nullptr, (int32_t*)nullptr, n, s));
  return tmp.ensure(bytes, err);
}

int scan_total(const int32_t* flag, int32_t* slot, int n, const DevArr<unsigned char>& tmp, int64_t* sum,
               hipStream_t s, std::string* err) {
  size_t bytes = tmp.n * sizeof(unsigned char);              // all of the scratch: no less than n needs
  MAP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp.p, bytes, flag, slot, n, s));
  int32_t last_flag = 0, last_slot = 0;
  MAP_TRY(hipMemcpyAsync(&last_flag, flag + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MAP_TRY(hipMemcpyAsync(&last_slot, slot + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MAP_TRY(hipStreamSynchronize(s));
  *sum = (int64_t)last_flag + last_slot;
  return 0;
}

int map_index(MapState* st, const char* seq, const int64_t* off, int n_contigs, int seed_len, int max_occ,
              hipStream_t s, std::string* err) {
  const int64_t total = n_contigs > 0 ? off[n_contigs] : 0;
  // positions, and position + read length, stay in int32
  if (total > ((int64_t)1 << 31) - 1 - 2 * kMapMaxRead) {
    *err = "contigs of " + std::to_string(total) + " bases in total do not fit 32-bit positions";
    return -7;
  }
  st->have_index = false;
  st->have_mask = false;
  (void)hipStreamSynchronize(s);         // a device-resident map_pairs may still read the old index
  std::vector<int32_t> coff((size_t)n_contigs + 1, 0);
  for (int c = 0; c <= n_contigs && n_contigs > 0; ++c) coff[c] = (int32_t)off[c];
  const int64_t words = (total + 31) / 32 + 2;
  DevArr<unsigned char> d_seq;
  return synced_on_error(s, [&]() -> int {
    MAP_RC(st->pk.ensure(words, err));
    MAP_RC(st->nm.ensure(words, err));
    MAP_RC(st->coff.ensure(coff.size(), err));
    MAP_RC(d_seq.ensure(total, err));
    MAP_TRY(hipMemcpyAsync(st->coff.p, coff.data(), coff.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (total > 0) MAP_TRY(hipMemcpyAsync(d_seq.p, seq, (size_t)total, hipMemcpyHostToDevice, s));
    MAP_RC(map_pack(d_seq.p, total, false, st->pk.p, st->nm.p, s, err));
    st->n_contigs = n_contigs;
    st->seed_len = seed_len;
    st->max_occ = max_occ;
    st->total = total;
    MAP_RC(map_build_index(st, nullptr, s, err));
    st->n_kmers_plain = st->n_kmers;
    st->have_index = true;
    return 0;
  });
}

int map_build_index(MapState* st, const uint32_t* dm, hipStream_t s, std::string* err) {
  const int seed_len = st->seed_len;
  const int n_pos = (int)std::max<int64_t>(st->total - seed_len + 1, 0);
  const unsigned blocks = (unsigned)((n_pos + 255) / 256);
  // declared in the reverse of the order they are to be freed in (flag, slot, keys, kpos, tmp):
  // the order decides which freed blocks the buffers allocated next reuse
  DevArr<unsigned char> d_tmp;
  DevArr<int32_t> d_kpos;
  DevArr<uint64_t> d_keys;
  DevArr<int32_t> d_slot, d_flag;
  return synced_on_error(s, [&]() -> int {
    const MapIndexView ix = map_view(st);
    int64_t nk = 0;
    if (n_pos > 0) {
      MAP_RC(d_flag.ensure(n_pos, err));
      MAP_RC(d_slot.ensure(n_pos, err));
      hipLaunchKernelGGL(k_map_flag, dim3(blocks), dim3(256), 0, s, ix, dm, n_pos, d_flag.p);
      MAP_TRY(hipGetLastError());
      MAP_RC(scan_reserve(d_tmp, n_pos, s, err));
      MAP_RC(scan_total(d_flag.p, d_slot.p, n_pos, d_tmp, &nk, s, err));
    }
    MAP_RC(st->keys.ensure(std::max<int64_t>(nk, 1), err));
    MAP_RC(st->kpos.ensure(std::max<int64_t>(nk, 1), err));
    if (nk > 0) {
      MAP_RC(d_keys.ensure(nk, err));
      MAP_RC(d_kpos.ensure(nk, err));
      hipLaunchKernelGGL(k_map_emit, dim3(blocks), dim3(256), 0, s, ix, n_pos, d_flag.p, d_slot.p, d_keys.p, d_kpos.p);
      MAP_TRY(hipGetLastError());
      size_t bytes = 0;
      MAP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, d_keys.p, st->keys.p, d_kpos.p, st->kpos.p, (int)nk, 0,
                                                 2 * seed_len, s));
      MAP_RC(d_tmp.ensure(bytes, err));
      MAP_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, bytes, d_keys.p, st->keys.p, d_kpos.p, st->kpos.p, (int)nk, 0,
                                                 2 * seed_len, s));
    }
    // table bits: about two buckets per S-mer, at least 2^8 and at most 2^26 entries
    int bits = 8;
    while (bits < 26 && ((int64_t)1 << bits) < 2 * nk) ++bits;
    bits = std::min(bits, 2 * seed_len);
    st->bshift = 2 * seed_len - bits;
    st->n_kmers = nk;
    MAP_RC(st->bucket.ensure(((size_t)1 << bits) + 1, err));
    hipLaunchKernelGGL(k_map_bucket, dim3((unsigned)((nk + 1 + 255) / 256)), dim3(256), 0, s, st->keys.p, (int)nk,
                       st->bshift, (uint32_t)1 << bits, st->bucket.p);
    MAP_TRY(hipGetLastError());
    MAP_TRY(hipStreamSynchronize(s));
    return 0;
  });
}

namespace {

// map_pairs; with gout, also the gap fields (zeroed) and, for max_gap > 0, the rescue pass
int map_pairs_run(MapState* st, const MapReads& rd, const MapRule& rule, const MapOut& out, int max_gap,
                  const MapGapOut* gout, hipStream_t s, std::string* err) {
  const int64_t NP = rd.n_pairs;
  std::vector<int64_t> h1, h2;
  const int64_t *o1 = rd.off1, *o2 = rd.off2;
  if (NP == 0) return 0;
  if (rd.device_resident) {      // the read lengths are checked on the host either way
    h1.resize(NP + 1);
    h2.resize(NP + 1);
    MAP_TRY(hipMemcpyAsync(h1.data(), rd.off1, sizeof(int64_t) * (NP + 1), hipMemcpyDeviceToHost, s));
    MAP_TRY(hipMemcpyAsync(h2.data(), rd.off2, sizeof(int64_t) * (NP + 1), hipMemcpyDeviceToHost, s));
    MAP_TRY(hipStreamSynchronize(s));
    o1 = h1.data();
    o2 = h2.data();
  }
  for (const int64_t* o : {o1, o2}) {
    if (o[0] != 0) { *err = "read offsets must start at 0"; return -1; }
    for (int64_t i = 0; i < NP; ++i) {
      const int64_t len = o[i + 1] - o[i];
      if (len < 0) { *err = "read offsets decrease at pair " + std::to_string(i); return -1; }
      if (len > kMapMaxRead) {
        *err = "pair " + std::to_string(i) + ": a read of " + std::to_string(len) + " bases (at most " +
               std::to_string(kMapMaxRead) + ")";
        return -1;
      }
    }
  }
  MapPairArgs A{};
  A.ix = map_view(st);
  A.max_occ = rule.max_occ;
  A.max_mm = rule.max_mm;
  A.min_ins = rule.min_insert;
  A.max_ins = rule.max_insert;
  A.n_pairs = NP;
  if (rd.device_resident) {
    A.s1 = rd.seq1; A.o1 = rd.off1; A.s2 = rd.seq2; A.o2 = rd.off2;
    A.contig = out.contig; A.pos1 = out.pos1; A.pos2 = out.pos2;
    A.strand1 = out.strand1; A.mm1 = out.mm1; A.mm2 = out.mm2;
  } else {
    MAP_RC(st->s1.ensure(o1[NP], err));
    MAP_RC(st->s2.ensure(o2[NP], err));
    MAP_RC(st->o1.ensure(NP + 1, err));
    MAP_RC(st->o2.ensure(NP + 1, err));
    for (DevArr<int32_t>* b : {&st->r_contig, &st->r_pos1, &st->r_pos2}) MAP_RC(b->ensure(NP, err));
    for (DevArr<uint8_t>* b : {&st->r_strand, &st->r_mm1, &st->r_mm2}) MAP_RC(b->ensure(NP, err));
    if (o1[NP] > 0) MAP_TRY(hipMemcpyAsync(st->s1.p, rd.seq1, (size_t)o1[NP], hipMemcpyHostToDevice, s));
    if (o2[NP] > 0) MAP_TRY(hipMemcpyAsync(st->s2.p, rd.seq2, (size_t)o2[NP], hipMemcpyHostToDevice, s));
    MAP_TRY(hipMemcpyAsync(st->o1.p, o1, sizeof(int64_t) * (NP + 1), hipMemcpyHostToDevice, s));
    MAP_TRY(hipMemcpyAsync(st->o2.p, o2, sizeof(int64_t) * (NP + 1), hipMemcpyHostToDevice, s));
    A.s1 = st->s1.p; A.o1 = st->o1.p; A.s2 = st->s2.p; A.o2 = st->o2.p;
    A.contig = st->r_contig.p; A.pos1 = st->r_pos1.p; A.pos2 = st->r_pos2.p;
    A.strand1 = st->r_strand.p; A.mm1 = st->r_mm1.p; A.mm2 = st->r_mm2.p;
  }
  const size_t lds = (size_t)kMapFixedLds + (size_t)16 * 64 * (size_t)rule.max_occ;
  MAP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_map_pairs),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_map_pairs, dim3((unsigned)NP), dim3(64), lds, s, A);
  MAP_TRY(hipGetLastError());
  MapGapArgs GA{};
  if (gout) {
    GA.P = A;
    GA.max_gap = max_gap;
    if (rd.device_resident) {
      GA.d1 = gout->d1; GA.d2 = gout->d2; GA.k1 = gout->k1; GA.k2 = gout->k2; GA.flags = gout->flags;
    } else {
      MAP_RC(st->r_d1.ensure(NP, err));
      MAP_RC(st->r_d2.ensure(NP, err));
      MAP_RC(st->r_k1.ensure(NP, err));
      MAP_RC(st->r_k2.ensure(NP, err));
      MAP_RC(st->r_flags.ensure(NP, err));
      GA.d1 = st->r_d1.p; GA.d2 = st->r_d2.p; GA.k1 = st->r_k1.p; GA.k2 = st->r_k2.p; GA.flags = st->r_flags.p;
    }
    MAP_TRY(hipMemsetAsync(GA.d1, 0, (size_t)NP, s));
    MAP_TRY(hipMemsetAsync(GA.d2, 0, (size_t)NP, s));
    MAP_TRY(hipMemsetAsync(GA.k1, 0, sizeof(int16_t) * NP, s));
    MAP_TRY(hipMemsetAsync(GA.k2, 0, sizeof(int16_t) * NP, s));
    MAP_TRY(hipMemsetAsync(GA.flags, 0, (size_t)NP, s));
    if (max_gap > 0) MAP_RC(map_rescue(st, GA, s, err));
  }
  if (!rd.device_resident) {
    MAP_TRY(hipMemcpyAsync(out.contig, A.contig, sizeof(int32_t) * NP, hipMemcpyDeviceToHost, s));
    MAP_TRY(hipMemcpyAsync(out.pos1, A.pos1, sizeof(int32_t) * NP, hipMemcpyDeviceToHost, s));
    MAP_TRY(hipMemcpyAsync(out.pos2, A.pos2, sizeof(int32_t) * NP, hipMemcpyDeviceToHost, s));
    MAP_TRY(hipMemcpyAsync(out.strand1, A.strand1, (size_t)NP, hipMemcpyDeviceToHost, s));
    MAP_TRY(hipMemcpyAsync(out.mm1, A.mm1, (size_t)NP, hipMemcpyDeviceToHost, s));
    MAP_TRY(hipMemcpyAsync(out.mm2, A.mm2, (size_t)NP, hipMemcpyDeviceToHost, s));
    if (gout) {
      MAP_TRY(hipMemcpyAsync(gout->d1, GA.d1, (size_t)NP, hipMemcpyDeviceToHost, s));
      MAP_TRY(hipMemcpyAsync(gout->d2, GA.d2, (size_t)NP, hipMemcpyDeviceToHost, s));
      MAP_TRY(hipMemcpyAsync(gout->k1, GA.k1, sizeof(int16_t) * NP, hipMemcpyDeviceToHost, s));
      MAP_TRY(hipMemcpyAsync(gout->k2, GA.k2, sizeof(int16_t) * NP, hipMemcpyDeviceToHost, s));
      MAP_TRY(hipMemcpyAsync(gout->flags, GA.flags, (size_t)NP, hipMemcpyDeviceToHost, s));
    }
    MAP_TRY(hipStreamSynchronize(s));
  } else if (gout) {
    MAP_TRY(hipStreamSynchronize(s));
  }
  return 0;
}

}  // namespace

int map_pairs(MapState* st, const MapReads& rd, const MapRule& rule, const MapOut& out, hipStream_t s,
              std::string* err) {
  return map_pairs_run(st, rd, rule, out, 0, nullptr, s, err);
}

int map_pairs_gapped(MapState* st, const MapReads& rd, const MapRule& rule, int max_gap, const MapOut& out,
                     const MapGapOut& gout, hipStream_t s, std::string* err) {
  return map_pairs_run(st, rd, rule, out, max_gap, &gout, s, err);
}

}  // namespace wf
