// Paired-read mapper on MI355X (gfx950, wave64): a deterministic seed-and-verify ungapped
// mapper for waafle_junctions' read input (DESIGN.md §11 states the rule; tests/map_oracle.py
// restates it on the CPU).  Not a bowtie2 clone: no gaps, no clipping, no MAPQ.
//
// Index (map_index):
//   k_map_pack    thread per 32 bases: the contig store as two bit planes in one 64-bit word
//                 (x: low bit, y: high bit of the base code A0 C1 G2 T3) and a 1-bit N plane;
//                 the store is padded so the window read of words w and w + 1 stays in bounds
//   k_map_flag    thread per position: 1 when the S-mer there has no N and stays in its contig
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
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "wf_internal.h"
#include "wf_lanes.h"

namespace wf {

struct MapBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

struct MapState {
  // the index (kept between calls)
  MapBuf pk, nm, coff, keys, kpos, bucket;
  int n_contigs = 0, seed_len = 0, max_occ = 0, bshift = 0;
  int64_t total = 0, n_kmers = 0;
  bool have_index = false;
  // read staging (host-resident calls)
  MapBuf s1, o1, s2, o2, r_contig, r_pos1, r_pos2, r_strand, r_mm1, r_mm2;
};

namespace {

constexpr int kMapMaxRead = 512;        // bases per mate
constexpr int kMapSlots = 16;           // seed slots per (mate, strand)
constexpr int kMapWords = kMapMaxRead / 32;
constexpr int kMapRow = kMapWords + 1;  // + a zero word: the seed window reads word w + 1
constexpr int kMapFixedLds = (3 * 4 * kMapRow + 8) * 4 + 2 * kMapMaxRead;

struct MapIndexView {
  const uint2* pk;            // [words + 2] x: low plane, y: high plane
  const uint32_t* nm;         // [words + 2] N plane
  const int32_t* coff;        // [n_contigs + 1] start of each contig in the store
  const uint64_t* keys;       // [n_kmers] sorted
  const int32_t* kpos;        // [n_kmers] position of each sorted S-mer
  const uint32_t* bucket;     // [2^bits + 1]
  int n_contigs, S, bshift;
};

struct MapPairArgs {
  MapIndexView ix;
  int max_occ, max_mm;
  int64_t min_ins, max_ins, n_pairs;
  const char* s1; const int64_t* o1; const char* s2; const int64_t* o2;
  int32_t* contig; int32_t* pos1; int32_t* pos2; uint8_t* strand1; uint8_t* mm1; uint8_t* mm2;
};

// A0 C1 G2 T3, anything else 4 (N); lower case counts as upper
__device__ __forceinline__ int base_code(unsigned char ch) {
  if (ch >= 'a' && ch <= 'z') ch -= 32;
  return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4;
}

// bits [sh, sh + 32) of the 64-bit value hi:lo
__device__ __forceinline__ uint32_t window32(uint32_t lo, uint32_t hi, int sh) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
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

__global__ void k_map_pack(const unsigned char* seq, int64_t total, int64_t words, uint2* pk, uint32_t* nm) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= words) return;
  uint32_t lo = 0, hi = 0, n = 0;
  for (int b = 0; b < 32; ++b) {
    const int64_t i = w * 32 + b;
    const int code = i < total ? base_code(seq[i]) : 4;      // the padding is N
    lo |= (uint32_t)(code & 1) << b;
    hi |= (uint32_t)((code >> 1) & 1) << b;
    n |= (uint32_t)(code >> 2) << b;
  }
  pk[w] = make_uint2(lo & ~n, hi & ~n);
  nm[w] = n;
}

// the S-mer at store position q: false when it holds an N
__device__ __forceinline__ bool store_kmer(const MapIndexView& ix, int q, uint64_t* key) {
  const int W = q >> 5, sh = q & 31;
  const uint32_t mask = ix.S == 32 ? 0xFFFFFFFFu : (1u << ix.S) - 1u;
  if (window32(ix.nm[W], ix.nm[W + 1], sh) & mask) return false;
  const uint2 a = ix.pk[W], b = ix.pk[W + 1];
  *key = ((uint64_t)(window32(a.y, b.y, sh) & mask) << ix.S) | (window32(a.x, b.x, sh) & mask);
  return true;
}

__global__ void k_map_flag(const MapIndexView ix, int n_pos, int32_t* flag) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_pos) return;
  uint64_t key;
  const int c = contig_of(ix.coff, ix.n_contigs, q);
  flag[q] = (int64_t)q + ix.S <= ix.coff[c + 1] && store_kmer(ix, q, &key);
}

__global__ void k_map_emit(const MapIndexView ix, int n_pos, const int32_t* flag, const int32_t* slot,
                           uint64_t* keys, int32_t* kpos) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_pos || !flag[q]) return;
  uint64_t key = 0;
  store_kmer(ix, q, &key);
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
  {
    const unsigned char* src = asc + (v >> 1) * kMapMaxRead;
    uint32_t lo = 0, hi = 0, n = 0;
    for (int b = 0; b < 32; ++b) {
      const int i = slot * 32 + b;
      if (i >= Lv) break;
      int code = base_code((v & 1) ? src[Lv - 1 - i] : src[i]);
      if ((v & 1) && code < 4) code = 3 - code;
      lo |= (uint32_t)(code & 1) << b;
      hi |= (uint32_t)((code >> 1) & 1) << b;
      n |= (uint32_t)(code >> 2) << b;
    }
    xlo[v * kMapRow + slot] = lo & ~n;
    xhi[v * kMapRow + slot] = hi & ~n;
    xnn[v * kMapRow + slot] = n;
    if (slot == 0) {
      xlo[v * kMapRow + kMapWords] = 0;
      xhi[v * kMapRow + kMapWords] = 0;
      xnn[v * kMapRow + kMapWords] = 0;
    }
  }
  __syncthreads();

  // lane = variant * 16 + seed slot: the seed's occurrences (none when it holds an N, is
  // absent, or occurs more than max_occ times)
  int first = 0, cnt = 0;
  const int off = slot * S;
  if (slot < min(Lv / S, kMapSlots)) {
    const int W = off >> 5, sh = off & 31;
    const uint32_t mask = S == 32 ? 0xFFFFFFFFu : (1u << S) - 1u;
    const uint32_t* r = xnn + v * kMapRow + W;
    if ((window32(r[0], r[1], sh) & mask) == 0) {
      const uint32_t* pl = xlo + v * kMapRow + W;
      const uint32_t* ph = xhi + v * kMapRow + W;
      const uint64_t key = ((uint64_t)(window32(ph[0], ph[1], sh) & mask) << S) | (window32(pl[0], pl[1], sh) & mask);
      const uint32_t b = (uint32_t)(key >> ix.bshift);
      int lo = (int)ix.bucket[b];
      const int end = (int)ix.bucket[b + 1];
      int hi = end;
      while (lo < hi) {                                      // lower bound within the bucket
        const int mid = (lo + hi) >> 1;
        if (ix.keys[mid] < key) lo = mid + 1; else hi = mid;
      }
      first = lo;
      while (cnt <= A.max_occ && lo + cnt < end && ix.keys[lo + cnt] == key) ++cnt;
      if (cnt > A.max_occ) cnt = 0;
    }
  }
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
    const int W = gg >> 5, sh = gg & 31;
    const uint2 a = ix.pk[W], b = ix.pk[W + 1];
    uint32_t mis = (xlo[uv * kMapRow + w] ^ window32(a.x, b.x, sh)) |
                   (xhi[uv * kMapRow + w] ^ window32(a.y, b.y, sh)) |
                   xnn[uv * kMapRow + w] | window32(ix.nm[W], ix.nm[W + 1], sh);
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

int map_ensure(MapBuf& b, size_t bytes, std::string* err) {
  if (bytes == 0) bytes = 16;
  if (b.bytes >= bytes) return 0;
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.bytes = 0;
  const hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) {
    *err = "hipMalloc(" + std::to_string(bytes) + ") failed: " + hipGetErrorString(e);
    return -2;
  }
  b.bytes = bytes;
  return 0;
}

void map_release(MapBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.bytes = 0;
}

MapIndexView map_view(const MapState* st) {
  MapIndexView ix{};
  ix.pk = static_cast<const uint2*>(st->pk.p);
  ix.nm = static_cast<const uint32_t*>(st->nm.p);
  ix.coff = static_cast<const int32_t*>(st->coff.p);
  ix.keys = static_cast<const uint64_t*>(st->keys.p);
  ix.kpos = static_cast<const int32_t*>(st->kpos.p);
  ix.bucket = static_cast<const uint32_t*>(st->bucket.p);
  ix.n_contigs = st->n_contigs;
  ix.S = st->seed_len;
  ix.bshift = st->bshift;
  return ix;
}

#define MAP_TRY(x)                                                                      \
  do {                                                                                  \
    hipError_t e_ = (x);                                                                \
    if (e_ != hipSuccess) { *err = std::string(#x) + ": " + hipGetErrorString(e_); rc = -2; goto done; } \
  } while (0)
#define MAP_RC(x)          \
  do {                     \
    if ((rc = (x))) goto done; \
  } while (0)

}  // namespace

MapState* map_create() { return new MapState(); }

void map_destroy(MapState* st) {
  if (!st) return;
  MapBuf* bufs[] = {&st->pk, &st->nm, &st->coff, &st->keys, &st->kpos, &st->bucket, &st->s1, &st->o1,
                    &st->s2, &st->o2, &st->r_contig, &st->r_pos1, &st->r_pos2, &st->r_strand, &st->r_mm1,
                    &st->r_mm2};
  for (MapBuf* b : bufs) map_release(*b);
  delete st;
}

int map_index_params(const MapState* st, int* seed_len, int* max_occ) {
  if (!st || !st->have_index) return 0;
  *seed_len = st->seed_len;
  *max_occ = st->max_occ;
  return 1;
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
  (void)hipStreamSynchronize(s);         // a device-resident map_pairs may still read the old index
  std::vector<int32_t> coff((size_t)n_contigs + 1, 0);
  for (int c = 0; c <= n_contigs && n_contigs > 0; ++c) coff[c] = (int32_t)off[c];
  const int64_t words = (total + 31) / 32 + 2;
  const int n_pos = (int)std::max<int64_t>(total - seed_len + 1, 0);
  MapBuf d_seq, d_flag, d_slot, d_keys, d_kpos, d_tmp;
  int rc = 0;
  int32_t last_flag = 0, last_slot = 0;
  int64_t nk = 0;
  int bits = 0;
  size_t tmp_bytes = 0;
  MapIndexView ix{};
  MAP_RC(map_ensure(st->pk, (size_t)words * sizeof(uint2), err));
  MAP_RC(map_ensure(st->nm, (size_t)words * sizeof(uint32_t), err));
  MAP_RC(map_ensure(st->coff, coff.size() * sizeof(int32_t), err));
  MAP_RC(map_ensure(d_seq, (size_t)total, err));
  MAP_TRY(hipMemcpyAsync(st->coff.p, coff.data(), coff.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (total > 0) MAP_TRY(hipMemcpyAsync(d_seq.p, seq, (size_t)total, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_map_pack, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s,
                     static_cast<const unsigned char*>(d_seq.p), total, words, static_cast<uint2*>(st->pk.p),
                     static_cast<uint32_t*>(st->nm.p));
  MAP_TRY(hipGetLastError());
  st->n_contigs = n_contigs;
  st->seed_len = seed_len;
  st->max_occ = max_occ;
  st->total = total;
  ix = map_view(st);
  if (n_pos > 0) {
    MAP_RC(map_ensure(d_flag, (size_t)n_pos * sizeof(int32_t), err));
    MAP_RC(map_ensure(d_slot, (size_t)n_pos * sizeof(int32_t), err));
    hipLaunchKernelGGL(k_map_flag, dim3((unsigned)((n_pos + 255) / 256)), dim3(256), 0, s, ix, n_pos,
                       static_cast<int32_t*>(d_flag.p));
    MAP_TRY(hipGetLastError());
    MAP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, static_cast<const int32_t*>(d_flag.p),
                                             static_cast<int32_t*>(d_slot.p), n_pos, s));
    MAP_RC(map_ensure(d_tmp, tmp_bytes, err));
    MAP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, tmp_bytes, static_cast<const int32_t*>(d_flag.p),
                                             static_cast<int32_t*>(d_slot.p), n_pos, s));
    MAP_TRY(hipMemcpyAsync(&last_flag, static_cast<const int32_t*>(d_flag.p) + (n_pos - 1), sizeof(int32_t),
                           hipMemcpyDeviceToHost, s));
    MAP_TRY(hipMemcpyAsync(&last_slot, static_cast<const int32_t*>(d_slot.p) + (n_pos - 1), sizeof(int32_t),
                           hipMemcpyDeviceToHost, s));
    MAP_TRY(hipStreamSynchronize(s));
    nk = (int64_t)last_flag + last_slot;
  }
  MAP_RC(map_ensure(st->keys, (size_t)std::max<int64_t>(nk, 1) * sizeof(uint64_t), err));
  MAP_RC(map_ensure(st->kpos, (size_t)std::max<int64_t>(nk, 1) * sizeof(int32_t), err));
  if (nk > 0) {
    MAP_RC(map_ensure(d_keys, (size_t)nk * sizeof(uint64_t), err));
    MAP_RC(map_ensure(d_kpos, (size_t)nk * sizeof(int32_t), err));
    hipLaunchKernelGGL(k_map_emit, dim3((unsigned)((n_pos + 255) / 256)), dim3(256), 0, s, ix, n_pos,
                       static_cast<const int32_t*>(d_flag.p), static_cast<const int32_t*>(d_slot.p),
                       static_cast<uint64_t*>(d_keys.p), static_cast<int32_t*>(d_kpos.p));
    MAP_TRY(hipGetLastError());
    tmp_bytes = 0;
    MAP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, static_cast<const uint64_t*>(d_keys.p),
                                               static_cast<uint64_t*>(st->keys.p),
                                               static_cast<const int32_t*>(d_kpos.p),
                                               static_cast<int32_t*>(st->kpos.p), (int)nk, 0, 2 * seed_len, s));
    MAP_RC(map_ensure(d_tmp, tmp_bytes, err));
    MAP_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, tmp_bytes, static_cast<const uint64_t*>(d_keys.p),
                                               static_cast<uint64_t*>(st->keys.p),
                                               static_cast<const int32_t*>(d_kpos.p),
                                               static_cast<int32_t*>(st->kpos.p), (int)nk, 0, 2 * seed_len, s));
  }
  // table bits: about two buckets per S-mer, at least 2^8 and at most 2^26 entries
  bits = 8;
  while (bits < 26 && ((int64_t)1 << bits) < 2 * nk) ++bits;
  bits = std::min(bits, 2 * seed_len);
  st->bshift = 2 * seed_len - bits;
  st->n_kmers = nk;
  MAP_RC(map_ensure(st->bucket, (((size_t)1 << bits) + 1) * sizeof(uint32_t), err));
  hipLaunchKernelGGL(k_map_bucket, dim3((unsigned)((nk + 1 + 255) / 256)), dim3(256), 0, s,
                     static_cast<const uint64_t*>(st->keys.p), (int)nk, st->bshift, (uint32_t)1 << bits,
                     static_cast<uint32_t*>(st->bucket.p));
  MAP_TRY(hipGetLastError());
  MAP_TRY(hipStreamSynchronize(s));
  st->have_index = true;
done:
  if (rc) (void)hipStreamSynchronize(s);
  for (MapBuf* b : {&d_seq, &d_flag, &d_slot, &d_keys, &d_kpos, &d_tmp}) map_release(*b);
  return rc;
}

int map_pairs(MapState* st, const MapReads& rd, const MapRule& rule, const MapOut& out, hipStream_t s,
              std::string* err) {
  const int64_t NP = rd.n_pairs;
  int rc = 0;
  std::vector<int64_t> h1, h2;
  const int64_t *o1 = rd.off1, *o2 = rd.off2;
  MapPairArgs A{};
  size_t lds = 0;
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
    MAP_RC(map_ensure(st->s1, (size_t)o1[NP], err));
    MAP_RC(map_ensure(st->s2, (size_t)o2[NP], err));
    MAP_RC(map_ensure(st->o1, sizeof(int64_t) * (NP + 1), err));
    MAP_RC(map_ensure(st->o2, sizeof(int64_t) * (NP + 1), err));
    MAP_RC(map_ensure(st->r_contig, sizeof(int32_t) * NP, err));
    MAP_RC(map_ensure(st->r_pos1, sizeof(int32_t) * NP, err));
    MAP_RC(map_ensure(st->r_pos2, sizeof(int32_t) * NP, err));
    MAP_RC(map_ensure(st->r_strand, (size_t)NP, err));
    MAP_RC(map_ensure(st->r_mm1, (size_t)NP, err));
    MAP_RC(map_ensure(st->r_mm2, (size_t)NP, err));
    if (o1[NP] > 0) MAP_TRY(hipMemcpyAsync(st->s1.p, rd.seq1, (size_t)o1[NP], hipMemcpyHostToDevice, s));
    if (o2[NP] > 0) MAP_TRY(hipMemcpyAsync(st->s2.p, rd.seq2, (size_t)o2[NP], hipMemcpyHostToDevice, s));
    MAP_TRY(hipMemcpyAsync(st->o1.p, o1, sizeof(int64_t) * (NP + 1), hipMemcpyHostToDevice, s));
    MAP_TRY(hipMemcpyAsync(st->o2.p, o2, sizeof(int64_t) * (NP + 1), hipMemcpyHostToDevice, s));
    A.s1 = static_cast<const char*>(st->s1.p); A.o1 = static_cast<const int64_t*>(st->o1.p);
    A.s2 = static_cast<const char*>(st->s2.p); A.o2 = static_cast<const int64_t*>(st->o2.p);
    A.contig = static_cast<int32_t*>(st->r_contig.p); A.pos1 = static_cast<int32_t*>(st->r_pos1.p);
    A.pos2 = static_cast<int32_t*>(st->r_pos2.p); A.strand1 = static_cast<uint8_t*>(st->r_strand.p);
    A.mm1 = static_cast<uint8_t*>(st->r_mm1.p); A.mm2 = static_cast<uint8_t*>(st->r_mm2.p);
  }
  lds = (size_t)kMapFixedLds + (size_t)16 * 64 * (size_t)rule.max_occ;
  MAP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_map_pairs),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_map_pairs, dim3((unsigned)NP), dim3(64), lds, s, A);
  MAP_TRY(hipGetLastError());
  if (!rd.device_resident) {
    MAP_TRY(hipMemcpyAsync(out.contig, A.contig, sizeof(int32_t) * NP, hipMemcpyDeviceToHost, s));
    MAP_TRY(hipMemcpyAsync(out.pos1, A.pos1, sizeof(int32_t) * NP, hipMemcpyDeviceToHost, s));
    MAP_TRY(hipMemcpyAsync(out.pos2, A.pos2, sizeof(int32_t) * NP, hipMemcpyDeviceToHost, s));
    MAP_TRY(hipMemcpyAsync(out.strand1, A.strand1, (size_t)NP, hipMemcpyDeviceToHost, s));
    MAP_TRY(hipMemcpyAsync(out.mm1, A.mm1, (size_t)NP, hipMemcpyDeviceToHost, s));
    MAP_TRY(hipMemcpyAsync(out.mm2, A.mm2, (size_t)NP, hipMemcpyDeviceToHost, s));
    MAP_TRY(hipStreamSynchronize(s));
  }
done:
  return rc;
}

}  // namespace wf
