// Market1501-protocol CMC / mAP without the [num_q][num_g] matrix: the gallery's distances arrive in column slabs, in two
// passes.  The host knows every label before anything starts and hands over a plan: per query the gallery indices of
// its true matches (same identity, other camera) and of its removed entries (same identity, same camera), as two CSR
// lists.  Pass 1 (collect) turns the planned entries into (distance, GLOBAL index) keys; seal sorts them; pass 2
// (count) is rank_query_fast_kernel's stream over one slab -- the sorted matches in LDS, the cell table, a histogram,
// a prefix sum -- whose result is ADDED to a running count per match, so the slabs may come in any order; the removed
// entries leave through their sorted keys (in the count pass or by bisection in finish, see stream_by_keys), and finish
// forms AP and first exactly as the whole-row kernel does.  No labels on the device, no atomics on global memory, no
// floating-point atomics: the same bits on every call.
#include "rank_common.h"

namespace ieee {

// the device state of one evaluation, carved out of one allocation (every region on a 256-byte boundary)
struct StreamState {
  uint64_t* mkeys;    // [total_m] match keys, CSR order; sorted ascending inside a query after seal
  uint64_t* rkeys;    // [total_r] removed keys, likewise
  uint32_t* counts;   // [total_m] gallery entries with key <= the match key, over the slabs counted so far
  double* ap;         // [num_q]
  int32_t* first;     // [num_q]
  int64_t bytes;
};
static StreamState stream_layout(void* state, int64_t num_q, int64_t total_m, int64_t total_r) {
  StreamState s;
  char* p = (char*)state;
  int64_t at = 0;
  s.mkeys = (uint64_t*)(p + at);  at += align256(total_m * 8);
  s.rkeys = (uint64_t*)(p + at);  at += align256(total_r * 8);
  s.counts = (uint32_t*)(p + at); at += align256(total_m * 4);
  s.ap = (double*)(p + at);       at += align256(num_q * 8);
  s.first = (int32_t*)(p + at);   at += align256(num_q * 4);
  s.bytes = at;
  return s;
}

// Pass 1, grid (num_q, 2): y = 0 the query's matches, y = 1 its removed entries.  pos[i] is the place of entry i in
// match_columns; the slab holds places col_base ... col_base + slab_cols - 1.  Every entry has one place, so every key
// is written by exactly one launch of a full pass.
__global__ __launch_bounds__(256) void stream_collect_kernel(const float* __restrict__ slab, int64_t ldd, int slab_cols,
                                                             int col_base, const int64_t* __restrict__ m_off,
                                                             const int32_t* __restrict__ m_pos,
                                                             const int32_t* __restrict__ m_idx, uint64_t* mkeys,
                                                             const int64_t* __restrict__ r_off,
                                                             const int32_t* __restrict__ r_pos,
                                                             const int32_t* __restrict__ r_idx, uint64_t* rkeys) {
  const int q = blockIdx.x, t = threadIdx.x;
  const bool rem = blockIdx.y != 0;
  const int64_t* off = rem ? r_off : m_off;
  const int32_t* pos = rem ? r_pos : m_pos;
  const int32_t* idx = rem ? r_idx : m_idx;
  uint64_t* keys = rem ? rkeys : mkeys;
  const float* row = slab + (int64_t)q * ldd;
  const int64_t e = off[q + 1];
  for (int64_t i = off[q] + t; i < e; i += 256) {
    const uint32_t p = (uint32_t)(pos[i] - col_base);
    if (p < (uint32_t)slab_cols) keys[i] = make_key(row[p], (uint32_t)idx[i]);
  }
}

// Seal, grid (num_q, 2): sort one segment of keys ascending.  Up to RANK_CAP keys in LDS; a longer segment (rare) in
// place in global memory, by the bitonic network whose every comparison sends the larger key to the higher index --
// the places past the segment's end then stand for +inf without existing: no comparison would ever move them.
__global__ __launch_bounds__(256) void stream_seal_kernel(const int64_t* __restrict__ m_off, uint64_t* mkeys,
                                                          const int64_t* __restrict__ r_off, uint64_t* rkeys) {
  __shared__ uint64_t keys[RANK_CAP];
  const int q = blockIdx.x, t = threadIdx.x;
  const int64_t* off = blockIdx.y ? r_off : m_off;
  uint64_t* seg = (blockIdx.y ? rkeys : mkeys) + off[q];
  const int64_t n64 = off[q + 1] - off[q];
  if (n64 <= 1) return;
  if (n64 <= RANK_CAP) {
    const uint32_t n = (uint32_t)n64;
    for (uint32_t i = t; i < n; i += 256) keys[i] = seg[i];
    lds_bitonic_sort<256>(keys, n);
    for (uint32_t i = t; i < n; i += 256) seg[i] = keys[i];
    return;
  }
  const uint64_t n = (uint64_t)n64;
  uint64_t np2 = 1;
  while (np2 < n) np2 <<= 1;
  auto step = [&](uint64_t mask) {
    for (uint64_t i = t; i < np2; i += 256) {
      const uint64_t l = i ^ mask;
      if (l > i && l < n) {
        const uint64_t a = seg[i], b = seg[l];
        if (a > b) { seg[i] = b; seg[l] = a; }
      }
    }
    __syncthreads();
  };
  for (uint64_t k = 2; k <= np2; k <<= 1) {
    step(k - 1);                                  // two ascending runs of k/2: compare with the mirror place
    for (uint64_t j = k >> 2; j > 0; j >>= 1) step(j);
  }
}

// Which of the whole-matrix kernels serves a query: rank_query_fast_kernel up to RANK_CAP matches and RANK_CAP removed
// entries, rank_query_kernel beyond.  They place an element among the match keys in two ways -- the first decides on
// float compares where it can (a NaN beside finite matches goes after them whatever its sign), the second compares keys
// throughout -- and the streamed evaluation follows the one the whole matrix would have got, so that it returns the
// same numbers on every input.
__device__ __forceinline__ bool stream_by_keys(int64_t nm, int64_t nr) { return nm > RANK_CAP || nr > RANK_CAP; }

// Pass 2, one workgroup per query: rank_query_fast_kernel's stream over one slab.  For every batch of at most RANK_CAP
// of the query's sorted match keys: cell table, histogram of the slab's row (element keys carry the GLOBAL index
// g_base + column), prefix sum, and counts[match] += what this slab adds to the match's rank.  It reads no labels: a
// removed entry is counted like any element; then, for a query of the fast kind, the removed keys whose index lies in
// the slab are taken out of the slots they were counted in, as rank_query_fast_kernel does (the keys hold index and
// distance); for the other kind they leave in the finish.  Only this workgroup touches the query's counts, and
// launches on one stream are ordered: plain read-modify-write.
__global__ __launch_bounds__(256) void stream_count_kernel(const float* slab, int64_t ldd, int slab_g, int g_base,
                                                           const int64_t* __restrict__ m_off,
                                                           const int64_t* __restrict__ r_off,
                                                           const uint64_t* __restrict__ mkeys,
                                                           const uint64_t* __restrict__ rkeys, uint32_t* counts) {
  constexpr int HIST = RANK_CELLS + RANK_CAP + 2;
  __shared__ uint64_t keys[RANK_CAP];
  __shared__ uint32_t hist[HIST + 512];          // slack: the scan reads whole per-thread spans
  __shared__ uint32_t cellinfo[RANK_CELLS];      // first key index of the cell | keys in the cell << 16
  __shared__ uint32_t wsum[4];

  const int q = blockIdx.x, t = threadIdx.x;
  const float* row = slab + (int64_t)q * ldd;
  const int64_t m0 = m_off[q], nm = m_off[q + 1] - m0;
  const int64_t r0 = r_off[q], nr = r_off[q + 1] - r0;
  const bool by_keys = stream_by_keys(nm, nr);
  for (int64_t b0 = 0; b0 < nm; b0 += RANK_CAP) {
    const uint32_t nb = (uint32_t)min((int64_t)RANK_CAP, nm - b0);
    const uint64_t* src = mkeys + m0 + b0;
    for (uint32_t i = t; i < nb; i += 256) keys[i] = src[i];
    const RankGrid grid = rank_prepare_batch(keys, nb, hist, cellinfo, wsum);
    const float dmin = grid.dmin, dmax = grid.dmax, scale = grid.scale;
    const uint64_t kmin = grid.kmin, kmax = grid.kmax;
    // slot of an element (k: its GLOBAL index), or -1 when it lies after every match of the batch: the ends by keys as
    // in rank_query_kernel, or by float compares as in rank_query_fast_kernel
    auto slot_of = [&](float d, uint32_t k) -> int {
      if (by_keys) {
        const uint64_t key = make_key(d, k);
        if (key > kmax) return -1;
        if (key < kmin) return 0;
      } else {
        if (d > dmax) return -1;
        if (d < dmin) return 0;
      }
      const uint32_t c = rank_cell(d, dmin, scale);
      const uint32_t ci = cellinfo[c];
      uint32_t lo = ci & 0xffffu;
      if (ci >> 16) {
        const uint64_t key = make_key(d, k);
        uint32_t hi = lo + (ci >> 16);             // lower_bound among the keys of this cell
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (keys[mid] < key) lo = mid + 1; else hi = mid;
        }
      }
      return (int)(1 + c + lo);
    };
    uint32_t below = 0;
    auto visit = [&](float d, int k) {
      const int sl = slot_of(d, (uint32_t)(g_base + k));
      if (sl > 0) atomicAdd(&hist[sl], 1u);
      else if (sl == 0) ++below;
    };
    // ---- stream the slab's row: RANK_UNR independent 16-byte loads per thread in flight before any is used
    constexpr int UNR = RANK_UNR;
    int kdone = 0;
    if (((uintptr_t)row & 15) == 0) {
      for (; kdone + UNR * 1024 <= slab_g; kdone += UNR * 1024) {
        f32x4 d4[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) d4[u] = __builtin_nontemporal_load((const f32x4*)(row + kdone + u * 1024 + t * 4));
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const int k = kdone + u * 1024 + t * 4;
          visit(d4[u].x, k);
          visit(d4[u].y, k + 1);
          visit(d4[u].z, k + 2);
          visit(d4[u].w, k + 3);
        }
      }
    }
    for (int k = kdone + t; k < slab_g; k += 256) visit(row[k], k);
    if (below) atomicAdd(&hist[0], below);
    __syncthreads();
    if (!by_keys) {
      // ---- the removed entries of this slab (rank.py:136-137) leave the slots the stream counted them in
      for (uint32_t i = t; i < (uint32_t)nr; i += 256) {
        const uint64_t key = rkeys[r0 + i];
        const uint32_t k = (uint32_t)key;
        if (k - (uint32_t)g_base < (uint32_t)slab_g) {
          const int sl = slot_of(key_dist(key), k);
          if (sl >= 0) atomicSub(&hist[sl], 1u);
        }
      }
      __syncthreads();
    }
    rank_scan_hist(hist, grid.hlen, wsum);
    uint32_t* dst = counts + m0 + b0;
    for (uint32_t i = t; i < nb; i += 256) {
      const uint32_t c = rank_cell(key_dist(keys[i]), dmin, scale);
      dst[i] += hist[1 + c + i];                   // elements of this slab up to and including match i's key
    }
    __syncthreads();                               // the next batch overwrites keys, hist and cellinfo
  }
}

// Finish, one workgroup per query.  counts[i] is the number of gallery entries with key <= match i's key, itself
// included; where the count pass left the removed entries in (stream_by_keys), those among them are the removed keys
// below the match key (bisection in the sorted list), so
//   rank_i = counts[i] - 1 - #{removed keys < key_i}
// is the 0-based position of match i among the kept entries, and i matches precede it.  AP has
// rank_query_fast_kernel's association: thread-strided partial sums, then the block tree.
__global__ __launch_bounds__(256) void stream_finish_kernel(const int64_t* __restrict__ m_off,
                                                            const int64_t* __restrict__ r_off,
                                                            const uint64_t* __restrict__ mkeys,
                                                            const uint64_t* __restrict__ rkeys,
                                                            const uint32_t* __restrict__ counts, double* ap_out,
                                                            int32_t* first_out) {
  __shared__ double dsum[256];
  __shared__ int32_t imin[256];
  const int q = blockIdx.x, t = threadIdx.x;
  const int64_t m0 = m_off[q], nm = m_off[q + 1] - m0;
  const int64_t r0 = r_off[q], nr = r_off[q + 1] - r0;
  if (nm == 0) {
    if (t == 0) { ap_out[q] = -1.0; first_out[q] = -1; }   // rank.py:140-142: no valid match, query skipped
    return;
  }
  double part = 0.0;
  int32_t fmin = 0x7fffffff;
  const bool by_keys = stream_by_keys(nm, nr);             // else the count pass took the removed entries out already
  for (int64_t i = t; i < nm; i += 256) {
    const uint64_t key = mkeys[m0 + i];
    int64_t lo = 0, hi = by_keys ? nr : 0;                 // removed keys below the match key
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (rkeys[r0 + mid] < key) lo = mid + 1; else hi = mid;
    }
    const uint32_t rank = counts[m0 + i] - 1 - (uint32_t)lo;   // 0-based position among kept
    part += (double)(i + 1) / (double)(rank + 1);              // rank.py:156-157; i matches precede match i
    fmin = min(fmin, (int32_t)rank);
  }
  block_tree_sum(part, fmin, dsum, imin, [](int32_t a, int32_t b) { return min(a, b); });
  if (t == 0) {
    ap_out[q] = dsum[0] / (double)nm;                          // rank.py:153-158
    first_out[q] = imin[0];
  }
}

}  // namespace ieee

using namespace ieee;

#define STREAM_COMMON(who)                                                                                              \
  IEEE_REQUIRE(num_q >= 0 && total_match_keys >= 0 && total_removed_keys >= 0, who ": negative size");                  \
  IEEE_REQUIRE(num_q < (1ll << 31), who ": too many queries");                                                          \
  const StreamState S = stream_layout(state, num_q, total_match_keys, total_removed_keys);                              \
  IEEE_REQUIRE(state && ((uintptr_t)state & 7) == 0, who ": null or misaligned state");                                 \
  IEEE_REQUIRE(state_bytes >= S.bytes, who ": state of %ld bytes, %ld needed", (long)state_bytes, (long)S.bytes)

extern "C" int64_t ieee_rank_stream_workspace_bytes(int64_t num_q, int64_t total_match_keys, int64_t total_removed_keys) {
  if (num_q < 0 || total_match_keys < 0 || total_removed_keys < 0) return -1;
  const int64_t bytes = stream_layout(nullptr, num_q, total_match_keys, total_removed_keys).bytes;
  return bytes > 0 ? bytes : 256;
}

extern "C" int ieee_rank_stream_collect(const float* slab, int64_t ldd, int64_t num_q, int64_t slab_cols, int64_t col_base,
                                        const int64_t* m_off, const int32_t* m_pos, const int32_t* m_idx,
                                        const int64_t* r_off, const int32_t* r_pos, const int32_t* r_idx,
                                        int64_t total_match_keys, int64_t total_removed_keys, void* state,
                                        int64_t state_bytes, void* stream) {
  STREAM_COMMON("rank_stream_collect");
  IEEE_REQUIRE(slab_cols >= 0 && col_base >= 0 && col_base + slab_cols < (1ll << 31),
               "rank_stream_collect: columns %ld + %ld out of range", (long)col_base, (long)slab_cols);
  if (num_q == 0 || slab_cols == 0) return IEEE_OK;
  IEEE_REQUIRE(slab && m_off && r_off, "rank_stream_collect: null pointer");
  IEEE_REQUIRE((m_pos && m_idx) || total_match_keys == 0, "rank_stream_collect: null match plan");
  IEEE_REQUIRE((r_pos && r_idx) || total_removed_keys == 0, "rank_stream_collect: null removed plan");
  IEEE_REQUIRE(ldd >= slab_cols, "rank_stream_collect: ldd %ld < slab_cols %ld", (long)ldd, (long)slab_cols);
  stream_collect_kernel<<<dim3((unsigned)num_q, 2), 256, 0, (hipStream_t)stream>>>(
      slab, ldd, (int)slab_cols, (int)col_base, m_off, m_pos, m_idx, S.mkeys, r_off, r_pos, r_idx, S.rkeys);
  return launch_status("rank_stream_collect");
}

extern "C" int ieee_rank_stream_seal(int64_t num_q, const int64_t* m_off, const int64_t* r_off, int64_t total_match_keys,
                                     int64_t total_removed_keys, void* state, int64_t state_bytes, void* stream) {
  STREAM_COMMON("rank_stream_seal");
  if (num_q == 0) return IEEE_OK;
  IEEE_REQUIRE(m_off && r_off, "rank_stream_seal: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (total_match_keys) IEEE_HIP(hipMemsetAsync(S.counts, 0, sizeof(uint32_t) * total_match_keys, st));
  stream_seal_kernel<<<dim3((unsigned)num_q, 2), 256, 0, st>>>(m_off, S.mkeys, r_off, S.rkeys);
  return launch_status("rank_stream_seal");
}

extern "C" int ieee_rank_stream_count(const float* slab, int64_t ldd, int64_t num_q, int64_t slab_g, int64_t g_base,
                                      const int64_t* m_off, const int64_t* r_off, int64_t total_match_keys,
                                      int64_t total_removed_keys,
                                      void* state, int64_t state_bytes, void* stream) {
  STREAM_COMMON("rank_stream_count");
  IEEE_REQUIRE(slab_g >= 0 && g_base >= 0 && g_base + slab_g < (1ll << 31),
               "rank_stream_count: gallery entries %ld + %ld out of range", (long)g_base, (long)slab_g);
  if (num_q == 0 || slab_g == 0) return IEEE_OK;
  IEEE_REQUIRE(slab && m_off && r_off, "rank_stream_count: null pointer");
  IEEE_REQUIRE(ldd >= slab_g, "rank_stream_count: ldd %ld < slab_g %ld", (long)ldd, (long)slab_g);
  stream_count_kernel<<<(unsigned)num_q, 256, 0, (hipStream_t)stream>>>(slab, ldd, (int)slab_g, (int)g_base, m_off, r_off,
                                                                        S.mkeys, S.rkeys, S.counts);
  return launch_status("rank_stream_count");
}

extern "C" int ieee_rank_stream_finish(int64_t num_q, const int64_t* m_off, const int64_t* r_off, int64_t total_match_keys,
                                       int64_t total_removed_keys, void* state, int64_t state_bytes, int64_t max_rank,
                                       double* ap, int32_t* first_pos, int64_t* summary, void* stream) {
  STREAM_COMMON("rank_stream_finish");
  IEEE_REQUIRE(max_rank >= 1 && max_rank <= 1024, "rank_stream_finish: max_rank %ld out of range [1,1024]", (long)max_rank);
  IEEE_REQUIRE(summary, "rank_stream_finish: null summary");
  IEEE_REQUIRE(num_q == 0 || (m_off && r_off), "rank_stream_finish: null pointer");
  hipStream_t st = (hipStream_t)stream;
  double* ap_use = ap ? ap : S.ap;
  int32_t* first_use = first_pos ? first_pos : S.first;
  if (num_q)
    stream_finish_kernel<<<(unsigned)num_q, 256, 0, st>>>(m_off, r_off, S.mkeys, S.rkeys, S.counts, ap_use, first_use);
  return rank_finalize_launch(ap_use, first_use, num_q, max_rank, summary, st);
}
