// Workgroup building blocks of the retrieval kernels (evaluator.hip, rank_stream.hip, rank_cuhk03.hip, topk.hip,
// rerank_sparse.hip): sort keys, scans, the LDS bitonic sort, the fixed-association reductions and the Market
// evaluator's batch core.  Device code, all inlined, but for the one host declaration at the end.
#pragma once
#include "common.h"

namespace ieee {

// ---- order words: a monotone 32-bit image of a distance, so that (word << 32 | gallery index) sorts on
// (distance, index) with unsigned compares.  There are two orders, and each protocol keeps its own:
//   raw     the IEEE total order: -0.0 before +0.0, NaNs by sign and payload (negative NaNs first, positive last).
//           The Market1501 evaluator (rank_query_fast_kernel, rank_query_kernel) uses it.  Its reference sort
//           compares floats, for which -0.0 == +0.0: on a row that holds both zeros the evaluator puts a -0.0 entry
//           before a +0.0 entry of a lower gallery index and the reference does not.  That is a known property of
//           the evaluator, pinned by test_rank_signed_zero_order_is_the_same_on_both_paths.
//   folded  -0.0 == +0.0 and every NaN after +inf: a stable argsort's order.  The CUHK03 evaluator and the top-k
//           kernel use it.
// Making them one order would change results: do not.
__device__ __forceinline__ uint32_t order_word_raw(float d) {
  uint32_t u = __float_as_uint(d);
  u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
  return u;
}
__device__ __forceinline__ uint32_t order_word_folded(float d) {
  uint32_t u = order_word_raw(d);
  if (d == 0.f) u = 0x80000000u;
  if (d != d) u = 0xFFFFFFFFu;
  return u;
}
__device__ __forceinline__ uint64_t order_key(uint32_t word, uint32_t idx) { return ((uint64_t)word << 32) | idx; }
// the distance of a key (of a raw word: exactly; of a folded word: +0.0 for both zeros, one NaN for all)
__device__ __forceinline__ float key_dist(uint64_t key) {
  uint32_t u = (uint32_t)(key >> 32);
  u ^= (u >> 31) ? 0x80000000u : 0xFFFFFFFFu;
  return __uint_as_float(u);
}

// ---- scans
// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(v, o);
    if (lane >= o) v += y;
  }
  return v;
}

// exclusive scan of one word per thread over a 256-thread block: returns the exclusive prefix and writes the block
// total to *total.  wsum: 4 LDS words, free again on return (two barriers).
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* wsum, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t inc = wave_scan_incl(v);
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t s = wsum[w];
    if (w < wave) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

// ---- sort keys[0, n) in LDS ascending (n >= 1, room for the next power of two): [n, np2) is padded with ~0ull.
// The caller has NOT synchronised yet: the first barrier comes after the padding, so it also orders the caller's own
// writes of keys[0, n) and whatever else the caller cleared just before the call.  One barrier after every step; the
// keys are sorted and visible to all threads on return.
template <int THREADS>
__device__ __forceinline__ void lds_bitonic_sort(uint64_t* keys, uint32_t n) {
  const uint32_t t = threadIdx.x;
  uint32_t np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (uint32_t i = n + t; i < np2; i += THREADS) keys[i] = ~0ull;
  __syncthreads();
  for (uint32_t k = 2; k <= np2; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = t; i < np2; i += THREADS) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const uint64_t a = keys[i], b = keys[l];
          const bool up = (i & k) == 0;
          if ((a > b) == up) { keys[i] = b; keys[l] = a; }
        }
      }
      __syncthreads();
    }
  }
}

// ---- reductions over a 256-thread block with ONE association: the binary tree o = 128 ... 1 over LDS, so a float64
// sum has the same bits on every launch and in every kernel that sums the same values (the evaluators' repeat-call and
// cross-protocol tests rest on it; no shuffles here).  Results are in dsum[0] (and aux[0]) after the last barrier.
__device__ __forceinline__ void block_tree_sum(double s, double* dsum) {
  const int t = threadIdx.x;
  dsum[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) dsum[t] += dsum[t + o];
    __syncthreads();
  }
}
// the same tree with a second value reduced alongside by op (an int32 min, a uint32 sum)
template <typename T, typename Op>
__device__ __forceinline__ void block_tree_sum(double s, T v, double* dsum, T* aux, Op op) {
  const int t = threadIdx.x;
  dsum[t] = s;
  aux[t] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) { dsum[t] += dsum[t + o]; aux[t] = op(aux[t], aux[t + o]); }
    __syncthreads();
  }
}

// ---- the batch core of the Market evaluator's query kernels (evaluator.hip: rank_query_fast_kernel, rank_query_kernel;
// rank_stream.hip: stream_count_kernel)
constexpr int RANK_CAP = 1024;    // match keys sorted per batch (LDS)
constexpr int RANK_CELLS = 512;   // distance cells over the batch's match range
constexpr int RANK_UNR = 8;       // 16-byte loads per thread in flight in rank_query_fast_kernel's stream

// the Market protocol orders on the raw IEEE total order (see the order words above)
__device__ __forceinline__ uint64_t make_key(float d, uint32_t idx) { return order_key(order_word_raw(d), idx); }

// Cell of a distance on the uniform grid laid over [dmin, dmax] of a batch's sorted match keys.  Every step
// (subtract a constant, multiply by a non-negative constant, min, truncate) is monotone under rounding, so
// a < b implies cell(a) <= cell(b): keys in lower cells are smaller, keys in higher cells are larger, and only
// the keys sharing the element's cell have to be compared.
__device__ __forceinline__ uint32_t rank_cell(float d, float dmin, float scale) {
  return (uint32_t)(int)fminf((d - dmin) * scale, (float)(RANK_CELLS - 1));   // NaN -> last cell
}

// ---- the batch core of the two query kernels: what they do with a batch of nb <= RANK_CAP match keys is the same;
// how the keys are collected, what an element adds to hist and how the removed entries leave it is theirs.
struct RankGrid {
  uint64_t kmin, kmax;       // the batch's smallest and largest match key
  float dmin, dmax, scale;   // their distances, and cells per unit of distance
  uint32_t hlen;             // words of hist in use: slots 0 .. RANK_CELLS + nb + 1
};

// keys[0, nb) are the batch's match keys in any order, written by the caller and not yet synchronised (the first
// barrier is lds_bitonic_sort's; it also covers what the caller cleared just before the call).  On return the keys are
// sorted, hist is zero up to its scan slack, cellinfo[c] = first key index of cell c | keys in the cell << 16, and all
// of it is visible to the block.
__device__ __forceinline__ RankGrid rank_prepare_batch(uint64_t* keys, uint32_t nb, uint32_t* hist, uint32_t* cellinfo,
                                                       uint32_t* wsum) {
  const uint32_t t = threadIdx.x;
  RankGrid g;
  g.hlen = RANK_CELLS + nb + 2;
  for (uint32_t i = t; i < g.hlen + 512; i += 256) hist[i] = 0;
  for (uint32_t i = t; i < RANK_CELLS; i += 256) cellinfo[i] = 0;
  lds_bitonic_sort<256>(keys, nb);
  g.kmin = keys[0];
  g.kmax = keys[nb - 1];
  g.dmin = key_dist(g.kmin);
  g.dmax = key_dist(g.kmax);
  g.scale = (float)RANK_CELLS / (g.dmax - g.dmin);
  if (!(g.scale < 1e30f)) g.scale = 0.f;         // one distinct distance (or inf/NaN): a single cell
  // count the keys of every cell, then an exclusive scan gives the first key of each
  for (uint32_t i = t; i < nb; i += 256) atomicAdd(&cellinfo[rank_cell(key_dist(keys[i]), g.dmin, g.scale)], 1u);
  __syncthreads();
  constexpr int PER = RANK_CELLS / 256;
  uint32_t c[PER], sum = 0;
#pragma unroll
  for (int e = 0; e < PER; ++e) { c[e] = cellinfo[t * PER + e]; sum += c[e]; }
  uint32_t tot;
  uint32_t run = block_scan_excl(sum, wsum, &tot);
#pragma unroll
  for (int e = 0; e < PER; ++e) { cellinfo[t * PER + e] = run | (c[e] << 16); run += c[e]; }
  __syncthreads();
  return g;
}

// inclusive prefix sums over hist[0, hlen) in place: a contiguous odd-length span per thread (conflict-free; the spans
// reach into hist's 512 words of slack, which are zero)
__device__ __forceinline__ void rank_scan_hist(uint32_t* hist, uint32_t hlen, uint32_t* wsum) {
  const uint32_t t = threadIdx.x, per = ((hlen + 255) / 256) | 1u;
  uint32_t sum = 0;
  for (uint32_t e = 0; e < per; ++e) sum += hist[t * per + e];
  uint32_t tot;
  uint32_t run = block_scan_excl(sum, wsum, &tot);
  for (uint32_t e = 0; e < per; ++e) { run += hist[t * per + e]; hist[t * per + e] = run; }
  __syncthreads();
}

// rank_finalize_kernel (evaluator.hip) on ap / first: summary = [max_rank CMC counts, number of valid queries, bits of
// the AP sum].  The one host function of this header: the kernel lives in evaluator.hip and rank_stream.hip ends with it.
int rank_finalize_launch(const double* ap, const int32_t* first, int64_t num_q, int64_t max_rank, int64_t* summary,
                         hipStream_t stream);

}  // namespace ieee
