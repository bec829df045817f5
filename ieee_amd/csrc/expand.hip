// Query expansion / database augmentation (ieee_amd/expansion.py): a descriptor is replaced by the weighted sum of its
// nearest neighbours' normalised rows.  The neighbour lists come from ieee_rank_topk_merge; here are the weights
// (similarity^alpha) and the gather-and-sum over the listed rows.  The reference has no such step.
#include "rank_common.h"

namespace ieee {

constexpr int NS_KMAX = 1024;   // the longest list (TOPK_MAX of the drivers): index and coefficient of a row stay in LDS
constexpr int NS_TILE = 4096;   // columns a workgroup keeps in registers: four float4 per thread

// w = s^alpha, s = max(1 - dist, 0), by alpha - 1 multiplications left to right; alpha 0: 1; a padded place: 0
__global__ void expand_weights_kernel(const int32_t* idx, const float* dist, int64_t count, int alpha, float* w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  float r = 0.f;
  if (idx[i] >= 0) {
    r = 1.f;
    if (alpha > 0) {
      const float s = fmaxf(1.f - dist[i], 0.f);   // NaN -> 0, as +inf
      r = s;
      for (int a = 1; a < alpha; ++a) r *= s;
    }
  }
  w[i] = r;
}

// four columns of a row from `col` on; the scalar form reads nothing at or beyond column d
template <bool VEC>
__device__ __forceinline__ float4 ns_load4(const float* __restrict__ p, int col, int d) {
  if constexpr (VEC) return *(const float4*)(p + col);
  float4 v;
  v.x = p[col];
  v.y = col + 1 < d ? p[col + 1] : 0.f;
  v.z = col + 2 < d ? p[col + 2] : 0.f;
  v.w = col + 3 < d ? p[col + 3] : 0.f;
  return v;
}
template <bool VEC>
__device__ __forceinline__ void ns_store4(float* __restrict__ p, int col, int d, float4 v) {
  if constexpr (VEC) { *(float4*)(p + col) = v; return; }
  p[col] = v.x;
  if (col + 1 < d) p[col + 1] = v.y;
  if (col + 2 < d) p[col + 2] = v.z;
  if (col + 3 < d) p[col + 3] = v.w;
}
__device__ __forceinline__ float4 ns_fma(float c, float4 x, float4 a) {
  return make_float4(fmaf(c, x.x, a.x), fmaf(c, x.y, a.y), fmaf(c, x.z, a.z), fmaf(c, x.w, a.w));
}

// Columns [tile, tile + NS_TILE) of one output row; thread t owns columns tile + 4 (t + 256 m) ... + 3, m = 0 .. 3, in
// the vector and in the scalar form alike.  Per element one fp32 chain: the self term (a product), then one fma per
// kept list entry in list order.  Two rows' loads are in flight at a time.
template <bool VEC>
__device__ __forceinline__ void ns_tile(const float* __restrict__ src, int64_t ld_src, const int32_t* s_idx,
                                        const float* s_c, int kc, const float* __restrict__ self_row, bool scale_self,
                                        float self_r, int tile, int d, float4 (&acc)[4]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int col = tile + 4 * (t + 256 * m);
    acc[m] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (self_row && col < d) {
      const float4 v = ns_load4<VEC>(self_row, col, d);
      acc[m] = scale_self ? make_float4(self_r * v.x, self_r * v.y, self_r * v.z, self_r * v.w) : v;
    }
  }
  int j = 0;
  for (; j + 2 <= kc; j += 2) {
    const float* r0 = src + (int64_t)s_idx[j] * ld_src;
    const float* r1 = src + (int64_t)s_idx[j + 1] * ld_src;
    const float c0 = s_c[j], c1 = s_c[j + 1];
    float4 x0[4], x1[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int col = tile + 4 * (t + 256 * m);
      if (col < d) { x0[m] = ns_load4<VEC>(r0, col, d); x1[m] = ns_load4<VEC>(r1, col, d); }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int col = tile + 4 * (t + 256 * m);
      if (col < d) acc[m] = ns_fma(c1, x1[m], ns_fma(c0, x0[m], acc[m]));
    }
  }
  if (j < kc) {
    const float* r0 = src + (int64_t)s_idx[j] * ld_src;
    const float c0 = s_c[j];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int col = tile + 4 * (t + 256 * m);
      if (col < d) acc[m] = ns_fma(c0, ns_load4<VEC>(r0, col, d), acc[m]);
    }
  }
}

// the squares of this thread's columns of a tile, ascending, onto its running float64 sum
__device__ __forceinline__ double ns_squares(const float4 (&acc)[4], int tile, int d, double ss) {
  const int t = threadIdx.x;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int col = tile + 4 * (t + 256 * m);
    if (col < d) ss += (double)acc[m].x * acc[m].x;
    if (col + 1 < d) ss += (double)acc[m].y * acc[m].y;
    if (col + 2 < d) ss += (double)acc[m].z * acc[m].z;
    if (col + 3 < d) ss += (double)acc[m].w * acc[m].w;
  }
  return ss;
}

// One workgroup per output row.  The list is compacted first: an index outside [0, n_src) is dropped before anything
// is read through it, and the coefficient w * rinv[index] of a kept entry is formed once.  d <= NS_TILE: the row stays
// in registers until it is scaled.  Beyond: the tiles are stored unscaled and every thread scales its own columns in a
// second pass over out.  The sum of squares is float64: per thread ascending, then block_tree_sum's one association.
template <bool VEC>
__global__ __launch_bounds__(256) void neighbour_sum_kernel(const float* __restrict__ src, int64_t ld_src, int64_t n_src,
                                                            const float* __restrict__ rinv, const int32_t* __restrict__ idx,
                                                            const float* __restrict__ w, int64_t ld_list, int k,
                                                            const float* __restrict__ self_rows,
                                                            const float* __restrict__ self_rinv, int64_t ld_self, int d,
                                                            int normalize, float* __restrict__ out, int64_t ld_out) {
  __shared__ int32_t s_idx[NS_KMAX];
  __shared__ float s_c[NS_KMAX];
  __shared__ double dsum[256];
  __shared__ uint32_t wsum[4];
  const int t = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int32_t* irow = idx + row * ld_list;
  const float* wrow = w + row * ld_list;
  int32_t v[4];
  float c[4];
  bool ok[4];
  uint32_t mine = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = 4 * t + e;
    ok[e] = false;
    if (j < k) {
      v[e] = irow[j];
      ok[e] = v[e] >= 0 && (int64_t)v[e] < n_src;
      if (ok[e]) c[e] = rinv ? wrow[j] * rinv[v[e]] : wrow[j];
    }
    mine += ok[e] ? 1u : 0u;
  }
  uint32_t total;
  uint32_t pos = block_scan_excl(mine, wsum, &total);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (ok[e]) { s_idx[pos] = v[e]; s_c[pos] = c[e]; ++pos; }
  __syncthreads();
  const int kc = (int)total;
  const float* self_row = self_rows ? self_rows + row * ld_self : nullptr;
  const bool scale_self = self_rows && self_rinv;
  const float self_r = scale_self ? self_rinv[row] : 1.f;
  float* orow = out + row * ld_out;
  float4 acc[4];
  if (d <= NS_TILE) {
    ns_tile<VEC>(src, ld_src, s_idx, s_c, kc, self_row, scale_self, self_r, 0, d, acc);
    float r = 1.f;
    if (normalize) {
      block_tree_sum(ns_squares(acc, 0, d, 0.0), dsum);
      r = 1.0f / fmaxf((float)sqrt(dsum[0]), 1e-12f);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int col = 4 * (t + 256 * m);
      if (col < d) {
        if (normalize) acc[m] = make_float4(acc[m].x * r, acc[m].y * r, acc[m].z * r, acc[m].w * r);
        ns_store4<VEC>(orow, col, d, acc[m]);
      }
    }
    return;
  }
  double ss = 0.0;
  for (int tile = 0; tile < d; tile += NS_TILE) {
    ns_tile<VEC>(src, ld_src, s_idx, s_c, kc, self_row, scale_self, self_r, tile, d, acc);
    ss = ns_squares(acc, tile, d, ss);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int col = tile + 4 * (t + 256 * m);
      if (col < d) ns_store4<VEC>(orow, col, d, acc[m]);
    }
  }
  if (!normalize) return;
  block_tree_sum(ss, dsum);
  const float r = 1.0f / fmaxf((float)sqrt(dsum[0]), 1e-12f);
  for (int tile = 0; tile < d; tile += NS_TILE) {   // every thread reads back what it stored itself
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int col = tile + 4 * (t + 256 * m);
      if (col < d) {
        const float4 y = ns_load4<VEC>(orow, col, d);
        ns_store4<VEC>(orow, col, d, make_float4(y.x * r, y.y * r, y.z * r, y.w * r));
      }
    }
  }
}

// bytes [lo, hi) of n rows of d floats with row stride ld
static inline void row_span(const float* p, int64_t n, int64_t ld, int64_t d, uintptr_t* lo, uintptr_t* hi) {
  *lo = (uintptr_t)p;
  *hi = *lo + (n > 0 ? (uintptr_t)((n - 1) * ld + d) * sizeof(float) : 0);
}
static inline bool aligned16(const void* p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

}  // namespace ieee

using namespace ieee;

extern "C" int ieee_expand_weights(const int32_t* idx, const float* dist, int64_t count, int64_t alpha, float* w,
                                   void* stream) {
  IEEE_REQUIRE(count >= 0 && count < (1ll << 40), "expand_weights: count %ld", (long)count);
  IEEE_REQUIRE(alpha >= 0 && alpha <= 64, "expand_weights: alpha %ld out of range [0, 64]", (long)alpha);
  if (count == 0) return IEEE_OK;
  IEEE_REQUIRE(idx && dist && w, "expand_weights: null pointer");
  expand_weights_kernel<<<(unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream>>>(idx, dist, count, (int)alpha, w);
  return launch_status("expand_weights");
}

extern "C" int ieee_neighbour_sum(const float* src, int64_t ld_src, int64_t n_src, const float* rinv, const int32_t* idx,
                                  const float* w, int64_t ld_list, int64_t n, int64_t k, const float* self_rows,
                                  const float* self_rinv, int64_t ld_self, int64_t d, int normalize, float* out,
                                  int64_t ld_out, void* stream) {
  IEEE_REQUIRE(n >= 0 && n < (1ll << 31) && n_src >= 0 && n_src < (1ll << 31), "neighbour_sum: rows n %ld, n_src %ld",
               (long)n, (long)n_src);
  IEEE_REQUIRE(k >= 1 && k <= NS_KMAX, "neighbour_sum: k %ld out of range [1, %d]", (long)k, NS_KMAX);
  IEEE_REQUIRE(d >= 1 && d < (1ll << 31) - 4 * NS_TILE, "neighbour_sum: d %ld out of range", (long)d);
  IEEE_REQUIRE(ld_list >= k && ld_src >= d && ld_out >= d, "neighbour_sum: stride below the row (lists %ld, src %ld, out %ld)",
               (long)ld_list, (long)ld_src, (long)ld_out);
  IEEE_REQUIRE(self_rows || !self_rinv, "neighbour_sum: self_rinv without self rows");
  IEEE_REQUIRE(!self_rows || ld_self >= d, "neighbour_sum: stride below the row (self %ld)", (long)ld_self);
  if (n == 0) return IEEE_OK;
  IEEE_REQUIRE(idx && w && out && (src || n_src == 0), "neighbour_sum: null pointer");
  uintptr_t olo, ohi, lo, hi;
  row_span(out, n, ld_out, d, &olo, &ohi);
  row_span(src, n_src, ld_src, d, &lo, &hi);
  IEEE_REQUIRE(n_src == 0 || ohi <= lo || hi <= olo, "neighbour_sum: out overlaps src (the sum is out of place)");
  if (self_rows) {
    row_span(self_rows, n, ld_self, d, &lo, &hi);
    IEEE_REQUIRE(ohi <= lo || hi <= olo, "neighbour_sum: out overlaps the self rows (the sum is out of place)");
  }
  hipStream_t st = (hipStream_t)stream;
  const bool vec = d % 4 == 0 && aligned16(out, ld_out) && (n_src == 0 || aligned16(src, ld_src)) &&
                   (!self_rows || aligned16(self_rows, ld_self));
  if (vec)
    neighbour_sum_kernel<true><<<(unsigned)n, 256, 0, st>>>(src, ld_src, n_src, rinv, idx, w, ld_list, (int)k, self_rows,
                                                            self_rinv, ld_self, (int)d, normalize, out, ld_out);
  else
    neighbour_sum_kernel<false><<<(unsigned)n, 256, 0, st>>>(src, ld_src, n_src, rinv, idx, w, ld_list, (int)k, self_rows,
                                                             self_rinv, ld_self, (int)d, normalize, out, ld_out);
  return launch_status("neighbour_sum");
}
