// The kernels and the workspace plan of sparse k-reciprocal re-ranking, shared by rerank_sparse.hip (distances read from
// three finished matrices: RsView) and rerank_stream.hip (distances read from the buffer one distance GEMM left:
// RsBlockView, RsRangeView).  A kernel that reads distances is a template on the view; the others are static, one copy
// per file that launches them.
#pragma once
#include <algorithm>

#include "rank_common.h"

namespace ieee {

constexpr int RS_MAXK = 64;                        // k1 + 1 <= 64
constexpr int RS_MAXE = RS_MAXK * (RS_MAXK / 2 + 2);
constexpr int RS_U = 16;                           // rows loaded per lane between two candidate-buffer checks
constexpr int RS_MAXS = 16;                        // row chunks per column strip, at most
constexpr int RS_EXPAND_BLOCKS = 1024;             // resident rows of step D (each owns an N-float scratch row)

struct RsView {                   // the virtual all-pairs matrix, column-wise
  const float *qg, *qq, *gg;
  int Q, G;
  // &orig[a][i], and the distance to orig[a+1][i] while a+1 stays on the same side of Q
  __device__ __forceinline__ const float* col(int a, int i, int64_t& step) const {
    if (i < Q) {
      if (a < Q) { step = Q; return qq + (int64_t)a * Q + i; }
      step = 1; return qg + (int64_t)i * G + (a - Q);
    }
    step = G;
    return a < Q ? qg + (int64_t)a * G + (i - Q) : gg + (int64_t)(a - Q) * G + (i - Q);
  }
  __device__ __forceinline__ float at(int a, int i) const { int64_t s; return *col(a, i, s); }
  // what a view tells the strip kernels: the columns [c0, c1) and rows [r0, r1) it holds, and the row at which col()'s
  // step changes
  __device__ __forceinline__ int c0() const { return 0; }
  __device__ __forceinline__ int c1() const { return Q + G; }
  __device__ __forceinline__ int r0() const { return 0; }
  __device__ __forceinline__ int r1() const { return Q + G; }
  __device__ __forceinline__ int split() const { return Q; }
  // and step F: gallery columns [0, jw()) are rows joff() ... of the sparse arrays; qgat(i, g) is the Q x G block
  __device__ __forceinline__ int jw() const { return G; }
  __device__ __forceinline__ int joff() const { return Q; }
  __device__ __forceinline__ int64_t ldo() const { return G; }
  __device__ __forceinline__ float qgat(int i, int g) const { return qg[(int64_t)i * G + g]; }
};

// One block orig[a0, a1)[i0, i1) of the virtual matrix, where a distance GEMM left it: element (a, i) at
// buf[(a - a0) * sa + (i - i0) * si].  (sa, si) = (ld, 1) for a buffer whose rows are the rows a, (1, ld) for the
// Q x G block serving as orig[a in G][i in Q], which is read transposed.
struct RsBlockView {
  const float* buf;
  int64_t sa, si;
  int a0, a1, i0, i1;
  __device__ __forceinline__ const float* col(int a, int i, int64_t& step) const {
    step = sa;
    return buf + (int64_t)(a - a0) * sa + (int64_t)(i - i0) * si;
  }
  __device__ __forceinline__ int c0() const { return i0; }
  __device__ __forceinline__ int c1() const { return i1; }
  __device__ __forceinline__ int r0() const { return a0; }
  __device__ __forceinline__ int r1() const { return a1; }
  __device__ __forceinline__ int split() const { return a0; }        // one stride for all its rows
};

// Step F on one gallery range [g0, g0 + w): the Q x w distances of a slab buffer, the result into rows of stride ldo_
struct RsRangeView {
  const float* d;
  int64_t ldd, ldo_;
  int joff_, w;
  __device__ __forceinline__ int jw() const { return w; }
  __device__ __forceinline__ int joff() const { return joff_; }
  __device__ __forceinline__ int64_t ldo() const { return ldo_; }
  __device__ __forceinline__ float qgat(int i, int g) const { return d[(int64_t)i * ldd + g]; }
};

// A: one lane per column, rows [a0, a1) of that column.  Squares are >= 0, so the max is an unsigned max of the bits.
template <class View>
__global__ __launch_bounds__(64) void rs_colmax_kernel(View o, int rows_per_chunk, unsigned* __restrict__ colmax) {
  const int N = o.c1(), Q = o.split();
  const int i = o.c0() + blockIdx.x * 64 + threadIdx.x;
  const int ic = i < N ? i : N - 1;                  // idle lanes walk a real column and drop the result
  const int a0 = o.r0() + blockIdx.y * rows_per_chunk, a1 = min(o.r1(), a0 + rows_per_chunk);
  float m = 0.f;
  for (int side = 0; side < 2; ++side) {
    const int lo = side ? max(a0, Q) : a0, hi = side ? a1 : min(a1, Q);
    if (lo >= hi) continue;
    int64_t step;
    const float* p = o.col(lo, ic, step);
    int a = lo;
    for (; a + RS_U <= hi; a += RS_U, p += RS_U * step) {
      float v[RS_U];
#pragma unroll
      for (int u = 0; u < RS_U; ++u) v[u] = p[u * step];
#pragma unroll
      for (int u = 0; u < RS_U; ++u) m = fmaxf(m, v[u] * v[u]);
    }
    for (; a < hi; ++a, p += step) { const float v = *p; m = fmaxf(m, v * v); }
  }
  if (i < N) atomicMax(colmax + i, __float_as_uint(m));
}

// Largest s with fl(s / c) <= d, or +inf when that is not found in a few steps.  Division by c > 0 is monotone, so a
// square above the bound has D > d and cannot enter the candidate buffer; at or below it, the exact key decides.
static __device__ float rs_square_bound(float d, float c) {
  if (!(d >= 0.f && d < INFINITY && c > 0.f && c < INFINITY)) return INFINITY;
  float s = d * c;
  if (!(s < INFINITY)) return INFINITY;
  for (int n = 0; n < 8; ++n) {
    const float up = __uint_as_float(__float_as_uint(s) + 1u);
    if (!(up / c <= d)) return s;
    s = up;
  }
  return INFINITY;
}

// B1: one lane per column i, rows [a0, a1): the K smallest keys (bits(D) << 32 | j) -- D >= 0, so the unsigned order
// of the key is the dense kernel's (D, j) order, ties to the lower index.  A key enters the lane's LDS buffer only
// below the running K-th key; when a lane's buffer could overflow during the next group, every lane cuts back to K.
// SEED (the view holds some of the rows only): seed[i][0..K) is column i's list over the rows seen before, ascending,
// ~0 where it is not full yet.  Its K-th key bounds every chunk from the start and chunk 0 carries its keys on, so the
// chunk lists of this call merge into the list over all rows so far.  part is [chunk][column - c0][K].
template <class View, bool SEED>
__global__ __launch_bounds__(64) void rs_select_kernel(View o, const unsigned* __restrict__ colmax, int rows_per_chunk,
                                                       int K, uint64_t* __restrict__ part,
                                                       const uint64_t* __restrict__ seed) {
  extern __shared__ uint64_t buf[];                // [cap][64]
  const int N = o.c1(), Q = o.split(), lane = threadIdx.x, cap = K + 2 * RS_U;
  const int i = o.c0() + blockIdx.x * 64 + lane;
  const int ic = i < N ? i : N - 1;
  const int a0 = o.r0() + blockIdx.y * rows_per_chunk, a1 = min(o.r1(), a0 + rows_per_chunk);
  const float c = __uint_as_float(colmax[ic]);
  uint64_t thr = ~0ull;
  float sq_hi = INFINITY;
  int cnt = 0;
  if constexpr (SEED) {
    const uint64_t* s = seed + (int64_t)ic * K;
    if (blockIdx.y == 0)
      for (int k = 0; k < K; ++k) {
        const uint64_t key = s[k];
        if (key != ~0ull) { buf[cnt * 64 + lane] = key; ++cnt; }
      }
    const uint64_t last = s[K - 1];
    if (last != ~0ull) {
      thr = last;
      sq_hi = rs_square_bound(__uint_as_float((uint32_t)(thr >> 32)), c);
    }
  }
  auto compact = [&]() {                           // buf[0, min(K, cnt)) = the smallest keys, ascending
    const int keep = min(K, cnt);
    for (int k = 0; k < keep; ++k) {
      int best = k;
      uint64_t bv = buf[k * 64 + lane];
      for (int s = k + 1; s < cnt; ++s) {
        const uint64_t x = buf[s * 64 + lane];
        if (x < bv) { bv = x; best = s; }
      }
      buf[best * 64 + lane] = buf[k * 64 + lane];
      buf[k * 64 + lane] = bv;
    }
    cnt = keep;
    if (keep == K) {
      thr = buf[(K - 1) * 64 + lane];
      sq_hi = rs_square_bound(__uint_as_float((uint32_t)(thr >> 32)), c);
    }
  };
  for (int side = 0; side < 2; ++side) {
    const int lo = side ? max(a0, Q) : a0, hi = side ? a1 : min(a1, Q);
    if (lo >= hi) continue;
    int64_t step;
    const float* p = o.col(lo, ic, step);
    for (int a = lo; a < hi; a += RS_U) {
      const int n = min(RS_U, hi - a);             // uniform over the wave
      float v[RS_U];
#pragma unroll
      for (int u = 0; u < RS_U; ++u) v[u] = u < n ? p[u * step] : 0.f;
#pragma unroll
      for (int u = 0; u < RS_U; ++u) {
        const float sq = v[u] * v[u];
        if (u < n && !(sq > sq_hi)) {
          const float d = sq / c;
          const uint64_t key = (uint64_t)__float_as_uint(d) << 32 | (uint32_t)(a + u);
          if (key < thr) { buf[cnt * 64 + lane] = key; ++cnt; }
        }
      }
      p += (int64_t)n * step;
      if (__any(cnt > cap - RS_U)) compact();
    }
  }
  compact();
  if (i < N) {
    uint64_t* dst = part + ((int64_t)blockIdx.y * (N - o.c0()) + (i - o.c0())) * K;
    for (int k = 0; k < K; ++k) dst[k] = k < cnt ? buf[k * 64 + lane] : ~0ull;
  }
}

// B2: one wave per column: the K smallest of its S chunk lists.  An index that is not a real column (a padding key:
// only when fewer than K rows were seen, which N >= K excludes) is replaced by i, so rank never points out of [0, N).
// KEYS: part holds the lists of the N columns from c0 on, and the merged keys themselves go to keys[c0 + i] (the
// running lists that rs_select_kernel<., true> is seeded with), padding keys included.
template <bool KEYS>
__global__ __launch_bounds__(64) void rs_merge_kernel(const uint64_t* __restrict__ part, int S, int N, int K,
                                                      int* __restrict__ rank, uint64_t* __restrict__ keys, int c0) {
  constexpr int PER = RS_MAXS * RS_MAXK / 64;
  const int i = blockIdx.x, lane = threadIdx.x, tot = S * K;
  uint64_t kv[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int p = lane + 64 * u;
    kv[u] = p < tot ? part[((int64_t)(p / K) * N + i) * K + p % K] : ~0ull;
  }
  for (int k = 0; k < K; ++k) {
    uint64_t best = ~0ull;
#pragma unroll
    for (int u = 0; u < PER; ++u) best = kv[u] < best ? kv[u] : best;
    for (int off = 32; off > 0; off >>= 1) {
      const uint64_t other = __shfl_xor(best, off);
      best = other < best ? other : best;
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) if (kv[u] == best) kv[u] = ~0ull;     // keys are unique
    const uint32_t j = (uint32_t)best;
    if constexpr (KEYS) {
      if (lane == 0) keys[(int64_t)(c0 + i) * K + k] = best;
    } else {
      if (lane == 0) rank[(int64_t)i * K + k] = (best != ~0ull && j < (uint32_t)N) ? (int)j : i;
    }
  }
}

struct RsSets {                   // the LDS of one row's set logic
  int R[RS_MAXK], Rc[RS_MAXK], E[RS_MAXE];
  unsigned char F[RS_MAXE];
  int nR, nRc, nE, cnt, nU;
};

// The set logic of row i (a 64-thread block): E[0, ne) = R(i) and the accepted half-size reciprocal sets, in the order
// the dense kernel appends them, repeats included.  Returns ne; nU is zeroed.
__device__ __forceinline__ int rs_krecip_sets(RsSets& s, const int* __restrict__ rank, int i, int K, int Kh) {
  int (&R)[RS_MAXK] = s.R, (&Rc)[RS_MAXK] = s.Rc, (&E)[RS_MAXE] = s.E;
  int &nR = s.nR, &nRc = s.nRc, &nE = s.nE, &cnt = s.cnt, &nU = s.nU;
  const int t = threadIdx.x;
  if (t == 0) { nR = 0; nE = 0; nU = 0; }
  __syncthreads();
  for (int k = 0; k < K; ++k) {                    // R(i), in rank order
    const int f = rank[(int64_t)i * K + k];
    bool hit = false;
    for (int u = t; u < K; u += 64) hit |= rank[(int64_t)f * K + u] == i;
    const bool any = __syncthreads_or(hit);
    if (any && t == 0) { R[nR] = f; E[nE] = f; ++nR; ++nE; }
    __syncthreads();
  }
  const int nr = nR;
  for (int c = 0; c < nr; ++c) {                   // expansion by the half-size reciprocal sets
    const int cand = R[c];
    if (t == 0) { nRc = 0; cnt = 0; }
    __syncthreads();
    for (int k = 0; k < Kh; ++k) {
      const int f = rank[(int64_t)cand * K + k];
      bool hit = false;
      for (int u = t; u < Kh; u += 64) hit |= rank[(int64_t)f * K + u] == cand;
      const bool any = __syncthreads_or(hit);
      if (any && t == 0) { Rc[nRc] = f; ++nRc; }
      __syncthreads();
    }
    const int nrc = nRc;
    if (t < nrc) {
      bool in = false;
      for (int u = 0; u < nr; ++u) in |= R[u] == Rc[t];
      if (in) atomicAdd(&cnt, 1);
    }
    __syncthreads();
    if ((double)cnt > 2. / 3 * (double)nrc) {
      if (t < nrc) E[nE + t] = Rc[t];
      __syncthreads();
      if (t == 0) nE += nrc;
    }
    __syncthreads();
  }
  return nE;
}

// C: the dense rr_krecip_kernel's set logic and weight sum (same association), with D[i][e] gathered from the inputs;
// the unique members are written in ascending column order.  One 64-thread block per row.
template <class View>
__global__ __launch_bounds__(64) void rs_krecip_kernel(View o, const unsigned* __restrict__ colmax,
                                                       const int* __restrict__ rank, int N, int K, int Kh, int capV,
                                                       int* __restrict__ Vn, int* __restrict__ Vi, float* __restrict__ Vv) {
  __shared__ RsSets sets;
  __shared__ float wsum[64];
  const int i = blockIdx.x, t = threadIdx.x;
  const int ne = rs_krecip_sets(sets, rank, i, K, Kh);
  int (&E)[RS_MAXE] = sets.E;
  unsigned char (&F)[RS_MAXE] = sets.F;
  int& nU = sets.nU;
  const float ci = __uint_as_float(colmax[i]);
  float local = 0.f;
  for (int p = t; p < ne; p += 64) {               // unique(E): a position counts if no earlier one holds its index
    const int e = E[p];
    bool first = true;
    for (int u = 0; u < p; ++u) first &= E[u] != e;
    F[p] = first;
    if (first) {
      const float v = o.at(e, i);
      local += expf(-(v * v / ci));
      atomicAdd(&nU, 1);
    }
  }
  wsum[t] = local;
  __syncthreads();
  for (int s = 32; s > 0; s >>= 1) { if (t < s) wsum[t] += wsum[t + s]; __syncthreads(); }
  const float total = wsum[0];
  for (int p = t; p < ne; p += 64) {
    if (!F[p]) continue;
    const int e = E[p];
    int pos = 0;
    for (int u = 0; u < ne; ++u) pos += F[u] && E[u] < e;
    const float v = o.at(e, i);
    if (pos < capV) {
      Vi[(int64_t)i * capV + pos] = e;
      Vv[(int64_t)i * capV + pos] = 1.f * expf(-(v * v / ci)) / total;
    }
  }
  if (t == 0) Vn[i] = min(nU, capV);
}

__device__ __forceinline__ unsigned rs_load_word(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// D: rows r = blockIdx.x, +gridDim.x, ...  The k2 rows are added into a dense scratch row in t order (the columns of one
// row are distinct: no races; 0 + v = v, so skipping the dense path's zero terms keeps its bits), touched columns are
// marked in a bitmap (global atomics), and the bitmap is walked in ascending order to emit, divide and clear.
static __global__ __launch_bounds__(256) void rs_expand_kernel(const int* __restrict__ rank, int N, int K, int k2,
                                                        const int* __restrict__ Vn, const int* __restrict__ Vi,
                                                        const float* __restrict__ Vv, int capV, int capQ,
                                                        float* __restrict__ scratch, int64_t sstride,
                                                        int* __restrict__ Qn, int* __restrict__ Qi, float* __restrict__ Qv) {
  __shared__ uint32_t s_wsum[4];
  float* acc = scratch + (int64_t)blockIdx.x * sstride;
  unsigned* bits = (unsigned*)(acc + N);
  const int W = (N + 31) >> 5, per = (W + 255) / 256;
  const int w0 = min(W, (int)threadIdx.x * per), w1 = min(W, w0 + per);
  const float fk2 = (float)k2;
  for (int r = blockIdx.x; r < N; r += gridDim.x) {
    for (int t = 0; t < k2; ++t) {
      const int j = rank[(int64_t)r * K + t];
      const int n = Vn[j];
      for (int p = threadIdx.x; p < n; p += 256) {
        const int c = Vi[(int64_t)j * capV + p];
        acc[c] += Vv[(int64_t)j * capV + p];
        atomicOr(bits + (c >> 5), 1u << (c & 31));
      }
      __syncthreads();
    }
    uint32_t mine = 0, total;
    for (int w = w0; w < w1; ++w) mine += __popc(rs_load_word(bits + w));
    int off = (int)block_scan_excl(mine, s_wsum, &total);
    for (int w = w0; w < w1; ++w) {
      unsigned b = rs_load_word(bits + w);
      if (!b) continue;
      atomicExch(bits + w, 0u);
      while (b) {
        const int c = w * 32 + __ffs(b) - 1;
        b &= b - 1;
        if (off < capQ) {
          Qi[(int64_t)r * capQ + off] = c;
          Qv[(int64_t)r * capQ + off] = acc[c] / fk2;
        }
        acc[c] = 0.f;
        ++off;
      }
    }
    if (threadIdx.x == 0) Qn[r] = min((int)total, capQ);
    __syncthreads();
  }
}

// E1: entries per column over the gallery rows
static __global__ __launch_bounds__(256) void rs_inv_count_kernel(const int* __restrict__ n, const int* __restrict__ idx, int cap,
                                                           int Q, int* __restrict__ cnt) {
  const int j = Q + blockIdx.x;
  const int nj = n[j];
  for (int p = threadIdx.x; p < nj; p += 256) atomicAdd(cnt + idx[(int64_t)j * cap + p], 1);
}

// E2: off[c] = sum of cnt[0, c), off[N] = total (one block)
static __global__ __launch_bounds__(1024) void rs_scan_kernel(const int* __restrict__ cnt, int N, int64_t* __restrict__ off) {
  __shared__ int64_t s[1024];
  const int t = threadIdx.x, per = (N + 1023) / 1024;
  const int c0 = min(N, t * per), c1 = min(N, c0 + per);
  int64_t mine = 0;
  for (int c = c0; c < c1; ++c) mine += cnt[c];
  s[t] = mine;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int64_t add = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  int64_t run = s[t] - mine;
  for (int c = c0; c < c1; ++c) { off[c] = run; run += cnt[c]; }
  if (t == 1023) off[N] = s[1023];
}

// E3: fill; the order inside a column does not matter (its rows are distinct).  cnt counts down to 0 again.
static __global__ __launch_bounds__(256) void rs_inv_fill_kernel(const int* __restrict__ n, const int* __restrict__ idx,
                                                          const float* __restrict__ val, int cap, int Q,
                                                          const int64_t* __restrict__ off, int* __restrict__ cnt,
                                                          int* __restrict__ inv_j, float* __restrict__ inv_v) {
  const int j = Q + blockIdx.x;
  const int nj = n[j];
  for (int p = threadIdx.x; p < nj; p += 256) {
    const int c = idx[(int64_t)j * cap + p];
    const int64_t q = off[c] + atomicSub(cnt + c, 1) - 1;
    inv_j[q] = j;
    inv_v[q] = val[(int64_t)j * cap + p];
  }
}

// F: one block per query row.  The output row is the accumulator: zeroed, then for each c of the row's support in
// ascending order min(Vq[i][c], Vq[j][c]) is added at every gallery j of column c (distinct j: no atomics; a barrier
// between two c keeps each sum in c order), then the final combine in place, as rr_jaccard_kernel writes it.
// The view names the gallery columns it covers (all of them, or one range whose inverted index this is).
template <class View>
__global__ __launch_bounds__(256) void rs_jaccard_kernel(View o, const unsigned* __restrict__ colmax,
                                                         const int* __restrict__ n, const int* __restrict__ idx,
                                                         const float* __restrict__ val, int cap,
                                                         const int64_t* __restrict__ off, const int* __restrict__ inv_j,
                                                         const float* __restrict__ inv_v, float one_minus_lambda,
                                                         float lambda, float* __restrict__ out) {
  const int i = blockIdx.x, t = threadIdx.x, Q = o.joff(), G = o.jw();
  float* row = out + (int64_t)i * o.ldo();
  for (int g = t; g < G; g += 256) row[g] = 0.f;
  __syncthreads();
  const int ni = n[i];
  for (int p = 0; p < ni; ++p) {
    const int c = idx[(int64_t)i * cap + p];
    const float a = val[(int64_t)i * cap + p];
    const int64_t q1 = off[c + 1];
    for (int64_t q = off[c] + t; q < q1; q += 256) {
      float* dst = row + (inv_j[q] - Q);
      *dst = *dst + fminf(a, inv_v[q]);
    }
    __syncthreads();
  }
  const float ci = __uint_as_float(colmax[i]);
  for (int g = t; g < G; g += 256) {
#pragma clang fp contract(off)      // two rounded products and a rounded sum, as rr_jaccard_kernel computes them
    const float tm = row[g];
    const float jac = 1.f - tm / (2.f - tm);
    const float v = o.qgat(i, g);
    const float d = v * v / ci;
    row[g] = jac * one_minus_lambda + d * lambda;
  }
}

// Workspace plan: one function for the query and the launch, so the two cannot drift.
struct RsPlan {
  int64_t N, K, Kh, capV, capQ, capUse, S, rows, P, sstride;
  int64_t colmax, rank, vn, vi, vv, qn, qi, qv, cnt, off, uni, part, scr, invj, invv, total;
};

static bool rs_plan(int64_t Q, int64_t G, int64_t k1, int64_t k2, RsPlan& p) {
  if (Q <= 0 || G <= 0 || k1 < 1 || k1 + 1 > RS_MAXK || k2 < 1 || k2 > k1 + 1) return false;
  const int64_t N = Q + G;
  if (N >= ((int64_t)1 << 31) || k1 + 1 > N) return false;
  p.N = N;
  p.K = k1 + 1;
  p.Kh = (int64_t)nearbyint((double)k1 / 2.) + 1;                 // np.around: round half to even (rerank.py:63)
  p.capV = std::min(p.K * (1 + p.Kh), N);
  p.capQ = k2 != 1 ? std::min(k2 * p.capV, N) : 0;
  p.capUse = k2 != 1 ? p.capQ : p.capV;
  const int64_t strips = (N + 63) / 64;
  int64_t S = std::max<int64_t>(1, std::min<int64_t>({(8192 + strips - 1) / strips, (int64_t)RS_MAXS, N / 256}));
  p.rows = (N + S - 1) / S;
  p.S = (N + p.rows - 1) / p.rows;
  p.P = std::min<int64_t>(N, RS_EXPAND_BLOCKS);
  p.sstride = (N + (N + 31) / 32 + 63) & ~(int64_t)63;            // floats: acc[N] + bitmap[N/32], 256-byte rows
  int64_t at = 0;
  auto take = [&](int64_t bytes) { const int64_t a = at; at += align256(bytes); return a; };
  p.colmax = take(N * 4);
  p.rank = take(N * p.K * 4);
  p.vn = take(N * 4);
  p.vi = take(N * p.capV * 4);
  p.vv = take(N * p.capV * 4);
  p.qn = take(k2 != 1 ? N * 4 : 0);
  p.qi = take(N * p.capQ * 4);
  p.qv = take(N * p.capQ * 4);
  p.cnt = take(N * 4);
  p.off = take((N + 1) * 8);
  p.uni = at;                                      // one region, three lives: B's chunk lists, D's scratch, E's index
  const int64_t part = p.S * N * p.K * 8;
  const int64_t scr = k2 != 1 ? p.P * p.sstride * 4 : 0;
  const int64_t inv = align256(G * p.capUse * 4) * 2;
  p.part = p.scr = p.invj = p.uni;
  p.invv = p.uni + align256(G * p.capUse * 4);
  p.total = p.uni + align256(std::max({part, scr, inv})) + 256;
  return true;
}

}  // namespace ieee
