// GNN re-ranking on sparse rows: the algorithm of gnn_rerank.hip (same step numbers) with only the structural non-zeros
// stored, as CSR (row pointers int64, columns int32 strictly ascending inside a row, values fp32).  Nothing of size
// N x N or Q x G is allocated here (N = Q + G).  The sizes depend on the data, so every stage is its own call and the
// caller allocates between them (ieee_amd/rerank.py::_gnn_sparse):
//   1  rank, S: the caller's, from ieee_rank_topk_merge over column slabs of -X_u X_u^T
//   2  M0 = B + B^T          transpose(B), then symmetrise(B, B^T); B is the CSR view of rank: pointers i*k1, values 1
//   3  M1 = propagate(M0)    M1[i] = sum_{j<k2} S[i][j]^2 M0[rank[i][j]], j ascending per column; norm[i] = |M1[i]|
//   4  M0' = M1/n + (M1/n)^T transpose(M1) scaled by 1/n_r as it is filled, then symmetrise; n = max(norm, 1e-12)
//   5  R = propagate(M0')    unnormalised, with its norms
//   6  out[q][g] = 1 - <R_q, R_g> / (n_q n_g): per gallery range, transpose(R[Q+g0 .. Q+g1)) and one cosine kernel
// k2 = 1: R = B with sorted rows (a symmetrise with an empty transposed side), then step 6.
// symmetrise and propagate are one kernel (gs_gather_kernel): a fixed number of resident workgroups, each with an N-float
// scratch row and a bitmap of touched columns.  A row's sources are added one after the other with a barrier between
// (inside one source the columns are distinct: no conflicts, and a column's sum runs in source order: the dense kernel's
// arithmetic with the zero terms skipped), then the bitmap is walked in ascending order to emit and to clear.  A count
// pass (bitmap only) sizes the output, a scan gives the row pointers, a fill pass writes it.
// No floating-point atomics; the integer atomics (bitmap bits, transposed-list slots) decide no float's value: where
// slot order is arbitrary, every slot of a list goes to a different accumulator.  Same bits on every call.
#include "rank_common.h"

namespace ieee {

constexpr int GS_MAXK = 1024;                      // ieee_rank_topk's bound on k1
constexpr int GS_BLOCKS = 512;                     // resident workgroups of gs_gather_kernel
constexpr int GS_LDS_BITMAP_WORDS = 8192;          // bitmap in LDS up to N = 262 144, else in the scratch row
constexpr int GS_LDS_ACC = 16384;                  // step 6: range widths up to this accumulate in LDS (64 KiB)

__device__ __forceinline__ int gs_clamp(int c, int N) { return min(max(c, 0), N - 1); }

struct GsGather {
  int kind;                                        // 0 propagate, 1 symmetrise
  int N, k1, k2;
  const int64_t* aptr; const int* acol; const float* aval;      // the source rows (aval null: count pass)
  const int64_t* tptr; const int* trow; const float* tval;      // symmetrise: the transposed lists, already scaled
  const int* rank; const float* S;                 // propagate
  const float* anorm;                              // symmetrise: row norms of the source, or null (scale 1)
  float* scratch; int64_t sstride;
  int64_t* ocnt;                                   // count pass: entries of row r
  const int64_t* optr; int* ocol; float* oval; float* onorm; int64_t cap;   // fill pass
};

__device__ __forceinline__ unsigned gs_load_word(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One source segment [p0, p1) of (column, value) into the scratch row: acc[c] = fma(w, v, acc[c]) (w = 1 and acc = 0 or
// one earlier term in the symmetrise: exact either way), bit c set.
template <bool LDSBITS, bool DIVIDE>
__device__ __forceinline__ void gs_add_segment(const int* __restrict__ col, const float* __restrict__ val, int64_t p0,
                                               int64_t p1, float w, int N, float* acc, unsigned* lbits, unsigned* gbits) {
  for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) {
    const int c = gs_clamp(col[p], N);
    if (val) acc[c] = DIVIDE ? acc[c] + val[p] / w : fmaf(w, val[p], acc[c]);
    if (LDSBITS) atomicOr(lbits + (c >> 5), 1u << (c & 31));
    else atomicOr(gbits + (c >> 5), 1u << (c & 31));
  }
}

template <bool LDSBITS>
__global__ __launch_bounds__(256) void gs_gather_kernel(GsGather g) {
  extern __shared__ unsigned s_bits[];
  __shared__ uint32_t s_wsum[4];
  __shared__ float s_red[4];
  const int t = threadIdx.x, N = g.N;
  float* acc = g.scratch + (int64_t)blockIdx.x * g.sstride;
  unsigned* gbits = (unsigned*)(acc + N);
  const int W = (N + 31) >> 5, per = (W + 255) / 256;
  const int w0 = min(W, t * per), w1 = min(W, w0 + per);
  const bool fill = g.aval != nullptr;
  if (LDSBITS) {
    for (int w = t; w < W; w += 256) s_bits[w] = 0u;
    __syncthreads();
  }
  for (int r = blockIdx.x; r < N; r += gridDim.x) {
    if (g.kind == 0) {
      for (int j = 0; j < g.k2; ++j) {
        const int s = gs_clamp(g.rank[(int64_t)r * g.k1 + j], N);
        const float sc = fill ? g.S[(int64_t)r * g.k1 + j] : 0.f;
        gs_add_segment<LDSBITS, false>(g.acol, g.aval, g.aptr[s], g.aptr[s + 1], sc * sc, N, acc, s_bits, gbits);
        __syncthreads();
      }
    } else {
      const float n = fill && g.anorm ? fmaxf(g.anorm[r], 1e-12f) : 1.f;
      gs_add_segment<LDSBITS, true>(g.acol, g.aval, g.aptr[r], g.aptr[r + 1], n, N, acc, s_bits, gbits);
      __syncthreads();
      gs_add_segment<LDSBITS, false>(g.trow, fill ? g.tval : nullptr, g.tptr[r], g.tptr[r + 1], 1.f, N, acc, s_bits, gbits);
      __syncthreads();
    }
    uint32_t mine = 0, total;
    for (int w = w0; w < w1; ++w) mine += __popc(LDSBITS ? s_bits[w] : gs_load_word(gbits + w));
    int64_t off = block_scan_excl(mine, s_wsum, &total);
    float ss = 0.f;
    const int64_t base = fill ? g.optr[r] : 0;
    const int64_t room = fill ? min(g.optr[r + 1], g.cap) - base : 0;
    for (int w = w0; w < w1; ++w) {
      unsigned b = LDSBITS ? s_bits[w] : gs_load_word(gbits + w);
      if (!b) continue;
      if (LDSBITS) s_bits[w] = 0u; else atomicExch(gbits + w, 0u);
      if (!fill) continue;
      while (b) {
        const int c = w * 32 + __ffs(b) - 1;
        b &= b - 1;
        const float v = acc[c];
        acc[c] = 0.f;
        if (off < room) { g.ocol[base + off] = c; g.oval[base + off] = v; }
        ss = fmaf(v, v, ss);
        ++off;
      }
    }
    if (!fill) {
      if (t == 0) g.ocnt[r] = total;
    } else if (g.onorm) {
      ss = wave_sum(ss);
      if ((t & 63) == 0) s_red[t >> 6] = ss;
      __syncthreads();
      if (t == 0) g.onorm[r] = sqrtf((s_red[0] + s_red[1]) + (s_red[2] + s_red[3]));
    }
    __syncthreads();
  }
}

// a[0, n) counts -> exclusive prefix sums in place, a[n] = total (one block; a thread touches its own span only)
__global__ __launch_bounds__(1024) void gs_scan_kernel(int64_t* __restrict__ a, int n) {
  __shared__ int64_t s[1024];
  const int t = threadIdx.x, per = (n + 1023) / 1024;
  const int c0 = min(n, t * per), c1 = min(n, c0 + per);
  int64_t mine = 0;
  for (int c = c0; c < c1; ++c) mine += a[c];
  s[t] = mine;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int64_t add = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  int64_t run = s[t] - mine;
  for (int c = c0; c < c1; ++c) { const int64_t v = a[c]; a[c] = run; run += v; }
  if (t == 1023) a[n] = s[1023];
}

// transpose of rows [r0, r1): one wave per row.  Count, then (after the scan) fill: the slot inside a list is drawn
// from a counter, so a list's order is arbitrary -- its entries have distinct rows, and every reader sends them to
// distinct accumulators.
__global__ __launch_bounds__(256) void gs_tcount_kernel(const int64_t* __restrict__ ptr, const int* __restrict__ col,
                                                        int N, int r0, int r1, int64_t* __restrict__ cnt) {
  const int64_t r = (int64_t)r0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= r1) return;
  for (int64_t p = ptr[r] + (threadIdx.x & 63); p < ptr[r + 1]; p += 64)
    atomicAdd((unsigned long long*)(cnt + gs_clamp(col[p], N)), 1ull);
}

__global__ __launch_bounds__(256) void gs_tfill_kernel(const int64_t* __restrict__ ptr, const int* __restrict__ col,
                                                       const float* __restrict__ val, const float* __restrict__ norm,
                                                       int N, int r0, int r1, const int64_t* __restrict__ tptr,
                                                       int* __restrict__ cursor, int* __restrict__ trow,
                                                       float* __restrict__ tval, int64_t cap) {
  const int64_t r = (int64_t)r0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= r1) return;
  const float n = norm ? fmaxf(norm[r], 1e-12f) : 1.f;
  for (int64_t p = ptr[r] + (threadIdx.x & 63); p < ptr[r + 1]; p += 64) {
    const int c = gs_clamp(col[p], N);
    const int64_t q = tptr[c] + atomicAdd(cursor + c, 1);
    if (q < cap) { trow[q] = (int)r; tval[q] = val[p] / n; }
  }
}

// Step 6: one workgroup per query, the accumulator (LDS, or the output row itself) over the range's `width` gallery
// entries.  The columns of R_q go by in ascending order with a barrier after each, so the sum of one (q, g) runs in
// ascending column order however the gallery is cut into ranges; a list's entries are distinct gallery rows.
template <bool LDSACC>
__global__ __launch_bounds__(256) void gs_cosine_kernel(const int64_t* __restrict__ ptr, const int* __restrict__ col,
                                                        const float* __restrict__ val, const float* __restrict__ norm,
                                                        const int64_t* __restrict__ tptr, const int* __restrict__ trow,
                                                        const float* __restrict__ tval, int N, int first, int width,
                                                        float* __restrict__ out, int64_t ldo) {
  extern __shared__ float s_acc[];
  const int q = blockIdx.x, t = threadIdx.x;
  float* row = out + (int64_t)q * ldo;
  for (int g = t; g < width; g += 256) { if (LDSACC) s_acc[g] = 0.f; else row[g] = 0.f; }
  __syncthreads();
  const int64_t p1 = ptr[q + 1];
  for (int64_t p = ptr[q]; p < p1; ++p) {
    const int c = gs_clamp(col[p], N);
    const int64_t s0 = tptr[c], s1 = tptr[c + 1];
    if (s0 == s1) continue;                        // the same for every thread
    const float a = val[p];
    for (int64_t s = s0 + t; s < s1; s += 256) {
      const unsigned g = (unsigned)(trow[s] - first);
      if (g >= (unsigned)width) continue;
      if (LDSACC) s_acc[g] = fmaf(a, tval[s], s_acc[g]); else row[g] = fmaf(a, tval[s], row[g]);
    }
    __syncthreads();
  }
  const float nq = fmaxf(norm[q], 1e-12f);
  for (int g = t; g < width; g += 256) {
    const float dot = LDSACC ? s_acc[g] : row[g];
    row[g] = 1.f - dot / (nq * fmaxf(norm[first + g], 1e-12f));
  }
}

static const char* gs_check(int64_t Q, int64_t G, int64_t k1, int64_t k2) {
  if (Q <= 0 || G <= 0) return "empty query or gallery set";
  if (Q >= ((int64_t)1 << 30) || G >= ((int64_t)1 << 30)) return "Q+G must stay below 2^31";
  if (k1 < 1 || k1 > GS_MAXK || k1 > Q + G) return "k1 out of range (1..1024, <= Q+G)";
  if (k2 < 1 || k2 > k1) return "k2 out of range (1..k1)";
  return nullptr;
}

static inline int64_t gs_sstride(int64_t N) { return (N + (N + 31) / 32 + 63) & ~(int64_t)63; }   // floats, 256-byte rows
static inline int64_t gs_blocks(int64_t N) { return N < GS_BLOCKS ? N : GS_BLOCKS; }
static inline int64_t gs_scratch_bytes(int64_t N) { return gs_blocks(N) * gs_sstride(N) * 4; }

static int gs_gather(GsGather g, hipStream_t st, const char* what) {
  const int W = (g.N + 31) >> 5;
  if (W <= GS_LDS_BITMAP_WORDS) gs_gather_kernel<true><<<(unsigned)gs_blocks(g.N), 256, sizeof(unsigned) * W, st>>>(g);
  else gs_gather_kernel<false><<<(unsigned)gs_blocks(g.N), 256, 0, st>>>(g);
  return launch_status(what);
}

static int gs_scan(int64_t* a, int64_t n, hipStream_t st) {
  gs_scan_kernel<<<1, 1024, 0, st>>>(a, (int)n);
  return launch_status("gs_scan_kernel");
}

}  // namespace ieee

using namespace ieee;

#define GS_ARGS(who, N, scratch_bytes)                                                                          \
  IEEE_REQUIRE((N) >= 1 && (N) < ((int64_t)1 << 31), who ": N = %ld out of range (1 .. 2^31 - 1)", (long)(N)); \
  IEEE_REQUIRE((scratch_bytes) >= gs_scratch_bytes(N), who ": scratch too small (%ld < %ld bytes)",              \
               (long)(scratch_bytes), (long)gs_scratch_bytes(N))

extern "C" int64_t ieee_gnn_sparse_scratch_bytes(int64_t Q, int64_t G, int64_t k1, int64_t k2) {
  if (const char* why = gs_check(Q, G, k1, k2)) {
    set_error(IEEE_ERR_BAD_ARG, "gnn_sparse: %s (Q=%ld G=%ld k1=%ld k2=%ld)", why, (long)Q, (long)G, (long)k1, (long)k2);
    return -1;
  }
  return gs_scratch_bytes(Q + G);
}

extern "C" int ieee_gnn_sparse_transpose(const int64_t* rowptr, const int32_t* col, const float* val, const float* norm,
                                         int64_t N, int64_t r0, int64_t r1, int32_t* cursor, int64_t* tptr,
                                         int32_t* trow, float* tval, int64_t cap, void* stream) {
  IEEE_REQUIRE(rowptr && col && val && cursor && tptr && trow && tval, "gnn_sparse_transpose: null pointer");
  IEEE_REQUIRE(N >= 1 && N < ((int64_t)1 << 31), "gnn_sparse_transpose: N = %ld out of range (1 .. 2^31 - 1)", (long)N);
  IEEE_REQUIRE(0 <= r0 && r0 <= r1 && r1 <= N && cap >= 0, "gnn_sparse_transpose: rows [%ld, %ld) of %ld, cap %ld",
               (long)r0, (long)r1, (long)N, (long)cap);
  hipStream_t st = (hipStream_t)stream;
  IEEE_HIP(hipMemsetAsync(tptr, 0, sizeof(int64_t) * (size_t)(N + 1), st));
  IEEE_HIP(hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t)N, st));
  if (r1 > r0) {
    gs_tcount_kernel<<<cdiv(r1 - r0, 4), 256, 0, st>>>(rowptr, col, (int)N, (int)r0, (int)r1, tptr);
    IEEE_TRY(launch_status("gs_tcount_kernel"));
  }
  IEEE_TRY(gs_scan(tptr, N, st));
  if (r1 > r0) {
    gs_tfill_kernel<<<cdiv(r1 - r0, 4), 256, 0, st>>>(rowptr, col, val, norm, (int)N, (int)r0, (int)r1, tptr, cursor, trow,
                                                     tval, cap);
    IEEE_TRY(launch_status("gs_tfill_kernel"));
  }
  return IEEE_OK;
}

extern "C" int ieee_gnn_sparse_symmetrise_count(const int64_t* rowptr, const int32_t* col, const int64_t* tptr,
                                                const int32_t* trow, int64_t N, void* scratch, int64_t scratch_bytes,
                                                int64_t* out_rowptr, void* stream) {
  IEEE_REQUIRE(rowptr && col && tptr && trow && scratch && out_rowptr, "gnn_sparse_symmetrise_count: null pointer");
  GS_ARGS("gnn_sparse_symmetrise_count", N, scratch_bytes);
  GsGather g = {};
  g.kind = 1; g.N = (int)N;
  g.aptr = rowptr; g.acol = col; g.tptr = tptr; g.trow = trow;
  g.scratch = (float*)scratch; g.sstride = gs_sstride(N); g.ocnt = out_rowptr;
  IEEE_TRY(gs_gather(g, (hipStream_t)stream, "gs_gather_kernel (symmetrise, count)"));
  return gs_scan(out_rowptr, N, (hipStream_t)stream);
}

extern "C" int ieee_gnn_sparse_symmetrise_fill(const int64_t* rowptr, const int32_t* col, const float* val,
                                               const float* norm, const int64_t* tptr, const int32_t* trow,
                                               const float* tval, int64_t N, void* scratch, int64_t scratch_bytes,
                                               const int64_t* out_rowptr, int32_t* out_col, float* out_val,
                                               float* out_norm, int64_t cap, void* stream) {
  IEEE_REQUIRE(rowptr && col && val && tptr && trow && tval && scratch && out_rowptr && out_col && out_val,
               "gnn_sparse_symmetrise_fill: null pointer");
  GS_ARGS("gnn_sparse_symmetrise_fill", N, scratch_bytes);
  IEEE_REQUIRE(cap >= 0, "gnn_sparse_symmetrise_fill: cap %ld", (long)cap);
  GsGather g = {};
  g.kind = 1; g.N = (int)N;
  g.aptr = rowptr; g.acol = col; g.aval = val; g.anorm = norm; g.tptr = tptr; g.trow = trow; g.tval = tval;
  g.scratch = (float*)scratch; g.sstride = gs_sstride(N);
  g.optr = out_rowptr; g.ocol = out_col; g.oval = out_val; g.onorm = out_norm; g.cap = cap;
  return gs_gather(g, (hipStream_t)stream, "gs_gather_kernel (symmetrise, fill)");
}

extern "C" int ieee_gnn_sparse_propagate_count(const int64_t* rowptr, const int32_t* col, const int32_t* rank, int64_t N,
                                               int64_t k1, int64_t k2, void* scratch, int64_t scratch_bytes,
                                               int64_t* out_rowptr, void* stream) {
  IEEE_REQUIRE(rowptr && col && rank && scratch && out_rowptr, "gnn_sparse_propagate_count: null pointer");
  GS_ARGS("gnn_sparse_propagate_count", N, scratch_bytes);
  IEEE_REQUIRE(k1 >= 1 && k1 <= GS_MAXK && k1 <= N, "gnn_sparse_propagate_count: k1 %ld out of range (1..1024, <= N)", (long)k1);
  IEEE_REQUIRE(k2 >= 1 && k2 <= k1, "gnn_sparse_propagate_count: k2 %ld out of range (1..k1)", (long)k2);
  GsGather g = {};
  g.kind = 0; g.N = (int)N; g.k1 = (int)k1; g.k2 = (int)k2;
  g.aptr = rowptr; g.acol = col; g.rank = rank;
  g.scratch = (float*)scratch; g.sstride = gs_sstride(N); g.ocnt = out_rowptr;
  IEEE_TRY(gs_gather(g, (hipStream_t)stream, "gs_gather_kernel (propagate, count)"));
  return gs_scan(out_rowptr, N, (hipStream_t)stream);
}

extern "C" int ieee_gnn_sparse_propagate_fill(const int64_t* rowptr, const int32_t* col, const float* val,
                                              const int32_t* rank, const float* S, int64_t N, int64_t k1, int64_t k2,
                                              void* scratch, int64_t scratch_bytes, const int64_t* out_rowptr,
                                              int32_t* out_col, float* out_val, float* out_norm, int64_t cap,
                                              void* stream) {
  IEEE_REQUIRE(rowptr && col && val && rank && S && scratch && out_rowptr && out_col && out_val && out_norm,
               "gnn_sparse_propagate_fill: null pointer");
  GS_ARGS("gnn_sparse_propagate_fill", N, scratch_bytes);
  IEEE_REQUIRE(k1 >= 1 && k1 <= GS_MAXK && k1 <= N, "gnn_sparse_propagate_fill: k1 %ld out of range (1..1024, <= N)", (long)k1);
  IEEE_REQUIRE(k2 >= 1 && k2 <= k1, "gnn_sparse_propagate_fill: k2 %ld out of range (1..k1)", (long)k2);
  IEEE_REQUIRE(cap >= 0, "gnn_sparse_propagate_fill: cap %ld", (long)cap);
  GsGather g = {};
  g.kind = 0; g.N = (int)N; g.k1 = (int)k1; g.k2 = (int)k2;
  g.aptr = rowptr; g.acol = col; g.aval = val; g.rank = rank; g.S = S;
  g.scratch = (float*)scratch; g.sstride = gs_sstride(N);
  g.optr = out_rowptr; g.ocol = out_col; g.oval = out_val; g.onorm = out_norm; g.cap = cap;
  return gs_gather(g, (hipStream_t)stream, "gs_gather_kernel (propagate, fill)");
}

extern "C" int ieee_gnn_sparse_cosine(const int64_t* rowptr, const int32_t* col, const float* val, const float* norm,
                                      const int64_t* tptr, const int32_t* trow, const float* tval, int64_t Q, int64_t G,
                                      int64_t g0, int64_t g1, float* out, int64_t ldo, void* stream) {
  IEEE_REQUIRE(rowptr && col && val && norm && tptr && trow && tval && out, "gnn_sparse_cosine: null pointer");
  IEEE_REQUIRE(Q >= 1 && G >= 1 && Q < ((int64_t)1 << 30) && G < ((int64_t)1 << 30),
               "gnn_sparse_cosine: Q = %ld, G = %ld out of range (1 .. 2^30 - 1)", (long)Q, (long)G);
  IEEE_REQUIRE(0 <= g0 && g0 < g1 && g1 <= G && ldo >= g1 - g0, "gnn_sparse_cosine: range [%ld, %ld) of %ld, ldo %ld",
               (long)g0, (long)g1, (long)G, (long)ldo);
  hipStream_t st = (hipStream_t)stream;
  const int width = (int)(g1 - g0), N = (int)(Q + G), first = (int)(Q + g0);
  if (width <= GS_LDS_ACC)
    gs_cosine_kernel<true><<<(unsigned)Q, 256, sizeof(float) * width, st>>>(rowptr, col, val, norm, tptr, trow, tval, N, first,
                                                                             width, out, ldo);
  else
    gs_cosine_kernel<false><<<(unsigned)Q, 256, 0, st>>>(rowptr, col, val, norm, tptr, trow, tval, N, first, width, out, ldo);
  return launch_status("gs_cosine_kernel");
}
