// GNN re-ranking (the reference's torchreid/utils/GPU-Re-Ranking: gnn_reranking.py:27-59 and its two CUDA kernels,
// build_adjacency_matrix and gnn_propagate), dense, in two N x ld fp32 matrices M0 and M1 (N = Q + G, ld = N rounded
// up to 8, pad columns zero so that a row can be an operand of ieee_sqeuclid_distmat):
//   1  M1 = -X_u X_u^T (distmat metric 2; four blocks when the query and gallery rows are separate arrays);
//      rank, S = ieee_rank_topk(M1, k1): (score descending, index ascending), S = -score
//   2  M0 = B + B^T, B[i][rank[i][j]] = 1                                 memset + 2 N k1 exact float adds
//   3  M1[i] = sum_{j<k2} S[i][j]^2 M0[rank[i][j]], j ascending; ss[i] = |M1[i]|^2     whole-row gather
//   4  M0[i][j] = M1[i][j]/n_i + M1[j][i]/n_j, n = max(sqrt(ss), 1e-12)    normalise and symmetrise in one pass
//   5  step 3 again (the second round's rows stay unnormalised in M1)
//   6  out = 1 - cos(M1[:Q], M1[Q:])  (distmat metric 1: its epilogue normalises, eps 1e-12)
// k2 = 1 skips 3-5: M0 = B (plain stores) and out = 1 - cos(B[:Q], B[Q:]) = 1 - shared/k1.
// Nothing here depends on the order in which workgroups run: the only float atomics add 1.0 to sums below 3.
#include <algorithm>

#include "common.h"

namespace ieee {

constexpr int GNN_MAXK = 1024;                     // ieee_rank_topk's bound on k1

// Step 2.  One thread per (i, j).  rank comes from ieee_rank_topk over N >= k1 columns, so it lies in [0, N); the
// clamp keeps any bits memory-safe.
__global__ __launch_bounds__(256) void gnn_adjacency_kernel(const int* __restrict__ rank, int64_t total, int N, int ld,
                                                            int k1, int symmetric, float* __restrict__ A) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int i = (int)(e / k1);
  const int r = min(max(rank[e], 0), N - 1);
  if (symmetric) {
    atomicAdd(A + (int64_t)i * ld + r, 1.f);
    atomicAdd(A + (int64_t)r * ld + i, 1.f);
  } else {
    A[(int64_t)i * ld + r] = 1.f;                  // the k1 columns of one row are distinct
  }
}

// Steps 3 and 5.  One workgroup per row, a thread owns 16-byte column chunks and walks the k2 source rows in j order
// (four loads in flight).  Handing each XCD a contiguous range of rows instead of every eighth one (neighbouring rows
// share neighbours) was tried once and changed nothing measurable at Q+G = 23 100 (LABNOTES.md): not kept.
__global__ __launch_bounds__(256) void gnn_propagate_kernel(const float* __restrict__ A, float* __restrict__ P,
                                                            const int* __restrict__ rank, const float* __restrict__ S,
                                                            int N, int ld, int k1, int k2,
                                                            float* __restrict__ sumsq) {
  __shared__ int r[GNN_MAXK];
  __shared__ float w[GNN_MAXK];
  __shared__ float red[4];
  const int t = threadIdx.x, i = blockIdx.x;
  for (int j = t; j < k2; j += 256) {
    r[j] = min(max(rank[(int64_t)i * k1 + j], 0), N - 1);
    const float s = S[(int64_t)i * k1 + j];
    w[j] = s * s;
  }
  __syncthreads();
  float ss = 0.f;
  for (int c = t * 4; c < ld; c += 1024) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int j = 0;
    for (; j + 4 <= k2; j += 4) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *(const f32x4*)(A + (int64_t)r[j + u] * ld + c);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc += w[j + u] * v[u];
    }
    for (; j < k2; ++j) acc += w[j] * *(const f32x4*)(A + (int64_t)r[j] * ld + c);
    *(f32x4*)(P + (int64_t)i * ld + c) = acc;
    ss += (acc[0] * acc[0] + acc[1] * acc[1]) + (acc[2] * acc[2] + acc[3] * acc[3]);
  }
  ss = wave_sum(ss);
  if ((t & 63) == 0) red[t >> 6] = ss;
  __syncthreads();
  if (t == 0) sumsq[i] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Step 4.  A 64 x 64 tile (I, J) of the output needs tile (I, J) and tile (J, I) of P: both are read by rows, the
// second goes through LDS (row stride 65 words: the transposed read walks the banks) and comes back transposed.
__global__ __launch_bounds__(256) void gnn_normsym_kernel(const float* __restrict__ P, const float* __restrict__ sumsq,
                                                          float* __restrict__ A, int N, int ld) {
  __shared__ float T[64][65];
  __shared__ float nI[64], nJ[64];
  const int t = threadIdx.x, c4 = (t & 15) * 4, r0 = t >> 4;
  const int I0 = blockIdx.y * 64, J0 = blockIdx.x * 64;
  if (t < 64) nI[t] = I0 + t < N ? fmaxf(sqrtf(sumsq[I0 + t]), 1e-12f) : 1.f;
  else if (t < 128) nJ[t - 64] = J0 + t - 64 < N ? fmaxf(sqrtf(sumsq[J0 + t - 64]), 1e-12f) : 1.f;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int rr = r0 + 16 * p, j = J0 + rr, col = I0 + c4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (j < N && col < ld) v = *(const f32x4*)(P + (int64_t)j * ld + col);
#pragma unroll
    for (int e = 0; e < 4; ++e) T[rr][c4 + e] = v[e];
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int rr = r0 + 16 * p, i = I0 + rr, col = J0 + c4;
    if (i >= N || col >= ld) continue;             // ld % 8 == 0: a chunk that starts inside the row ends inside it
    const f32x4 a = *(const f32x4*)(P + (int64_t)i * ld + col);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = col + e < N ? a[e] / nI[rr] + T[c4 + e][rr] / nJ[c4 + e] : 0.f;
    *(f32x4*)(A + (int64_t)i * ld + col) = o;
  }
}

// Workspace plan: one function for the query, the layout and the launch.
struct GnnPlan {
  int64_t N, ld, rank, s, sumsq, dwork, dwork_bytes, m0, m1, total;
};

static const char* gnn_plan(int64_t Q, int64_t G, int64_t d, int64_t k1, int64_t k2, int precision, GnnPlan& p) {
  if (Q <= 0 || G <= 0) return "empty query or gallery set";
  if (d <= 0 || d % 8 != 0) return "feature dim must be a positive multiple of 8";
  if (Q >= ((int64_t)1 << 30) || G >= ((int64_t)1 << 30)) return "Q+G must stay below 2^31";
  const int64_t N = Q + G;
  if (k1 < 1 || k1 > GNN_MAXK || k1 > N) return "k1 out of range (1..1024, <= Q+G)";
  if (k2 < 1 || k2 > k1) return "k2 out of range (1..k1)";
  if (precision != 0 && precision != IEEE_SPLIT_BF16X3 && precision != IEEE_SPLIT_BF16X2 && precision != IEEE_SPLIT_F16X2)
    return "unknown precision (0 = fp32, or IEEE_SPLIT_BF16X3 / _BF16X2 / _F16X2)";
  p.N = N;
  p.ld = (N + 7) & ~(int64_t)7;
  if (precision == 0) {
    p.dwork_bytes = 2 * N * 4;                     // row norms of the largest call
  } else {
    p.dwork_bytes = std::max(ieee_sqeuclid_distmat_split_workspace_bytes(N, N, d, precision),
                             ieee_sqeuclid_distmat_split_workspace_bytes(Q, G, p.ld, precision));
  }
  int64_t at = 0;
  auto take = [&](int64_t bytes) { const int64_t a = at; at += align256(bytes); return a; };
  p.rank = take(N * k1 * 4);
  p.s = take(N * k1 * 4);
  p.sumsq = take(N * 4);
  p.dwork = take(p.dwork_bytes);
  p.m0 = take(N * p.ld * 4);
  p.m1 = take(N * p.ld * 4);
  p.total = at;
  return nullptr;
}

}  // namespace ieee

using namespace ieee;

extern "C" int64_t ieee_gnn_rerank_workspace_bytes(int64_t Q, int64_t G, int64_t d, int64_t k1, int64_t k2, int precision) {
  GnnPlan p;
  if (const char* why = gnn_plan(Q, G, d, k1, k2, precision, p)) {
    set_error(IEEE_ERR_BAD_ARG, "gnn_rerank: %s (Q=%ld G=%ld d=%ld k1=%ld k2=%ld precision=%d)", why, (long)Q, (long)G,
              (long)d, (long)k1, (long)k2, precision);
    return -1;
  }
  return p.total;
}

extern "C" int ieee_gnn_rerank_layout(int64_t Q, int64_t G, int64_t d, int64_t k1, int64_t k2, int precision,
                                      int64_t* fields) {
  GnnPlan p;
  IEEE_REQUIRE(fields, "gnn_rerank_layout: null pointer");
  const char* why = gnn_plan(Q, G, d, k1, k2, precision, p);
  IEEE_REQUIRE(!why, "gnn_rerank_layout: %s", why);
  const int64_t v[] = {p.ld, p.rank, p.s, p.sumsq, p.m0, p.m1, k2 == 1 ? p.m0 : p.m1};
  for (int k = 0; k < 7; ++k) fields[k] = v[k];
  return IEEE_OK;
}

extern "C" int ieee_gnn_rerank(const float* xq, const float* xg, int64_t Q, int64_t G, int64_t d, int64_t k1, int64_t k2,
                               int precision, float* out, void* work, int64_t work_bytes, void* stream) {
  IEEE_REQUIRE(xq && xg && out && work, "gnn_rerank: null pointer");
  GnnPlan p;
  const char* why = gnn_plan(Q, G, d, k1, k2, precision, p);
  IEEE_REQUIRE(!why, "gnn_rerank: %s (Q=%ld G=%ld d=%ld k1=%ld k2=%ld precision=%d)", why, (long)Q, (long)G, (long)d,
               (long)k1, (long)k2, precision);
  IEEE_REQUIRE(work_bytes >= p.total, "gnn_rerank: workspace too small (%ld < %ld bytes)", (long)work_bytes, (long)p.total);
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)work;
  int* rank = (int*)(w + p.rank);
  float* S = (float*)(w + p.s);
  float* sumsq = (float*)(w + p.sumsq);
  void* dwork = w + p.dwork;
  float *M0 = (float*)(w + p.m0), *M1 = (float*)(w + p.m1);
  const int N = (int)p.N, ld = (int)p.ld;
  auto gemm = [&](const float* a, const float* b, int64_t m, int64_t n, int64_t dd, int metric, float* o, int64_t ldo) {
    return precision == 0 ? ieee_sqeuclid_distmat(a, b, m, n, dd, IEEE_F32, metric, o, ldo, dwork, stream)
                          : ieee_sqeuclid_distmat_split(a, b, m, n, dd, precision, metric, o, ldo, dwork, p.dwork_bytes,
                                                        stream);
  };

  // 1: -X_u X_u^T, then the k1 best of every row.  Gallery rows that follow the query rows in memory make X_u one
  // array and the scores one GEMM; otherwise four blocks (at 836 + 836 rows four launches of 49 tiles each fill a
  // fifth of the device: the whole call took 1.06 ms that way and 0.52 ms with one launch of 196 tiles)
  if (xg == xq + Q * d) {
    IEEE_TRY(gemm(xq, xq, N, N, d, 2, M1, ld));
  } else {
    IEEE_TRY(gemm(xq, xq, Q, Q, d, 2, M1, ld));
    IEEE_TRY(gemm(xq, xg, Q, G, d, 2, M1 + Q, ld));
    IEEE_TRY(gemm(xg, xq, G, Q, d, 2, M1 + Q * (int64_t)ld, ld));
    IEEE_TRY(gemm(xg, xg, G, G, d, 2, M1 + Q * (int64_t)ld + Q, ld));
  }
  IEEE_TRY(ieee_rank_topk(M1, ld, N, N, nullptr, nullptr, nullptr, nullptr, 0, k1, rank, S, stream));
  // 2
  IEEE_HIP(hipMemsetAsync(M0, 0, sizeof(float) * (size_t)N * ld, st));
  const int64_t pairs = (int64_t)N * k1;
  gnn_adjacency_kernel<<<cdiv(pairs, 256), 256, 0, st>>>(rank, pairs, N, ld, (int)k1, k2 != 1, M0);
  IEEE_TRY(launch_status("gnn_adjacency_kernel"));
  const float* rows = M0;
  if (k2 != 1) {
    gnn_propagate_kernel<<<N, 256, 0, st>>>(M0, M1, rank, S, N, ld, (int)k1, (int)k2, sumsq);
    IEEE_TRY(launch_status("gnn_propagate_kernel"));
    gnn_normsym_kernel<<<dim3(cdiv(ld, 64), cdiv(N, 64)), 256, 0, st>>>(M1, sumsq, M0, N, ld);
    IEEE_TRY(launch_status("gnn_normsym_kernel"));
    gnn_propagate_kernel<<<N, 256, 0, st>>>(M0, M1, rank, S, N, ld, (int)k1, (int)k2, sumsq);
    IEEE_TRY(launch_status("gnn_propagate_kernel"));
    rows = M1;
  }
  // 6
  return gemm(rows, rows + Q * (int64_t)ld, Q, G, ld, 1, out, G);
}
