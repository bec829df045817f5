// Exact (dense, O(N^2)) t-SNE in two output dimensions, Student-t degree of freedom 1: the figure the reference's
// evaluator draws (torchreid/engine/engine.py:463-490 calls sklearn.manifold.TSNE once per 768-wide descriptor slice).
// `batch` independent problems of the same n run per call, on a grid axis.
//   affinities  one workgroup per row: the row of squared distances sits in LDS for the whole perplexity search
//               (n <= 12 288: 48 KiB, three workgroups per CU), the conditional row p_{j|i} goes straight into P, and a
//               second kernel symmetrises P in place, tile pair by tile pair
//   run         per iteration two launches: tsne_force_kernel (one wave per row and 512-column slab: one pass over P,
//               six partial sums per row and slab) and tsne_update_kernel (one workgroup per problem: slabs summed in
//               ascending order, Z, the gains / momentum update, the history entry)
// Every sum has a fixed order (lane-sequential, shuffle butterfly, LDS in wave order, slabs ascending) and there are no
// atomics: two calls give the same bits.  Nothing reads back to the host.
#include "common.h"

namespace ieee {

constexpr int TSNE_MAX_N = 12288;                  // the LDS row of the search; P for batch = 3 is then 1.7 GiB
constexpr int TSNE_SLAB = 512;                     // columns per force workgroup: 2 x (64 lanes x 4)
constexpr int TSNE_SUMS = 6;                       // per row: attraction x, y; repulsion x, y; sum w; sum P log(1 + d^2)
constexpr int TSNE_UPD = 1024;                     // threads of the update workgroup

// (a, b) -> block sums, the same in every thread.  red: 2 x 8 floats, `parity` alternates between calls so that one
// barrier per call is enough (a thread that writes parity p again has passed the barrier of the call in between).
__device__ __forceinline__ void block_sum2_256(float& a, float& b, float* red, int parity) {
  a = wave_sum(a);
  b = wave_sum(b);
  float* r = red + parity * 8;
  const int t = threadIdx.x;
  if ((t & 63) == 0) {
    r[t >> 6] = a;
    r[4 + (t >> 6)] = b;
  }
  __syncthreads();
  a = (r[0] + r[1]) + (r[2] + r[3]);
  b = (r[4] + r[5]) + (r[6] + r[7]);
}

// sklearn/manifold/_utils.pyx::_binary_search_perplexity for one row, on d'_j = d_j - min_{k != i} d_k.  The exponent
// argument beta * d' is formed in double and rounded once, so that an element of the row carries one rounding of an
// argument below 88, the exponential and the division, whatever the scale of the distances.
__global__ __launch_bounds__(256) void tsne_search_kernel(const float* __restrict__ dist, int64_t ldd, int n,
                                                          float log_perplexity, float* __restrict__ P, int64_t ldp,
                                                          float* __restrict__ beta_out) {
  extern __shared__ float drow[];                  // n floats
  __shared__ float red[16];
  const int t = threadIdx.x, i = blockIdx.x;
  const int64_t row = (int64_t)blockIdx.y * n + i;
  const float* d = dist + row * ldd;
  float lo = INFINITY;
  for (int j = t; j < n; j += 256) {
    const float v = d[j];
    drow[j] = v;
    if (j != i) lo = fminf(lo, v);
  }
  lo = wave_max(-lo);
  if ((t & 63) == 0) red[t >> 6] = lo;
  __syncthreads();                                 // also: drow is complete
  const double dmin = -(double)fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();                                 // red is reused by the sums

  float beta = 1.f, beta_min = -INFINITY, beta_max = INFINITY;
  int parity = 0;
  for (int step = 0; step < 100; ++step) {
    const double b = (double)beta;
    float S = 0.f, T = 0.f;
    for (int j = t; j < n; j += 256) {
      if (j == i) continue;
      const float a = (float)(b * ((double)drow[j] - dmin));
      const float e = expf(-a);
      S += e;
      T += a * e;
    }
    block_sum2_256(S, T, red, parity);
    parity ^= 1;
    const float diff = (logf(S) + T / S) - log_perplexity;      // S >= 1: the nearest neighbour's term is exp(0)
    if (fabsf(diff) <= 1e-5f) break;
    if (diff > 0.f) {
      beta_min = beta;
      beta = beta_max == INFINITY ? beta * 2.f : (beta + beta_max) * 0.5f;
    } else {
      beta_max = beta;
      beta = beta_min == -INFINITY ? beta * 0.5f : (beta + beta_min) * 0.5f;
    }
  }
  // the row for the beta that is returned (after 100 steps without a hit sklearn keeps the row of the beta before)
  const double b = (double)beta;
  float S = 0.f, unused = 0.f;
  for (int j = t; j < n; j += 256)
    if (j != i) S += expf(-(float)(b * ((double)drow[j] - dmin)));
  block_sum2_256(S, unused, red, parity);
  float* p = P + row * ldp;
  for (int j = t; j < (int)ldp; j += 256)
    p[j] = (j < n && j != i) ? expf(-(float)(b * ((double)drow[j] - dmin))) / S : 0.f;
  if (t == 0) beta_out[row] = beta;
}

// P_ij = (p_{j|i} + p_{i|j}) / (2n), in place.  Workgroup (I, J), I <= J, owns the 64 x 64 tiles (I, J) and (J, I): both
// are read by rows into LDS (row stride 65 words: the transposed reads walk the banks), and each of the two outputs is
// the same sum of the same two numbers, so P comes out bitwise symmetric.
__global__ __launch_bounds__(256) void tsne_symmetrize_kernel(float* __restrict__ P, int64_t ldp, int n) {
  __shared__ float A[64][65], B[64][65];
  if (blockIdx.x < blockIdx.y) return;
  const int t = threadIdx.x, c = t & 63, r0 = t >> 6;
  const int I0 = blockIdx.y * 64, J0 = blockIdx.x * 64;
  float* Pb = P + (int64_t)blockIdx.z * n * ldp;
  const float den = 2.f * (float)n;
#pragma unroll 4
  for (int p = 0; p < 16; ++p) {
    const int r = r0 + 4 * p;
    A[r][c] = (I0 + r < n && J0 + c < n) ? Pb[(int64_t)(I0 + r) * ldp + J0 + c] : 0.f;
    B[r][c] = (J0 + r < n && I0 + c < n) ? Pb[(int64_t)(J0 + r) * ldp + I0 + c] : 0.f;
  }
  __syncthreads();
#pragma unroll 4
  for (int p = 0; p < 16; ++p) {
    const int r = r0 + 4 * p;
    if (I0 + r < n && J0 + c < n) Pb[(int64_t)(I0 + r) * ldp + J0 + c] = (A[r][c] + B[c][r]) / den;
    if (J0 + r < n && I0 + c < n) Pb[(int64_t)(J0 + r) * ldp + I0 + c] = (A[c][r] + B[r][c]) / den;
  }
}

// One wave per row: sum_j P log P and sum_j P, the terms of the KL divergence that no iteration changes.
__global__ __launch_bounds__(256) void tsne_rowconst_kernel(const float* __restrict__ P, int64_t ldp, int n,
                                                            float* __restrict__ rowconst, int64_t batch_stride) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const float* p = P + ((int64_t)blockIdx.y * n + i) * ldp;
  float plogp = 0.f, sum = 0.f;
  for (int j = lane * 4; j < n; j += 256) {
    const f32x4 v = *(const f32x4*)(p + j);        // ldp % 4 == 0: the chunk ends inside the row
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = (j + e < n && j + e != i) ? v[e] : 0.f;
      if (x > 0.f) plogp += x * logf(x);
      sum += x;
    }
  }
  plogp = wave_sum(plogp);
  sum = wave_sum(sum);
  if (lane == 0) {
    float* o = rowconst + blockIdx.y * batch_stride;
    o[i] = plogp;
    o[n + i] = sum;
  }
}

// The pairwise pass.  Wave (row i, slab s) walks columns [512 s, 512 s + 512): a lane takes 4 consecutive columns per
// step (one 16-byte load of P), two steps per slab, and the six sums leave through a shuffle butterfly.
// part[batch][slab][6][n].
template <bool KL>
__global__ __launch_bounds__(256) void tsne_force_kernel(const float* __restrict__ P, int64_t ldp, int n,
                                                         const float* __restrict__ Y, float* __restrict__ part,
                                                         int64_t batch_stride) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;                              // whole waves: no barrier below
  const int bz = blockIdx.z, slab = blockIdx.y;
  const float* p = P + ((int64_t)bz * n + i) * ldp;
  const float2* y = (const float2*)Y + (int64_t)bz * n;
  const float2 yi = y[i];
  float ax = 0.f, ay = 0.f, rx = 0.f, ry = 0.f, ws = 0.f, kl = 0.f;
#pragma unroll
  for (int it = 0; it < TSNE_SLAB / 256; ++it) {
    const int j = slab * TSNE_SLAB + (it * 64 + lane) * 4;
    if (j >= n) break;
    const f32x4 v = *(const f32x4*)(p + j);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool on = j + e < n && j + e != i;
      const float2 yj = y[min(j + e, n - 1)];
      const float dx = yi.x - yj.x, dy = yi.y - yj.y;
      const float d2 = dx * dx + dy * dy;
      const float q = 1.f + d2;
      const float w = on ? 1.f / q : 0.f;
      const float pw = on ? v[e] * w : 0.f;
      const float ww = w * w;
      ax += pw * dx;
      ay += pw * dy;
      rx += ww * dx;
      ry += ww * dy;
      ws += w;
      if (KL) kl += on ? v[e] * log1pf(d2) : 0.f;      // not logf(q): at |y| ~ 1e-4, d2 is far below an ulp of 1
    }
  }
  ax = wave_sum(ax); ay = wave_sum(ay); rx = wave_sum(rx); ry = wave_sum(ry); ws = wave_sum(ws);
  if (KL) kl = wave_sum(kl);
  if (lane == 0) {
    float* o = part + bz * batch_stride + (int64_t)slab * TSNE_SUMS * n + i;
    o[0] = ax; o[n] = ay; o[2 * (int64_t)n] = rx; o[3 * (int64_t)n] = ry; o[4 * (int64_t)n] = ws;
    o[5 * (int64_t)n] = kl;
  }
}

__device__ __forceinline__ float block_sum_1024(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();                                 // the previous call's readers are done with red
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < TSNE_UPD / 64; ++k) s += red[k];
  return s;
}

// One workgroup per problem.  Pass 1 sums every row's slabs in ascending order into rows[6][n] and, over the rows, Z and
// the KL terms; pass 2 is sklearn's _gradient_descent step for every coordinate.  scal[8] = {Z, sum P log(1 + d^2),
// sum P log P, sum P, |g|^2, ...}.
__global__ __launch_bounds__(TSNE_UPD) void tsne_update_kernel(const float* __restrict__ part, int nslab, int n,
                                                               int64_t part_stride, float* __restrict__ rows,
                                                               const float* __restrict__ rowconst,
                                                               float* __restrict__ scal, float* __restrict__ Y,
                                                               float* __restrict__ update, float* __restrict__ gains,
                                                               float alpha, float momentum, float lr,
                                                               float* __restrict__ history, int64_t hist_stride) {
  __shared__ float red[TSNE_UPD / 64];
  const int t = threadIdx.x, b = blockIdx.x;
  part += b * part_stride;
  rows += (int64_t)b * TSNE_SUMS * n;
  rowconst += (int64_t)b * 2 * n;
  float z = 0.f, klq = 0.f, c0 = 0.f, sp = 0.f;
  for (int i = t; i < n; i += TSNE_UPD) {
    float s[TSNE_SUMS];
#pragma unroll
    for (int k = 0; k < TSNE_SUMS; ++k) s[k] = 0.f;
    for (int sl = 0; sl < nslab; ++sl) {
#pragma unroll
      for (int k = 0; k < TSNE_SUMS; ++k) s[k] += part[((int64_t)sl * TSNE_SUMS + k) * n + i];
    }
#pragma unroll
    for (int k = 0; k < TSNE_SUMS; ++k) rows[(int64_t)k * n + i] = s[k];
    z += s[4];
    klq += s[5];
    if (history) {
      c0 += rowconst[i];
      sp += rowconst[n + i];
    }
  }
  const float Z = block_sum_1024(z, red);
  float g2 = 0.f;
  float* yb = Y + (int64_t)b * 2 * n;
  float* ub = update + (int64_t)b * 2 * n;
  float* gb = gains + (int64_t)b * 2 * n;
  for (int i = t; i < n; i += TSNE_UPD) {          // the rows this thread wrote in pass 1
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float g = 4.f * (alpha * rows[(int64_t)c * n + i] - rows[(int64_t)(2 + c) * n + i] / Z);
      const float u = ub[2 * i + c];
      float gain = gb[2 * i + c];
      gain = u * g < 0.f ? gain + 0.2f : gain * 0.8f;
      gain = fmaxf(gain, 0.01f);
      const float un = momentum * u - lr * (gain * g);
      gb[2 * i + c] = gain;
      ub[2 * i + c] = un;
      yb[2 * i + c] += un;
      g2 += g * g;
    }
  }
  g2 = block_sum_1024(g2, red);
  if (history) {
    klq = block_sum_1024(klq, red);
    c0 = block_sum_1024(c0, red);
    sp = block_sum_1024(sp, red);
  }
  if (t == 0) {
    float* s = scal + b * 8;
    s[0] = Z; s[1] = klq; s[2] = c0; s[3] = sp; s[4] = g2;
    if (history) {
      history[b * hist_stride] = (c0 + klq) + sp * logf(Z);
      history[b * hist_stride + 1] = sqrtf(g2);
    }
  }
}

// Workspace plan: one function for the query, the layout and the launches.
struct TsnePlan {
  int64_t nslab, part, part_stride, rows, rowconst, scal, total;
};

static const char* tsne_plan(int64_t n, int64_t batch, TsnePlan& p) {
  if (n < 4) return "n must be at least 4";
  if (n > TSNE_MAX_N) return "n above the cap of 12288 rows";
  if (batch < 1 || batch > 65535) return "batch out of range (1..65535)";
  p.nslab = (n + TSNE_SLAB - 1) / TSNE_SLAB;
  p.part_stride = p.nslab * TSNE_SUMS * n;         // floats per problem
  int64_t at = 0;
  auto take = [&](int64_t bytes) { const int64_t a = at; at += align256(bytes); return a; };
  p.part = take(batch * p.part_stride * 4);
  p.rows = take(batch * TSNE_SUMS * n * 4);
  p.rowconst = take(batch * 2 * n * 4);
  p.scal = take(batch * 8 * 4);
  p.total = at;
  return nullptr;
}

}  // namespace ieee

using namespace ieee;

extern "C" int64_t ieee_tsne_workspace_bytes(int64_t n, int64_t batch) {
  TsnePlan p;
  if (const char* why = tsne_plan(n, batch, p)) {
    set_error(IEEE_ERR_BAD_ARG, "tsne_workspace_bytes: %s (n=%ld batch=%ld)", why, (long)n, (long)batch);
    return -1;
  }
  return p.total;
}

extern "C" int ieee_tsne_layout(int64_t n, int64_t batch, int64_t* fields) {
  TsnePlan p;
  IEEE_REQUIRE(fields, "tsne_layout: null pointer");
  const char* why = tsne_plan(n, batch, p);
  IEEE_REQUIRE(!why, "tsne_layout: %s (n=%ld batch=%ld)", why, (long)n, (long)batch);
  const int64_t v[] = {p.nslab, p.part, p.rows, p.rowconst, p.scal, TSNE_SUMS};
  for (int k = 0; k < 6; ++k) fields[k] = v[k];
  return IEEE_OK;
}

extern "C" int ieee_tsne_affinities(const float* dist, int64_t ldd, int64_t n, int64_t batch, double perplexity, float* P,
                                    int64_t ldp, float* beta, void* work, int64_t work_bytes, void* stream) {
  IEEE_REQUIRE(dist && P && beta && work, "tsne_affinities: null pointer");
  TsnePlan p;
  const char* why = tsne_plan(n, batch, p);
  IEEE_REQUIRE(!why, "tsne_affinities: %s (n=%ld batch=%ld)", why, (long)n, (long)batch);
  IEEE_REQUIRE(perplexity > 0.0 && perplexity < (double)n, "tsne_affinities: perplexity must be positive and less than n "
               "(perplexity=%g n=%ld)", perplexity, (long)n);
  IEEE_REQUIRE(ldd >= n, "tsne_affinities: ldd=%ld is shorter than a row of n=%ld", (long)ldd, (long)n);
  IEEE_REQUIRE(ldp >= n && ldp % 4 == 0 && ((uintptr_t)P & 15) == 0, "tsne_affinities: P must be 16-byte aligned with ldp "
               ">= n a multiple of 4 (ldp=%ld n=%ld)", (long)ldp, (long)n);
  IEEE_REQUIRE(work_bytes >= p.total, "tsne_affinities: workspace too small (%ld < %ld bytes)", (long)work_bytes,
               (long)p.total);
  hipStream_t st = (hipStream_t)stream;
  tsne_search_kernel<<<dim3((unsigned)n, (unsigned)batch), 256, (size_t)n * sizeof(float), st>>>(
      dist, ldd, (int)n, (float)log(perplexity), P, ldp, beta);
  IEEE_TRY(launch_status("tsne_search_kernel"));
  const unsigned tiles = (unsigned)cdiv(n, 64);
  tsne_symmetrize_kernel<<<dim3(tiles, tiles, (unsigned)batch), 256, 0, st>>>(P, ldp, (int)n);
  return launch_status("tsne_symmetrize_kernel");
}

extern "C" int ieee_tsne_run(const float* P, int64_t ldp, int64_t n, int64_t batch, float* Y, float* update, float* gains,
                             int64_t iter0, int64_t n_iter, int64_t exaggeration_iters, double early_exaggeration,
                             double learning_rate, float* history, void* work, int64_t work_bytes, void* stream) {
  IEEE_REQUIRE(P && Y && update && gains && work, "tsne_run: null pointer");
  TsnePlan p;
  const char* why = tsne_plan(n, batch, p);
  IEEE_REQUIRE(!why, "tsne_run: %s (n=%ld batch=%ld)", why, (long)n, (long)batch);
  IEEE_REQUIRE(ldp >= n && ldp % 4 == 0 && ((uintptr_t)P & 15) == 0, "tsne_run: P must be 16-byte aligned with ldp >= n a "
               "multiple of 4 (ldp=%ld n=%ld)", (long)ldp, (long)n);
  IEEE_REQUIRE(((uintptr_t)Y & 7) == 0, "tsne_run: Y must be 8-byte aligned");
  IEEE_REQUIRE(iter0 >= 0 && n_iter >= 0, "tsne_run: iter0=%ld and n_iter=%ld must not be negative", (long)iter0,
               (long)n_iter);
  IEEE_REQUIRE(work_bytes >= p.total, "tsne_run: workspace too small (%ld < %ld bytes)", (long)work_bytes, (long)p.total);
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)work;
  float* part = (float*)(w + p.part);
  float* rows = (float*)(w + p.rows);
  float* rowconst = (float*)(w + p.rowconst);
  float* scal = (float*)(w + p.scal);
  const dim3 fgrid((unsigned)cdiv(n, 4), (unsigned)p.nslab, (unsigned)batch);
  if (history && n_iter > 0) {
    tsne_rowconst_kernel<<<dim3((unsigned)cdiv(n, 4), (unsigned)batch), 256, 0, st>>>(P, ldp, (int)n, rowconst, 2 * n);
    IEEE_TRY(launch_status("tsne_rowconst_kernel"));
  }
  for (int64_t k = 0; k < n_iter; ++k) {
    const bool early = iter0 + k < exaggeration_iters;
    if (history)
      tsne_force_kernel<true><<<fgrid, 256, 0, st>>>(P, ldp, (int)n, Y, part, p.part_stride);
    else
      tsne_force_kernel<false><<<fgrid, 256, 0, st>>>(P, ldp, (int)n, Y, part, p.part_stride);
    IEEE_TRY(launch_status("tsne_force_kernel"));
    tsne_update_kernel<<<(unsigned)batch, TSNE_UPD, 0, st>>>(part, (int)p.nslab, (int)n, p.part_stride, rows, rowconst, scal,
                                                            Y, update, gains, early ? (float)early_exaggeration : 1.f,
                                                            early ? 0.5f : 0.8f, (float)learning_rate,
                                                            history ? history + 2 * k : nullptr, 2 * n_iter);
    IEEE_TRY(launch_status("tsne_update_kernel"));
  }
  return IEEE_OK;
}
