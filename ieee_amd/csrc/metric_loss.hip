// Metric-learning criteria of torchreid/losses that are not on the margin config's path: the batch-hard triplet loss
// (hard_mine_triplet_loss.py:23-48), the hetero-center loss (hcloss.py:18-39) and the 'l1' distance of the 3M loss
// (multi_modal_margin_loss_new.py:19-40).  Forward AND backward, fp32, wave64, no floating-point atomics: every sum has one
// fixed order, so two calls give the same bits.  The problems are tiny (B <= a few thousand rows); what counts here is
// that the gradient is the reference's in every corner (clamped pairs, ties, the hinge), and the launch count.
//
// Triplet distances: d_ij = sqrt(max(d2_ij, 1e-12)) with d2 formed FROM DIFFERENCES, sum_k (x_ik - x_jk)^2, which is exactly 0
// on the diagonal and for duplicate rows, and bitwise symmetric (d2_ij == d2_ji).  The reference forms d2 from the Gram
// expansion |x_i|^2 + |x_j|^2 - 2 x_i.x_j; in fp32 that leaves +-6.6e-7 on the diagonal at D = 2304 (unit-norm parts), i.e.
// a "distance" of 8e-4 of a row to itself WITH a gradient.  The difference form is the quantity that expansion approximates.
#include "common.h"

namespace ieee {

static constexpr int kMaxRows = 4096;      // LDS: one row of distances / weights (16 KiB) + one index list (16 KiB)
static constexpr float kClamp = 1e-12f;    // dist.clamp(min=1e-12) (hard_mine_triplet_loss.py:35)

__device__ __forceinline__ int64_t desc_off(int p, int row, int k, int B, int D) {
  return ((int64_t)p * B + row) * (int64_t)D + k;
}

// Launch 1, one workgroup per anchor i.  The waves share the rows j; for each, lane l sums elements l, l + 64, ... of
// every part in order (one FMA chain of ceil(D/64) * parts terms), then a butterfly: the same bits in all 64 lanes.
// d2 goes to d2mat[i][j] for the gather pass.  Mining over the row: hardest positive = max over the same identity (the
// row itself included, as in the reference), hardest negative = min over the others, and HOW MANY entries are exactly
// equal to each (Tensor.max() / .min() without `dim` split the gradient evenly among equal entries).
// anc[0..4][B] = d_ap, d_an, coefficient per tied positive, per tied negative, hinge term.
__global__ __launch_bounds__(256) void triplet_mine_kernel(const float* __restrict__ x, const int64_t* __restrict__ pids,
                                                          float* __restrict__ d2mat, float* __restrict__ anc, int parts,
                                                          int B, int D, float margin) {
  __shared__ float s_d[kMaxRows];
  __shared__ float s_max[256], s_min[256];
  __shared__ int s_np[256], s_nn[256];
  const int i = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  // four rows j per pass of a wave: one load of x_i feeds four independent chains (the step is latency bound: B = 64 is 64
  // workgroups of 4 waves); each row's sum keeps its own order (lane chain, then butterfly), so d2_ij == d2_ji bitwise
  for (int jb = wave * 4; jb < B; jb += 16) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int jr[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) jr[q] = min(jb + q, B - 1);          // (a ragged last group re-reads row B-1; not stored)
    for (int p = 0; p < parts; ++p) {
      const float* xi = x + desc_off(p, i, 0, B, D);
      const float* xj[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) xj[q] = x + desc_off(p, jr[q], 0, B, D);
      for (int k = lane; k < D; k += 64) {
        const float a = xi[k];
#pragma unroll
        for (int q = 0; q < 4; ++q) { const float d = a - xj[q][k]; s[q] += d * d; }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float v = wave_sum(s[q]);
      const int j = jb + q;
      if (lane == 0 && j < B) { s_d[j] = sqrtf(fmaxf(v, kClamp)); d2mat[(int64_t)i * B + j] = v; }
    }
  }
  __syncthreads();
  const int64_t pi = pids[i];
  float mx = -INFINITY, mn = INFINITY;
  for (int j = t; j < B; j += 256) {
    const float d = s_d[j];
    if (pids[j] == pi) mx = fmaxf(mx, d); else mn = fminf(mn, d);
  }
  s_max[t] = mx; s_min[t] = mn;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) { s_max[t] = fmaxf(s_max[t], s_max[t + o]); s_min[t] = fminf(s_min[t], s_min[t + o]); }
    __syncthreads();
  }
  const float ap = s_max[0], an = s_min[0];
  int np = 0, nn = 0;
  for (int j = t; j < B; j += 256) {
    const float d = s_d[j];
    if (pids[j] == pi) np += d == ap ? 1 : 0; else nn += d == an ? 1 : 0;
  }
  s_np[t] = np; s_nn[t] = nn;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) { s_np[t] += s_np[t + o]; s_nn[t] += s_nn[t + o]; }
    __syncthreads();
  }
  if (t == 0) {
    const float h = margin + ap - an;                      // MarginRankingLoss(dist_an, dist_ap, y = 1) (:47-48)
    const bool active = h > 0.f && s_nn[0] > 0;
    anc[i] = ap;
    anc[B + i] = an;
    anc[2 * B + i] = active ? 1.0f / ((float)B * (float)s_np[0]) : 0.f;     // d mean-hinge / d d_ij of a tied positive
    anc[3 * B + i] = active ? 1.0f / ((float)B * (float)s_nn[0]) : 0.f;     // (minus that) of a tied negative
    anc[4 * B + i] = h > 0.f ? h : 0.f;
  }
}

// Launch 2, gather form, one workgroup per row i: dx_i = gscale * sum_j w_ij (x_i - x_j), j ascending, where w_ij collects
// what the pair (i, j) receives -- i as anchor with j among its hardest, and j as anchor with i among ITS hardest (d is
// bitwise symmetric, so row i of d2mat serves both) -- divided by d_ij.  A clamped pair (d2 < 1e-12) has w = 0: the clamp's
// gradient is zero there.  Wave 0 compacts the non-zero weights in ascending j (ballot + prefix count), so the element
// loop runs over the few pairs that matter.  Workgroup 0 also reduces the per-anchor terms to out[0..4) with a fixed tree.
__global__ __launch_bounds__(256) void triplet_gather_kernel(const float* __restrict__ x, const int64_t* __restrict__ pids,
                                                            const float* __restrict__ d2mat, const float* __restrict__ anc,
                                                            float* dx, float* __restrict__ out, int parts, int B, int D,
                                                            float gscale, int accumulate) {
  __shared__ float s_w[kMaxRows];
  __shared__ int s_idx[kMaxRows];
  __shared__ float s_red[4][256];
  __shared__ int s_n;
  const int i = blockIdx.x, t = threadIdx.x;
  if (i == 0) {
    float a = 0.f, b = 0.f, c = 0.f, n = 0.f;
    for (int j = t; j < B; j += 256) {
      a += anc[4 * B + j]; b += anc[j]; c += anc[B + j]; n += anc[4 * B + j] > 0.f ? 1.f : 0.f;
    }
    s_red[0][t] = a; s_red[1][t] = b; s_red[2][t] = c; s_red[3][t] = n;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (t < o) for (int q = 0; q < 4; ++q) s_red[q][t] += s_red[q][t + o];
      __syncthreads();
    }
    if (t == 0) { out[0] = s_red[0][0] / B; out[1] = s_red[1][0] / B; out[2] = s_red[2][0] / B; out[3] = s_red[3][0]; }
  }
  if (!dx) return;
  const int64_t pi = pids[i];
  const float ap_i = anc[i], an_i = anc[B + i], cp_i = anc[2 * B + i], cn_i = anc[3 * B + i];
  for (int j = t; j < B; j += 256) {
    const float d2 = d2mat[(int64_t)i * B + j];
    float w = 0.f;
    if (d2 >= kClamp) {
      const float d = sqrtf(d2);
      if (pids[j] == pi) {
        if (d == ap_i) w += cp_i;
        if (d == anc[j]) w += anc[2 * B + j];
      } else {
        if (d == an_i) w -= cn_i;
        if (d == anc[B + j]) w -= anc[3 * B + j];
      }
      w /= d;
    }
    s_w[j] = w;
  }
  __syncthreads();
  if (t < 64) {
    int count = 0;
    for (int base = 0; base < B; base += 64) {
      const int j = base + t;
      const float w = j < B ? s_w[j] : 0.f;
      const unsigned long long mask = __ballot(w != 0.f);
      const int pos = count + __popcll(mask & ((1ull << t) - 1ull));
      if (w != 0.f) { s_w[pos] = w; s_idx[pos] = j; }      // pos <= j, and this chunk is already in registers
      count += __popcll(mask);
    }
    if (t == 0) s_n = count;
  }
  __syncthreads();
  const int n = s_n;
  for (int p = 0; p < parts; ++p)
    for (int k = t; k < D; k += 256) {
      const int64_t o = desc_off(p, i, k, B, D);
      const float xi = x[o];
      float acc = 0.f;
      for (int c = 0; c < n; ++c) acc += s_w[c] * (xi - x[desc_off(p, s_idx[c], k, B, D)]);
      const float g = gscale * acc;
      dx[o] = accumulate ? dx[o] + g : g;
    }
}

// ---- centre losses --------------------------------------------------------------------------------------------------
// One workgroup per identity chunk, torch.chunk semantics exactly as margin3m_kernel (head.hip) has them: ceil(B/label_num)
// rows per chunk, every workgroup recounts label_num itself, rows beyond the chunks the reference loops over get no loss
// term and a zero gradient.  M modalities [M][B][D].  The <3, L2, MARGIN3M> instance restates margin3m_kernel statement by
// statement and gives its bits.
//   HETERO (M = 2):   l2 |sum_k (c1-c2)^2|,  l1 |mean_k |c1-c2||,  cos max(0, 1 - cos(c1, c2)) with nn.CosineSimilarity's
//                     eps = 1e-8 on each norm; python's max(0, v) keeps the int 0 (no gradient) unless v > 0.
//   MARGIN3M (M = 3): max(|m-d12|, |m-d23|, |m-d13|), the FIRST maximal argument in that order; sign(0) = 0.
enum { DIST_L2 = 0, DIST_L1 = 1, DIST_COS = 2 };
enum { MODE_HETERO = 0, MODE_MARGIN3M = 1 };

template <int M, int DIST, int MODE>
__global__ __launch_bounds__(256) void center_pairs_kernel(const float* feats, const int64_t* pids, float* dfeats,
                                                           float* terms, int B, int D, float margin, float gscale,
                                                           int accumulate) {
  __shared__ float red[3][256];
  __shared__ int s_cnt[256];
  __shared__ int s_sel;
  __shared__ float s_sign;
  __shared__ float s_cos[4];
  const int t = threadIdx.x;
  int cnt = 0;
  for (int i = t; i < B; i += 256) {
    bool seen = false;
    for (int j = 0; j < i; ++j) if (pids[j] == pids[i]) { seen = true; break; }
    cnt += seen ? 0 : 1;
  }
  s_cnt[t] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (t < o) s_cnt[t] += s_cnt[t + o]; __syncthreads(); }
  const int n = s_cnt[0];
  const int csize = (B + n - 1) / n;            // torch.chunk: ceil(B / chunks) rows per chunk
  const int nchunks = (B + csize - 1) / csize;
  const int nuse = nchunks < n ? nchunks : n;
  const int ch = blockIdx.x;
  const int64_t BD = (int64_t)B * D;
  if (ch == 0 && t == 0) { terms[B] = (float)n; terms[B + 1] = (float)nchunks; terms[B + 2] = (float)nuse; }
  const int r0 = ch * csize, r1 = min(B, r0 + csize), rows = r1 - r0;
  if (rows <= 0) { if (t == 0) terms[ch] = 0.f; return; }
  if (ch >= nuse) {   // rows beyond the chunks the reference loops over: no loss term, zero gradient
    if (t == 0) terms[ch] = 0.f;
    if (dfeats && !accumulate)
      for (int m = 0; m < M; ++m)
        for (int64_t i = t; i < (int64_t)rows * D; i += 256) dfeats[m * BD + (int64_t)r0 * D + i] = 0.f;
    return;
  }
  // per-thread partial sums: l2 / l1 -> the pair distances (1,2), (2,3), (1,3); cos -> c1.c2, |c1|^2, |c2|^2
  float d12 = 0.f, d23 = 0.f, d13 = 0.f;
  for (int k = t; k < D; k += 256) {
    float c1 = 0.f, c2 = 0.f, c3 = 0.f;
    if constexpr (M == 3) {
      for (int r = r0; r < r1; ++r) { c1 += feats[r * D + k]; c2 += feats[BD + r * D + k]; c3 += feats[2 * BD + r * D + k]; }
      c1 /= rows; c2 /= rows; c3 /= rows;
    } else {
      for (int r = r0; r < r1; ++r) { c1 += feats[(int64_t)r * D + k]; c2 += feats[BD + (int64_t)r * D + k]; }
      c1 /= rows; c2 /= rows;
    }
    if constexpr (DIST == DIST_L2) {
      d12 += (c1 - c2) * (c1 - c2);
      if constexpr (M == 3) {
        d23 += (c2 - c3) * (c2 - c3);
        d13 += (c1 - c3) * (c1 - c3);
      }
    } else if constexpr (DIST == DIST_L1) {
      d12 += fabsf(c1 - c2);
      if constexpr (M == 3) { d23 += fabsf(c2 - c3); d13 += fabsf(c1 - c3); }
    } else {
      d12 += c1 * c2; d23 += c1 * c1; d13 += c2 * c2;
    }
  }
  red[0][t] = d12; red[1][t] = d23; red[2][t] = d13;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; red[2][t] += red[2][t + o]; }
    __syncthreads();
  }
  if (t == 0) {
    if constexpr (DIST == DIST_L1) { red[0][0] /= D; red[1][0] /= D; red[2][0] /= D; }      // nn.L1Loss: the MEAN
    if constexpr (MODE == MODE_MARGIN3M) {
      // python max(a, b, c) keeps the FIRST maximal argument: order (1,2), (2,3), (1,3)  (:35)
      const float a1 = fabsf(margin - red[0][0]), a2 = fabsf(margin - red[1][0]), a3 = fabsf(margin - red[2][0]);
      int sel = 0; float best = a1;
      if (a2 > best) { best = a2; sel = 1; }
      if (a3 > best) { best = a3; sel = 2; }
      const float dsel = sel == 0 ? red[0][0] : (sel == 1 ? red[1][0] : red[2][0]);
      const float x = margin - dsel;
      s_sel = sel;
      s_sign = x > 0.f ? -1.f : (x < 0.f ? 1.f : 0.f);   // d|m-d|/dd
      terms[ch] = best;
    } else if constexpr (DIST == DIST_COS) {
      const float eps = 1e-8f;
      const float na = sqrtf(red[1][0]), nb = sqrtf(red[2][0]);
      const float ca = fmaxf(na, eps), cb = fmaxf(nb, eps);
      const float cs = red[0][0] / (ca * cb);
      const float v = 1.f - cs;
      s_sel = 0;
      s_sign = v > 0.f ? 1.f : 0.f;                      // max(0, 1 - cos): the int 0 unless 1 - cos > 0
      s_cos[0] = 1.f / (ca * cb);
      s_cos[1] = na >= eps ? cs / (ca * na) : 0.f;       // the clamped norm has no gradient
      s_cos[2] = nb >= eps ? cs / (cb * nb) : 0.f;
      terms[ch] = v > 0.f ? v : 0.f;
    } else {
      const float s = red[0][0];
      s_sel = 0;
      s_sign = s > 0.f ? 1.f : (s < 0.f ? -1.f : 0.f);   // d|s|/ds; max(0, |s|) is |s|
      terms[ch] = fabsf(s);
    }
  }
  __syncthreads();
  if (dfeats) {
    const int sel = s_sel;
    const int ia = sel == 1 ? 1 : 0;          // pair (a,b): (0,1), (1,2), (0,2)
    const int ib = sel == 0 ? 1 : 2;
    const int ic = 3 - ia - ib;               // the modality not in the selected pair gets zero
    if constexpr (DIST == DIST_L2) {
      const float coef = s_sign * 2.0f / rows * gscale;
      for (int k = t; k < D; k += 256) {
        float ca = 0.f, cb = 0.f;
        for (int r = r0; r < r1; ++r) { ca += feats[ia * BD + r * D + k]; cb += feats[ib * BD + r * D + k]; }
        const float diff = (ca - cb) / rows;
        for (int r = r0; r < r1; ++r) {
          if (accumulate) {
            dfeats[ia * BD + r * D + k] += coef * diff;
            dfeats[ib * BD + r * D + k] += -coef * diff;
          } else {
            dfeats[ia * BD + r * D + k] = coef * diff;
            dfeats[ib * BD + r * D + k] = -coef * diff;
            if constexpr (M == 3) dfeats[ic * BD + r * D + k] = 0.f;
          }
        }
      }
    } else if constexpr (DIST == DIST_L1) {
      const float coef = s_sign / D / rows * gscale;
      for (int k = t; k < D; k += 256) {
        float ca = 0.f, cb = 0.f;
        for (int r = r0; r < r1; ++r) { ca += feats[ia * BD + (int64_t)r * D + k]; cb += feats[ib * BD + (int64_t)r * D + k]; }
        ca /= rows; cb /= rows;                                  // the centres exactly as the forward pass formed them
        const float diff = ca - cb;
        const float g = coef * (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f));     // sign(0) = 0, as in torch
        for (int r = r0; r < r1; ++r) {
          if (accumulate) {
            dfeats[ia * BD + (int64_t)r * D + k] += g;
            dfeats[ib * BD + (int64_t)r * D + k] += -g;
          } else {
            dfeats[ia * BD + (int64_t)r * D + k] = g;
            dfeats[ib * BD + (int64_t)r * D + k] = -g;
            if constexpr (M == 3) dfeats[ic * BD + (int64_t)r * D + k] = 0.f;
          }
        }
      }
    } else {
      // d(1 - cos)/dc1_k = -(c2_k / (n1 n2) - cos c1_k / n1^2), and the same with 1 <-> 2
      const float sc = s_sign / rows * gscale, inv = s_cos[0], qa = s_cos[1], qb = s_cos[2];
      for (int k = t; k < D; k += 256) {
        float ca = 0.f, cb = 0.f;
        for (int r = r0; r < r1; ++r) { ca += feats[(int64_t)r * D + k]; cb += feats[BD + (int64_t)r * D + k]; }
        ca /= rows; cb /= rows;
        const float ga = -sc * (cb * inv - qa * ca), gb = -sc * (ca * inv - qb * cb);
        for (int r = r0; r < r1; ++r) {
          if (accumulate) { dfeats[(int64_t)r * D + k] += ga; dfeats[BD + (int64_t)r * D + k] += gb; }
          else { dfeats[(int64_t)r * D + k] = ga; dfeats[BD + (int64_t)r * D + k] = gb; }
        }
      }
    }
  }
}

// the chunk terms summed in chunk order by one thread, like margin3m_sum_kernel
__global__ void center_sum_kernel(const float* terms, float* out, int B) {
  if (threadIdx.x != 0) return;
  const int nuse = (int)terms[B + 2];
  float loss = 0.f;
  for (int c = 0; c < nuse; ++c) loss += terms[c];
  out[0] = loss; out[1] = terms[B]; out[2] = terms[B + 1];
}

}  // namespace ieee

using namespace ieee;

extern "C" int ieee_triplet_hard_fwd_bwd(const float* x, int64_t parts, const int64_t* pids, float* dx, float* out,
                                         float* work, int64_t B, int64_t D, float margin, float grad_scale,
                                         int accumulate, void* stream) {
  IEEE_REQUIRE(x && pids && out && work, "triplet_hard_fwd_bwd: null pointer");
  IEEE_REQUIRE(parts >= 1 && parts <= 64, "triplet_hard_fwd_bwd: parts must be in [1, 64]");
  IEEE_REQUIRE(B >= 1 && B <= kMaxRows, "triplet_hard_fwd_bwd: batch must be in [1, %d]", kMaxRows);
  IEEE_REQUIRE(D >= 1 && D <= (int64_t)1 << 24, "triplet_hard_fwd_bwd: feature width out of range");
  hipStream_t st = (hipStream_t)stream;
  float* d2mat = work;                  // [B][B]
  float* anc = work + B * B;            // [5][B]
  triplet_mine_kernel<<<(unsigned)B, 256, 0, st>>>(x, pids, d2mat, anc, (int)parts, (int)B, (int)D, margin);
  IEEE_TRY(launch_status("triplet_mine_kernel"));
  triplet_gather_kernel<<<dx ? (unsigned)B : 1u, 256, 0, st>>>(x, pids, d2mat, anc, dx, out, (int)parts, (int)B, (int)D,
                                                               grad_scale, accumulate);
  return launch_status("triplet_gather_kernel");
}

extern "C" int ieee_center_pairs_fwd_bwd(const float* feats, int64_t M, const int64_t* pids, float* dfeats, float* out3,
                                         float* work, int64_t B, int64_t D, int dist_type, int mode, float margin,
                                         float grad_scale, int accumulate, void* stream) {
  IEEE_REQUIRE(feats && pids && out3 && work, "center_pairs_fwd_bwd: null pointer");
  IEEE_REQUIRE(B >= 1 && D >= 1 && B <= 65535 && D <= (int64_t)1 << 24, "center_pairs_fwd_bwd: batch out of range");
  IEEE_REQUIRE(B * D * M < (int64_t)1 << 31, "center_pairs_fwd_bwd: more than 2^31 elements");
  hipStream_t st = (hipStream_t)stream;
  const unsigned g = (unsigned)B;
  const int b = (int)B, d = (int)D;
  if (mode == IEEE_CENTER_HETERO) {
    IEEE_REQUIRE(M == 2, "center_pairs_fwd_bwd: the hetero-center loss takes 2 modalities");
    if (dist_type == IEEE_DIST_L2)
      center_pairs_kernel<2, DIST_L2, MODE_HETERO><<<g, 256, 0, st>>>(feats, pids, dfeats, work, b, d, margin, grad_scale, accumulate);
    else if (dist_type == IEEE_DIST_L1)
      center_pairs_kernel<2, DIST_L1, MODE_HETERO><<<g, 256, 0, st>>>(feats, pids, dfeats, work, b, d, margin, grad_scale, accumulate);
    else if (dist_type == IEEE_DIST_COS)
      center_pairs_kernel<2, DIST_COS, MODE_HETERO><<<g, 256, 0, st>>>(feats, pids, dfeats, work, b, d, margin, grad_scale, accumulate);
    else
      IEEE_REQUIRE(false, "center_pairs_fwd_bwd: unknown dist_type %d", dist_type);
  } else if (mode == IEEE_CENTER_MARGIN3M) {
    IEEE_REQUIRE(M == 3, "center_pairs_fwd_bwd: the 3M loss takes 3 modalities");
    if (dist_type == IEEE_DIST_L2)
      center_pairs_kernel<3, DIST_L2, MODE_MARGIN3M><<<g, 256, 0, st>>>(feats, pids, dfeats, work, b, d, margin, grad_scale, accumulate);
    else if (dist_type == IEEE_DIST_L1)
      center_pairs_kernel<3, DIST_L1, MODE_MARGIN3M><<<g, 256, 0, st>>>(feats, pids, dfeats, work, b, d, margin, grad_scale, accumulate);
    else
      IEEE_REQUIRE(false, "center_pairs_fwd_bwd: the 3M loss has no dist_type %d (the reference's 'cos' branch never "
                   "assigns its distance)", dist_type);
  } else {
    IEEE_REQUIRE(false, "center_pairs_fwd_bwd: unknown mode %d", mode);
  }
  IEEE_TRY(launch_status("center_pairs_kernel"));
  center_sum_kernel<<<1, 64, 0, st>>>(work, out3, b);
  return launch_status("center_sum_kernel");
}
