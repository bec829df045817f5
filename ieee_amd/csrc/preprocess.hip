// Input pipeline on the device: the reference's per-image transform chain
//   Resize((H,W)) [PIL bilinear, antialiased] -> RandomHorizontalFlip -> ToTensor -> Normalize
// (torchreid/data/transforms.py:233-326, applied to every modality image separately in
// data/datasets/dataset.py:335-351) for a whole batch of decoded uint8 HWC images in two launches.
// The resize is Pillow's two-pass 8-bit resampler reproduced bit for bit: 22-bit fixed-point weights (computed on
// the host exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc do, ieee_amd/data/transforms.py), int32
// accumulation with the rounding bias, 8-bit clip after EACH pass (the horizontal pass writes a uint8 intermediate).
// Byte/integer work bound by HBM: nothing here belongs on the matrix cores.
#include "common.h"

#include <algorithm>
#include <cmath>

namespace ieee {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ uint8_t clip8(int acc) {
  const int v = acc >> PRECISION_BITS;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// horizontal pass: tmp[n][r][xx][c] = clip8(bias + sum_x src[n][y0 + r][xmin + x][c] * k[xx][x])
__global__ __launch_bounds__(256) void resize_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ tmp,
                                                       const int* __restrict__ bounds, const int* __restrict__ kk,
                                                       int ksize, int Hs, int Ws, int Wo, int y0, int rows,
                                                       int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (n, r, xx)
  if (i >= total) return;
  const int xx = (int)(i % Wo);
  const int64_t t = i / Wo;
  const int r = (int)(t % rows);
  const int64_t n = t / rows;
  const int xmin = bounds[2 * xx], cnt = bounds[2 * xx + 1];
  const uint8_t* p = src + ((n * Hs + y0 + r) * (int64_t)Ws + xmin) * 3;
  const int* k = kk + (int64_t)xx * ksize;
  int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
  for (int x = 0; x < cnt; ++x) {
    const int w = k[x];
    a0 += p[3 * x] * w;
    a1 += p[3 * x + 1] * w;
    a2 += p[3 * x + 2] * w;
  }
  uint8_t* o = tmp + i * 3;
  o[0] = clip8(a0); o[1] = clip8(a1); o[2] = clip8(a2);
}

// vertical pass (or none) fused with flip + ToTensor + Normalize:
// dst[n][c][yy][xo] = (u8 / 255 - mean[c]) / std[c],  xo = flip[n] ? Wo-1-xx : xx
__global__ __launch_bounds__(256) void resize_v_norm_kernel(const uint8_t* __restrict__ in, float* __restrict__ dst,
                                                            const int* __restrict__ bounds, const int* __restrict__ kk,
                                                            int ksize, int Hin, int Ho, int Wo, int yshift,
                                                            const uint8_t* __restrict__ flip, float m0, float m1,
                                                            float m2, float s0, float s1, float s2, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (n, yy, xx)
  if (i >= total) return;
  const int xx = (int)(i % Wo);
  const int64_t t = i / Wo;
  const int yy = (int)(t % Ho);
  const int64_t n = t / Ho;
  uint8_t u0, u1, u2;
  if (kk != nullptr) {
    const int ymin = bounds[2 * yy] - yshift, cnt = bounds[2 * yy + 1];
    const uint8_t* p = in + ((n * Hin + ymin) * (int64_t)Wo + xx) * 3;
    const int* k = kk + (int64_t)yy * ksize;
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int y = 0; y < cnt; ++y) {
      const int w = k[y];
      const uint8_t* q = p + (int64_t)y * Wo * 3;
      a0 += q[0] * w;
      a1 += q[1] * w;
      a2 += q[2] * w;
    }
    u0 = clip8(a0); u1 = clip8(a1); u2 = clip8(a2);
  } else {
    const uint8_t* p = in + ((n * Hin + yy) * (int64_t)Wo + xx) * 3;
    u0 = p[0]; u1 = p[1]; u2 = p[2];
  }
  const int xo = (flip != nullptr && flip[n]) ? Wo - 1 - xx : xx;
  const int64_t plane = (int64_t)Ho * Wo;
  float* o = dst + n * 3 * plane + (int64_t)yy * Wo + xo;
  o[0] = ((float)u0 / 255.0f - m0) / s0;          // ToTensor: u8 -> f32, div(255); Normalize: sub(mean).div(std)
  o[plane] = ((float)u1 / 255.0f - m1) / s1;
  o[2 * plane] = ((float)u2 / 255.0f - m2) / s2;
}

// ---- train augmentations (reference transforms.py: Random2DTranslation, torchvision ColorJitter through Pillow's
// ImageEnhance, RandomErasing), applied per image from a plan the host drew (ieee_amd/data/transforms.py, AugmentPlan):
//   stage  : vertical resize pass (or none) -> uint8 [N][Ho][Wo][3], FLIPPED (the enlargement below is not guaranteed to
//            commute with the flip bit for bit)
//   crop_h : images with the crop flag: horizontal pass of the Wo -> Wbig enlargement over columns x1 .. x1+Wo only and
//            over the stage rows the window's vertical pass reads, uint8 intermediate
//   crop_v : vertical pass Ho -> Hbig for rows y1 .. y1+Ho -> the cropped uint8 image; and, for the jitter, the image's
//            integer sum of L (exact in any order: vector integer atomics, one per block)
//   final  : brightness / contrast blends in the image's order, ToTensor, Normalize, erase rectangle
// A grid is (pixels of one image / 256, N): the plan words of a block are wave-uniform.
constexpr int PLAN_WORDS = 12;
enum { P_FLIP = 0, P_CROP = 1, P_X1 = 2, P_Y1 = 3, P_FIRST = 4, P_B = 5, P_C = 6, P_R0 = 7, P_C0 = 8, P_EH = 9, P_EW = 10, P_LSUM = 11 };
enum { ST_FLIP = 1, ST_CROP = 2, ST_JITTER = 4, ST_ERASE = 8 };

// Pillow's ImagingBlend on one byte: t = deg + f * (img - deg) in C float -- a rounded product, then a rounded sum: the
// contraction into one fused multiply-add that device code gets by default is switched off for this function;
// 0 <= f <= 1: (UINT8) t, else clipped to 0 .. 255 before the cast
__device__ __forceinline__ int blend8(int deg, int img, float f) {
#pragma clang fp contract(off)
  const float p = f * (float)(img - deg);
  const float t = (float)deg + p;
  if (f >= 0.0f && f <= 1.0f) return (int)t;
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// Pillow's RGB -> L
__device__ __forceinline__ unsigned luma(int r, int g, int b) { return (unsigned)(19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// the L of a pixel as the contrast stage meets it: after the brightness blend when brightness comes first
__device__ __forceinline__ unsigned luma_at_contrast(const int32_t* pl, int u0, int u1, int u2) {
  if (pl[P_FIRST] == 0) {
    const float b = __int_as_float(pl[P_B]);
    u0 = blend8(0, u0, b); u1 = blend8(0, u1, b); u2 = blend8(0, u2, b);
  }
  return luma(u0, u1, u2);
}

// the block's sum of v into *dst: waves by shuffle, the four waves through LDS, one atomic per block (every thread calls)
__device__ __forceinline__ void block_sum_add(unsigned v, unsigned* dst) {
  __shared__ unsigned part[4];
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(dst, part[0] + part[1] + part[2] + part[3]);
}

// one output pixel of the vertical pass (or, kk == nullptr, the pixel itself)
__device__ __forceinline__ void vertical_px(const uint8_t* __restrict__ in, const int* __restrict__ bounds,
                                            const int* __restrict__ kk, int ksize, int Hin, int Wo, int yshift, int64_t n,
                                            int yy, int xx, int& u0, int& u1, int& u2) {
  if (kk != nullptr) {
    const int ymin = bounds[2 * yy] - yshift, cnt = bounds[2 * yy + 1];
    const uint8_t* p = in + ((n * Hin + ymin) * (int64_t)Wo + xx) * 3;
    const int* k = kk + (int64_t)yy * ksize;
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int y = 0; y < cnt; ++y) {
      const int w = k[y];
      const uint8_t* q = p + (int64_t)y * Wo * 3;
      a0 += q[0] * w;
      a1 += q[1] * w;
      a2 += q[2] * w;
    }
    u0 = clip8(a0); u1 = clip8(a1); u2 = clip8(a2);
  } else {
    const uint8_t* p = in + ((n * Hin + yy) * (int64_t)Wo + xx) * 3;
    u0 = p[0]; u1 = p[1]; u2 = p[2];
  }
}

__global__ __launch_bounds__(256) void augment_stage_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ stage,
                                                            const int* __restrict__ bounds, const int* __restrict__ kk,
                                                            int ksize, int Hin, int Ho, int Wo, int yshift,
                                                            int32_t* plan, int stages, int sum_here) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const int64_t n = blockIdx.y;
  const bool live = pix < Ho * Wo;
  int32_t* pl = plan + n * PLAN_WORDS;
  unsigned l = 0;
  if (live) {
    const int yy = pix / Wo, xx = pix - yy * Wo;
    int u0, u1, u2;
    vertical_px(in, bounds, kk, ksize, Hin, Wo, yshift, n, yy, xx, u0, u1, u2);
    const int xo = ((stages & ST_FLIP) && pl[P_FLIP]) ? Wo - 1 - xx : xx;
    uint8_t* o = stage + ((n * Ho + yy) * (int64_t)Wo + xo) * 3;
    o[0] = (uint8_t)u0; o[1] = (uint8_t)u1; o[2] = (uint8_t)u2;
    if (sum_here) l = luma_at_contrast(pl, u0, u1, u2);
  }
  if (sum_here) block_sum_add(l, (unsigned*)(pl + P_LSUM));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ctmp[n][r][xx][c] = clip8(bias + sum_x stage[n][r][xmin + x][c] * k[x1 + xx][x]) for the stage rows r the window reads
__global__ __launch_bounds__(256) void augment_crop_h_kernel(const uint8_t* __restrict__ stage, uint8_t* __restrict__ ctmp,
                                                             const int* __restrict__ bounds_h, const int* __restrict__ kk_h,
                                                             int ksize_h, const int* __restrict__ bounds_v, int Ho, int Wo,
                                                             int Hbig, int Wbig, const int32_t* __restrict__ plan) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const int64_t n = blockIdx.y;
  const int32_t* pl = plan + n * PLAN_WORDS;
  if (pix >= Ho * Wo || !pl[P_CROP]) return;
  const int x1 = clampi(pl[P_X1], 0, Wbig - Wo), y1 = clampi(pl[P_Y1], 0, Hbig - Ho);
  const int r = pix / Wo, xx = pix - r * Wo;
  const int last = y1 + Ho - 1;
  if (r < bounds_v[2 * y1] || r >= bounds_v[2 * last] + bounds_v[2 * last + 1]) return;
  const int xb = x1 + xx;
  const int xmin = bounds_h[2 * xb], cnt = bounds_h[2 * xb + 1];
  const uint8_t* p = stage + ((n * Ho + r) * (int64_t)Wo + xmin) * 3;
  const int* k = kk_h + (int64_t)xb * ksize_h;
  int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
  for (int x = 0; x < cnt; ++x) {
    const int w = k[x];
    a0 += p[3 * x] * w;
    a1 += p[3 * x + 1] * w;
    a2 += p[3 * x + 2] * w;
  }
  uint8_t* o = ctmp + ((n * Ho + r) * (int64_t)Wo + xx) * 3;
  o[0] = clip8(a0); o[1] = clip8(a1); o[2] = clip8(a2);
}

// cimg[n][yy][xx][c] = row y1 + yy of the enlargement's vertical pass over ctmp (images with the flag); with the jitter on,
// every image's sum of L (of cimg where cropped, of the stage image where not)
__global__ __launch_bounds__(256) void augment_crop_v_kernel(const uint8_t* __restrict__ stage, const uint8_t* __restrict__ ctmp,
                                                             uint8_t* __restrict__ cimg, const int* __restrict__ bounds_v,
                                                             const int* __restrict__ kk_v, int ksize_v, int Ho, int Wo,
                                                             int Hbig, int32_t* plan, int stages) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const int64_t n = blockIdx.y;
  int32_t* pl = plan + n * PLAN_WORDS;
  const bool live = pix < Ho * Wo, crop = pl[P_CROP] != 0, jitter = (stages & ST_JITTER) != 0;
  unsigned l = 0;
  if (live && (crop || jitter)) {
    const int yy = pix / Wo, xx = pix - yy * Wo;
    int u0, u1, u2;
    if (crop) {
      const int y1 = clampi(pl[P_Y1], 0, Hbig - Ho);
      vertical_px(ctmp, bounds_v, kk_v, ksize_v, Ho, Wo, 0, n, y1 + yy, xx, u0, u1, u2);
      uint8_t* o = cimg + ((n * Ho + yy) * (int64_t)Wo + xx) * 3;
      o[0] = (uint8_t)u0; o[1] = (uint8_t)u1; o[2] = (uint8_t)u2;
    } else {
      vertical_px(stage, nullptr, nullptr, 0, Ho, Wo, 0, n, yy, xx, u0, u1, u2);
    }
    if (jitter) l = luma_at_contrast(pl, u0, u1, u2);
  }
  if (jitter) block_sum_add(l, (unsigned*)(pl + P_LSUM));
}

// staged: `in` is the flipped stage image (cimg for the images that were cropped); else `in` is the vertical pass's input
// and the flip happens here, as in resize_v_norm_kernel.  The float expression is that kernel's.
__global__ __launch_bounds__(256) void augment_final_kernel(const uint8_t* __restrict__ in, const uint8_t* __restrict__ cimg,
                                                            float* __restrict__ dst, const int* __restrict__ bounds,
                                                            const int* __restrict__ kk, int ksize, int Hin, int Ho, int Wo,
                                                            int yshift, const int32_t* __restrict__ plan, int stages,
                                                            int staged, float m0, float m1, float m2, float s0, float s1,
                                                            float s2) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const int64_t n = blockIdx.y;
  if (pix >= Ho * Wo) return;
  const int32_t* pl = plan + n * PLAN_WORDS;
  const int yy = pix / Wo, xx = pix - yy * Wo;
  int u0, u1, u2, xo = xx;
  if (staged) {
    const uint8_t* from = ((stages & ST_CROP) && pl[P_CROP]) ? cimg : in;
    vertical_px(from, nullptr, nullptr, 0, Ho, Wo, 0, n, yy, xx, u0, u1, u2);
  } else {
    vertical_px(in, bounds, kk, ksize, Hin, Wo, yshift, n, yy, xx, u0, u1, u2);
    if ((stages & ST_FLIP) && pl[P_FLIP]) xo = Wo - 1 - xx;
  }
  if (stages & ST_JITTER) {
    const float b = __int_as_float(pl[P_B]), c = __int_as_float(pl[P_C]);
    const int grey = (int)((double)(unsigned)pl[P_LSUM] / (double)(Ho * Wo) + 0.5);   // int(ImageStat mean + 0.5)
    if (pl[P_FIRST] == 0) { u0 = blend8(0, u0, b); u1 = blend8(0, u1, b); u2 = blend8(0, u2, b); }
    u0 = blend8(grey, u0, c); u1 = blend8(grey, u1, c); u2 = blend8(grey, u2, c);
    if (pl[P_FIRST] != 0) { u0 = blend8(0, u0, b); u1 = blend8(0, u1, b); u2 = blend8(0, u2, b); }
  }
  float f0 = ((float)u0 / 255.0f - m0) / s0;          // ToTensor: u8 -> f32, div(255); Normalize: sub(mean).div(std)
  float f1 = ((float)u1 / 255.0f - m1) / s1;
  float f2 = ((float)u2 / 255.0f - m2) / s2;
  if ((stages & ST_ERASE) && pl[P_EH] > 0 && yy >= pl[P_R0] && yy < pl[P_R0] + pl[P_EH] && xo >= pl[P_C0] &&
      xo < pl[P_C0] + pl[P_EW]) {
    f0 = m0; f1 = m1; f2 = m2;                        // RandomErasing(mean=norm_mean): the mean itself, not normalised
  }
  const int64_t plane = (int64_t)Ho * Wo;
  float* o = dst + n * 3 * plane + (int64_t)yy * Wo + xo;
  o[0] = f0;
  o[plane] = f1;
  o[2 * plane] = f2;
}

// ---- ragged batch (ieee_resize_normalize_ragged): N images, each with its own (Hs, Ws), in ONE launch and with no host
// tables.  A workgroup owns (image, band of R output rows): it computes Pillow's coefficients of every output column and of
// its own output rows (axis_row below), runs the horizontal pass over the source rows its band reads into LDS (one packed
// RGBx word per pixel, rounded to 8 bits like the uint8 intermediate of the two-launch form), then the vertical pass, the
// flip and the normalisation out of LDS.  A band whose source rows exceed the LDS rows of the launch is done in groups of
// output rows.  An axis that keeps its size gets the weight rows {1 << 22, 0}: the pass returns its input.

// Pillow's precompute_coeffs + normalize_coeffs_8bpc (bilinear) for output index xx of one axis, as _axis_tables
// (ieee_amd/data/transforms.py) restates them: fp64, the scale from the float32 of the size, ww summed left to right,
// weights trunc(+-0.5 + k * 2^22).  Every product feeds a sum here: contraction into an fma would change the bits, so it is
// off for this function.  bnd = (first source index, count <= cap); k[0 .. count) = weights; zero_to > count: k is zero-filled
// up to there (the table form).
__host__ __device__ inline int axis_ksize(int in_size, int out_size) {
  const double scale = (double)((float)in_size - 0.0f) / (double)out_size;
  const double support = scale > 1.0 ? scale : 1.0;
  return (int)ceil(support) * 2 + 1;
}

__device__ __forceinline__ void axis_row(int in_size, int out_size, int xx, int cap, int zero_to, int* __restrict__ bnd,
                                         int* __restrict__ k) {
#pragma clang fp contract(off)
  const double scale = (double)((float)in_size - 0.0f) / (double)out_size;
  const double filterscale = scale > 1.0 ? scale : 1.0;
  const double support = 1.0 * filterscale;
  const double inv = 1.0 / filterscale;
  const double center = ((double)xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  if (xmax > cap) xmax = cap;            // never taken: xmax <= ksize <= cap (the host checked); keeps the writes inside k
  if (xmax < 0) xmax = 0;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) {
    double w = fabs(((double)(x + xmin) - center + 0.5) * inv);
    w = w < 1.0 ? 1.0 - w : 0.0;
    ww += w;
  }
  for (int x = 0; x < xmax; ++x) {
    double w = fabs(((double)(x + xmin) - center + 0.5) * inv);
    w = w < 1.0 ? 1.0 - w : 0.0;
    if (ww != 0.0) w = w / ww;
    k[x] = (int)(w < 0.0 ? -0.5 + w * (double)(1 << PRECISION_BITS) : 0.5 + w * (double)(1 << PRECISION_BITS));
  }
  for (int x = xmax; x < zero_to; ++x) k[x] = 0;
  bnd[0] = xmin;
  bnd[1] = xmax;
}

__global__ __launch_bounds__(256) void resample_coeffs_kernel(int in_size, int out_size, int ksize, int* __restrict__ bounds,
                                                              int* __restrict__ kk) {
  const int xx = blockIdx.x * 256 + threadIdx.x;
  if (xx < out_size) axis_row(in_size, out_size, xx, ksize, ksize, bounds + 2 * xx, kk + (int64_t)xx * ksize);
}

// LDS (ints): bh [Wo][2] | kh [Wo][ksh_cap] | bv [R][2] | kv [R][ksv_cap] | tmp [cap_rows][Wo] (RGBx words).  An image's
// tables use its own ksize as the row stride (odd: consecutive columns fall on different banks).
__global__ __launch_bounds__(256) void resize_ragged_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                            const int64_t* __restrict__ offsets,
                                                            const int32_t* __restrict__ sizes,
                                                            const uint8_t* __restrict__ flip, float* __restrict__ dst, int Ho,
                                                            int Wo, int R, int nbands, int ksh_cap, int ksv_cap, int cap_rows,
                                                            float m0, float m1, float m2, float s0, float s1, float s2) {
  extern __shared__ __attribute__((aligned(16))) int ragged_lds[];
  int* bh = ragged_lds;
  int* kh = bh + 2 * Wo;
  int* bv = kh + Wo * ksh_cap;
  int* kv = bv + 2 * R;
  uint32_t* tmp = (uint32_t*)(kv + R * ksv_cap);
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.x / nbands;
  const int band = blockIdx.x - (int)n * nbands;
  const int Hs = sizes[2 * n], Ws = sizes[2 * n + 1];
  const int64_t off = offsets[n];
  // the device tables are the caller's copy of what the host checked; a copy that disagrees leaves the image unwritten
  // rather than reading or writing outside the buffers (block-uniform: no barrier is skipped by part of a block)
  if (Hs < 1 || Ws < 1 || off < 0 || off + (int64_t)Hs * Ws * 3 > src_bytes) return;
  const int ksh = axis_ksize(Ws, Wo), ksv = axis_ksize(Hs, Ho);
  if (ksh > ksh_cap || ksv > ksv_cap || ksv > cap_rows) return;
  const uint8_t* img = src + off;
  const int y0 = band * R, y1 = min(y0 + R, Ho);
  for (int i = tid; i < Wo + (y1 - y0); i += 256) {
    if (i < Wo) axis_row(Ws, Wo, i, ksh, 0, bh + 2 * i, kh + i * ksh);
    else axis_row(Hs, Ho, y0 + (i - Wo), ksv, 0, bv + 2 * (i - Wo), kv + (i - Wo) * ksv);
  }
  __syncthreads();
  const bool flipped = flip != nullptr && flip[n];
  const int64_t plane = (int64_t)Ho * Wo;
  float* out = dst + n * 3 * plane;
  int g0 = y0;
  while (g0 < y1) {
    // the output rows g0 .. g1 whose source rows rb .. rb + rows fit the LDS rows (first index and end both grow with yy)
    const int rb = bv[2 * (g0 - y0)];
    int g1 = g0 + 1;
    while (g1 < y1 && bv[2 * (g1 - y0)] + bv[2 * (g1 - y0) + 1] - rb <= cap_rows) ++g1;
    const int rows = min(bv[2 * (g1 - 1 - y0)] + bv[2 * (g1 - 1 - y0) + 1] - rb, cap_rows);
    for (int i = tid; i < rows * Wo; i += 256) {          // horizontal pass: lanes along the output columns
      const int r = i / Wo, xx = i - r * Wo;
      const int xmin = bh[2 * xx], cnt = bh[2 * xx + 1];
      const uint8_t* p = img + ((int64_t)(rb + r) * Ws + xmin) * 3;
      const int* k = kh + xx * ksh;
      int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
      for (int x = 0; x < cnt; ++x) {
        const int w = k[x];
        a0 += p[3 * x] * w;
        a1 += p[3 * x + 1] * w;
        a2 += p[3 * x + 2] * w;
      }
      tmp[i] = (uint32_t)clip8(a0) | ((uint32_t)clip8(a1) << 8) | ((uint32_t)clip8(a2) << 16);
    }
    __syncthreads();
    for (int i = tid; i < (g1 - g0) * Wo; i += 256) {     // vertical pass, flip, ToTensor, Normalize
      const int j = i / Wo, xx = i - j * Wo;
      const int yy = g0 + j;
      const int ymin = bv[2 * (yy - y0)] - rb, cnt = min(bv[2 * (yy - y0) + 1], rows - ymin);
      const int* k = kv + (yy - y0) * ksv;
      const uint32_t* q = tmp + ymin * Wo + xx;
      int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
      for (int y = 0; y < cnt; ++y) {
        const int w = k[y];
        const uint32_t v = q[y * Wo];
        a0 += (int)(v & 255u) * w;
        a1 += (int)((v >> 8) & 255u) * w;
        a2 += (int)((v >> 16) & 255u) * w;
      }
      const uint8_t u0 = clip8(a0), u1 = clip8(a1), u2 = clip8(a2);
      const int xo = flipped ? Wo - 1 - xx : xx;
      float* o = out + (int64_t)yy * Wo + xo;
      o[0] = ((float)u0 / 255.0f - m0) / s0;          // the float expression of resize_v_norm_kernel
      o[plane] = ((float)u1 / 255.0f - m1) / s1;
      o[2 * plane] = ((float)u2 / 255.0f - m2) / s2;
    }
    __syncthreads();
    g0 = g1;
  }
}

}  // namespace ieee

using namespace ieee;

extern "C" int ieee_resize_flip_normalize(const uint8_t* src, float* dst, uint8_t* tmp, int64_t N, int64_t Hs,
                                          int64_t Ws, int64_t Ho, int64_t Wo, const int32_t* bounds_h,
                                          const int32_t* kk_h, int64_t ksize_h, const int32_t* bounds_v,
                                          const int32_t* kk_v, int64_t ksize_v, int64_t ybox_first, int64_t tmp_rows,
                                          const uint8_t* flip, const float* mean3, const float* std3, void* stream) {
  IEEE_REQUIRE(src && dst && mean3 && std3, "resize_flip_normalize: null pointer");
  IEEE_REQUIRE(N > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, "resize_flip_normalize: empty images");
  IEEE_REQUIRE((kk_h == nullptr) == (Ws == Wo), "resize_flip_normalize: the horizontal table is needed iff the width changes");
  IEEE_REQUIRE((kk_v == nullptr) == (Hs == Ho), "resize_flip_normalize: the vertical table is needed iff the height changes");
  IEEE_REQUIRE(kk_h == nullptr || (bounds_h && tmp && tmp_rows > 0 && ybox_first >= 0 && ybox_first + tmp_rows <= Hs),
               "resize_flip_normalize: bad horizontal-pass arguments");
  IEEE_REQUIRE(kk_v == nullptr || bounds_v, "resize_flip_normalize: vertical bounds missing");
  hipStream_t st = (hipStream_t)stream;
  const uint8_t* vin = src;
  int64_t Hin = Hs, yshift = 0;
  if (kk_h != nullptr) {
    const int64_t total = N * tmp_rows * Wo;
    resize_h_kernel<<<(unsigned)cdiv(total, 256), 256, 0, st>>>(src, tmp, bounds_h, kk_h, (int)ksize_h, (int)Hs, (int)Ws,
                                                               (int)Wo, (int)ybox_first, (int)tmp_rows, total);
    IEEE_TRY(launch_status("resize_h_kernel"));
    vin = tmp;
    Hin = tmp_rows;
    yshift = ybox_first;
  }
  const int64_t total = N * Ho * Wo;
  resize_v_norm_kernel<<<(unsigned)cdiv(total, 256), 256, 0, st>>>(vin, dst, bounds_v, kk_v, (int)ksize_v, (int)Hin, (int)Ho,
                                                                  (int)Wo, (int)yshift, flip, mean3[0], mean3[1], mean3[2],
                                                                  std3[0], std3[1], std3[2], total);
  return launch_status("resize_v_norm_kernel");
}

extern "C" int ieee_augment_normalize(const uint8_t* src, float* dst, uint8_t* tmp, int64_t N, int64_t Hs, int64_t Ws,
                                      int64_t Ho, int64_t Wo, const int32_t* bounds_h, const int32_t* kk_h, int64_t ksize_h,
                                      const int32_t* bounds_v, const int32_t* kk_v, int64_t ksize_v, int64_t ybox_first,
                                      int64_t tmp_rows, int32_t* plan, int stages, uint8_t* work, int64_t work_bytes,
                                      int64_t Hbig, int64_t Wbig, const int32_t* big_bounds_h, const int32_t* big_kk_h,
                                      int64_t big_ksize_h, const int32_t* big_bounds_v, const int32_t* big_kk_v,
                                      int64_t big_ksize_v, const float* mean3, const float* std3, int* launches,
                                      void* stream) {
  IEEE_REQUIRE(src && dst && mean3 && std3 && plan, "augment_normalize: null pointer");
  IEEE_REQUIRE(N > 0 && N <= 65535 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0 && Ho * Wo <= (1 << 24),
               "augment_normalize: 1 .. 65535 images of at most 2^24 output pixels");
  IEEE_REQUIRE(stages >= 0 && stages < 16, "augment_normalize: unknown stage bits");
  IEEE_REQUIRE((kk_h == nullptr) == (Ws == Wo), "augment_normalize: the horizontal table is needed iff the width changes");
  IEEE_REQUIRE((kk_v == nullptr) == (Hs == Ho), "augment_normalize: the vertical table is needed iff the height changes");
  IEEE_REQUIRE(kk_h == nullptr || (bounds_h && tmp && tmp_rows > 0 && ybox_first >= 0 && ybox_first + tmp_rows <= Hs),
               "augment_normalize: bad horizontal-pass arguments");
  IEEE_REQUIRE(kk_v == nullptr || bounds_v, "augment_normalize: vertical bounds missing");
  const bool crop = stages & ST_CROP, jitter = stages & ST_JITTER, staged = crop || jitter;
  const int64_t image = N * Ho * Wo * 3;
  IEEE_REQUIRE(!staged || (work && work_bytes >= (crop ? 3 : 1) * image), "augment_normalize: work buffer too small");
  IEEE_REQUIRE(!crop || (big_bounds_h && big_kk_h && big_bounds_v && big_kk_v && big_ksize_h > 0 && big_ksize_v > 0 &&
                         Hbig > Ho && Wbig > Wo),
               "augment_normalize: the crop needs both enlargement tables and Hbig > Ho, Wbig > Wo");
  hipStream_t st = (hipStream_t)stream;
  int count = 0;
  if (launches) *launches = 0;
  const uint8_t* vin = src;
  int64_t Hin = Hs, yshift = 0;
  if (kk_h != nullptr) {
    const int64_t total = N * tmp_rows * Wo;
    resize_h_kernel<<<(unsigned)cdiv(total, 256), 256, 0, st>>>(src, tmp, bounds_h, kk_h, (int)ksize_h, (int)Hs, (int)Ws,
                                                               (int)Wo, (int)ybox_first, (int)tmp_rows, total);
    IEEE_TRY(launch_status("resize_h_kernel"));
    ++count;
    vin = tmp;
    Hin = tmp_rows;
    yshift = ybox_first;
  }
  const dim3 grid((unsigned)cdiv(Ho * Wo, 256), (unsigned)N);
  uint8_t* stage = work;
  uint8_t* ctmp = crop ? work + image : nullptr;
  uint8_t* cimg = crop ? work + 2 * image : nullptr;
  if (staged) {
    augment_stage_kernel<<<grid, 256, 0, st>>>(vin, stage, bounds_v, kk_v, (int)ksize_v, (int)Hin, (int)Ho, (int)Wo,
                                               (int)yshift, plan, stages, jitter && !crop);
    IEEE_TRY(launch_status("augment_stage_kernel"));
    ++count;
  }
  if (crop) {
    augment_crop_h_kernel<<<grid, 256, 0, st>>>(stage, ctmp, big_bounds_h, big_kk_h, (int)big_ksize_h, big_bounds_v, (int)Ho,
                                                (int)Wo, (int)Hbig, (int)Wbig, plan);
    IEEE_TRY(launch_status("augment_crop_h_kernel"));
    augment_crop_v_kernel<<<grid, 256, 0, st>>>(stage, ctmp, cimg, big_bounds_v, big_kk_v, (int)big_ksize_v, (int)Ho, (int)Wo,
                                                (int)Hbig, plan, stages);
    IEEE_TRY(launch_status("augment_crop_v_kernel"));
    count += 2;
  }
  augment_final_kernel<<<grid, 256, 0, st>>>(staged ? stage : vin, cimg, dst, bounds_v, kk_v, (int)ksize_v, (int)Hin, (int)Ho,
                                             (int)Wo, (int)yshift, plan, stages, staged, mean3[0], mean3[1], mean3[2],
                                             std3[0], std3[1], std3[2]);
  IEEE_TRY(launch_status("augment_final_kernel"));
  if (launches) *launches = count + 1;
  return 0;
}

constexpr int RAGGED_MAX_SIDE = 4096;
constexpr int64_t RAGGED_LDS_BYTES = 64 * 1024;

extern "C" int ieee_resample_ksize(int64_t in_size, int64_t out_size) {
  if (in_size < 1 || in_size > RAGGED_MAX_SIDE || out_size < 1 || out_size > RAGGED_MAX_SIDE) return 0;
  return axis_ksize((int)in_size, (int)out_size);
}

extern "C" int ieee_resample_coeffs(int64_t in_size, int64_t out_size, int32_t* bounds, int32_t* kk, int64_t ksize,
                                    void* stream) {
  IEEE_REQUIRE(bounds && kk, "resample_coeffs: null pointer");
  IEEE_REQUIRE(in_size >= 1 && in_size <= RAGGED_MAX_SIDE && out_size >= 1 && out_size <= RAGGED_MAX_SIDE,
               "resample_coeffs: sizes of 1 .. 4096");
  IEEE_REQUIRE(ksize == axis_ksize((int)in_size, (int)out_size), "resample_coeffs: ksize is not ieee_resample_ksize(in, out)");
  resample_coeffs_kernel<<<(unsigned)cdiv(out_size, 256), 256, 0, (hipStream_t)stream>>>((int)in_size, (int)out_size,
                                                                                        (int)ksize, bounds, kk);
  return launch_status("resample_coeffs_kernel");
}

extern "C" int ieee_resize_normalize_ragged(const uint8_t* src, int64_t src_bytes, const int64_t* offsets,
                                            const int32_t* sizes, const uint8_t* flip, const int64_t* host_offsets,
                                            const int32_t* host_sizes, float* dst, int64_t N, int64_t Ho, int64_t Wo,
                                            const float* mean3, const float* std3, int* launches, void* stream) {
  if (launches) *launches = 0;
  IEEE_REQUIRE(N >= 0, "resize_normalize_ragged: negative image count");
  if (N == 0) return IEEE_OK;
  IEEE_REQUIRE(src && offsets && sizes && host_offsets && host_sizes && dst && mean3 && std3,
               "resize_normalize_ragged: null pointer");
  IEEE_REQUIRE(Ho >= 1 && Ho <= RAGGED_MAX_SIDE && Wo >= 1 && Wo <= RAGGED_MAX_SIDE,
               "resize_normalize_ragged: output sides of 1 .. 4096");
  int ksh_cap = 3, ksv_cap = 3;
  double vscale = 0.0;
  for (int64_t i = 0; i < N; ++i) {
    const int64_t hs = host_sizes[2 * i], ws = host_sizes[2 * i + 1], off = host_offsets[i];
    IEEE_REQUIRE(hs >= 1 && ws >= 1, "resize_normalize_ragged: image %lld is empty (%lld x %lld)", (long long)i, (long long)hs,
                 (long long)ws);
    if (hs > RAGGED_MAX_SIDE || ws > RAGGED_MAX_SIDE) {
      set_error(IEEE_ERR_UNSUPPORTED, "resize_normalize_ragged: image %lld is %lld x %lld; source sides of 1 .. 4096 are supported",
                (long long)i, (long long)hs, (long long)ws);
      return IEEE_ERR_UNSUPPORTED;
    }
    IEEE_REQUIRE(off >= 0 && off + hs * ws * 3 <= src_bytes, "resize_normalize_ragged: image %lld lies outside the %lld source bytes",
                 (long long)i, (long long)src_bytes);
    ksh_cap = std::max(ksh_cap, axis_ksize((int)ws, (int)Wo));
    ksv_cap = std::max(ksv_cap, axis_ksize((int)hs, (int)Ho));
    vscale = std::max(vscale, (double)hs / (double)Ho);
  }
  // the band height: the largest of 16, 8, .. 1 output rows whose tables leave LDS rows for one output row's window at least
  const double vsupport = std::max(vscale, 1.0);
  int R = 16;
  int64_t cap_rows = 0, fixed = 0;
  for (;; R >>= 1) {
    fixed = 4 * (2 * Wo + Wo * ksh_cap + 2 * (int64_t)R + (int64_t)R * ksv_cap);
    cap_rows = fixed < RAGGED_LDS_BYTES ? (RAGGED_LDS_BYTES - fixed) / (4 * Wo) : 0;
    if (cap_rows >= ksv_cap || R == 1) break;
  }
  if (cap_rows < ksv_cap) {
    set_error(IEEE_ERR_UNSUPPORTED, "resize_normalize_ragged: the tables of a %lld x %lld output for these sources (%d and %d taps) "
              "and one output row's window do not fit 64 KiB of LDS", (long long)Ho, (long long)Wo, ksh_cap, ksv_cap);
    return IEEE_ERR_UNSUPPORTED;
  }
  // no more LDS rows than the tallest band reads (an upper bound; the kernel splits a band that needs more than it got)
  const int64_t need = (int64_t)ceil((R - 1) * vscale + 2.0 * vsupport) + 2;
  cap_rows = std::max<int64_t>(ksv_cap, std::min(cap_rows, need));
  const int64_t nbands = (Ho + R - 1) / R;
  IEEE_REQUIRE(N * nbands <= 0x7fffffffLL, "resize_normalize_ragged: too many images");
  const size_t lds = (size_t)(fixed + cap_rows * 4 * Wo);
  resize_ragged_kernel<<<(unsigned)(N * nbands), 256, lds, (hipStream_t)stream>>>(
      src, src_bytes, offsets, sizes, flip, dst, (int)Ho, (int)Wo, R, (int)nbands, ksh_cap, ksv_cap, (int)cap_rows, mean3[0],
      mean3[1], mean3[2], std3[0], std3[1], std3[2]);
  IEEE_TRY(launch_status("resize_ragged_kernel"));
  if (launches) *launches = 1;
  return IEEE_OK;
}
