// Input pipeline on the device: the reference's per-image transform chain
//   Resize((H,W)) [PIL bilinear, antialiased] -> RandomHorizontalFlip -> ToTensor -> Normalize
// (torchreid/data/transforms.py:233-326, applied to every modality image separately in
// data/datasets/dataset.py:335-351) for a whole batch of decoded uint8 HWC images in two launches.
// The resize is Pillow's two-pass 8-bit resampler reproduced bit for bit: 22-bit fixed-point weights (computed on
// the host exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc do, ieee_amd/data/transforms.py), int32
// accumulation with the rounding bias, 8-bit clip after EACH pass (the horizontal pass writes a uint8 intermediate).
// Byte/integer work bound by HBM: nothing here belongs on the matrix cores.
#include "common.h"

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
