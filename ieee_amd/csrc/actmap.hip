// Activation maps: where the trunk looks.  Reference: tools/visualize_actmap.py:84-88 (channel energy of the last
// convolutional map, L2-normalised per image) and :119-146 (resize to the image size, min-max scaling, colour table,
// overlay, the three-panel figure).  Two kernels, one workgroup per image each; the map never leaves the device and only
// finished bytes are written.  Both are bandwidth- and latency-shaped: no MFMA.
#include "common.h"

// The render arithmetic is specified operation by operation (include/ieee_amd.h) so that a host restatement reproduces
// every byte: no product-sum of this file may be contracted into a fused multiply-add (the division and square-root
// sequences keep their own).
#pragma clang fp contract(off)

namespace ieee {

constexpr int AM_MAX_P = 4096;        // positions of one map: its energies (16 KB) stay in LDS
constexpr int AM_E_THREADS = 1024;    // 16 waves keep about 64 KB of 16-byte loads in flight per workgroup
constexpr int AM_E_WAVES = AM_E_THREADS / 64;
constexpr int AM_R_THREADS = 1024;
constexpr int AM_R_WAVES = AM_R_THREADS / 64;
constexpr int AM_GAP = 10;            // GRID_SPACING, visualize_actmap.py:22
constexpr int AM_STAGE = 24576;       // finished figure rows wait here (LDS) and leave as whole dwords
constexpr int AM_MAX_WIDTH = 2048;    // one figure row, (3 * width + 20) * 3 bytes, fits the stage

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}

// E[p] = sum_c x[n][p][c]^2, then E / max(||E||_2, 1e-12).  A wave owns a position, its lanes take 16-byte chunks of the
// channel row in a fixed order; lane sums meet in the xor butterfly (every lane ends with the same bits), wave sums of
// the norm in LDS, added in wave order by every thread: no atomics, the same bits on every call.
template <typename T>
__global__ __launch_bounds__(AM_E_THREADS) void actmap_energy_kernel(const T* __restrict__ x, int P, int C,
                                                                     float* __restrict__ out) {
  constexpr int V = Vec16<T>::N;
  __shared__ float E[AM_MAX_P];
  __shared__ float part[AM_E_WAVES];
  const int n = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int chunks = C / V;
  const uint4* img = reinterpret_cast<const uint4*>(x + (int64_t)n * P * C);
  for (int p = wave; p < P; p += AM_E_WAVES) {
    const uint4* row = img + (int64_t)p * chunks;
    float acc = 0.f;
#pragma unroll 4
    for (int k = lane; k < chunks; k += 64) {
      const uint4 v = row[k];
      float f[V];
      Vec16<T>::unpack(v, f);
#pragma unroll
      for (int e = 0; e < V; ++e) acc += f[e] * f[e];
    }
    acc = wave_sum(acc);
    if (lane == 0) E[p] = acc;
  }
  __syncthreads();
  float s = 0.f;
  for (int p = t; p < P; p += AM_E_THREADS) s += E[p] * E[p];
  s = wave_sum(s);
  if (lane == 0) part[wave] = s;
  __syncthreads();
  float total = 0.f;
#pragma unroll
  for (int i = 0; i < AM_E_WAVES; ++i) total += part[i];
  const float den = fmaxf(sqrtf(total), 1e-12f);   // F.normalize's eps: a zero map gives zeros
  float* o = out + (int64_t)n * P;
  for (int p = t; p < P; p += AM_E_THREADS) o[p] = E[p] / den;
}

struct ActmapRender {
  const float* amap;
  const float* img;
  const uint8_t* lut;
  uint8_t* grid;
  uint8_t* index;
  int h, w, height, width;
  float mean[3], std[3];
};

// OpenCV's INTER_LINEAR sampling position of destination coordinate d: source index and weight of its successor;
// clamped with weight 0 at both edges
__device__ __forceinline__ void am_coord(int d, float ratio, int n, int& i0, int& i1, float& f) {
  const float s = ((float)d + 0.5f) * ratio - 0.5f;
  const float fl = floorf(s);
  i0 = (int)fl;
  f = s - fl;
  if (i0 < 0) { i0 = 0; f = 0.f; }
  if (i0 >= n - 1) { i0 = n - 1; f = 0.f; }
  i1 = min(i0 + 1, n - 1);
}

// one resized value: rows y0 / y1 interpolated horizontally, then the two results vertically, a + (b - a) * f each
__device__ __forceinline__ float am_sample(const float* m, int w, int y0, int y1, float fy, int x0, int x1, float fx) {
  const float a0 = m[y0 * w + x0], b0 = m[y0 * w + x1];
  const float a1 = m[y1 * w + x0], b1 = m[y1 * w + x1];
  const float r0 = a0 + (b0 - a0) * fx;
  const float r1 = a1 + (b1 - a1) * fx;
  return r0 + (r1 - r0) * fy;
}

// nbytes of LDS to global memory by the whole workgroup: bytes up to the first 4-byte boundary of dst, whole dwords, the
// rest in bytes (a figure's rows are 3-byte pixels at any alignment; byte stores alone leave most of a wave's store
// width unused)
__device__ __forceinline__ void am_copy_out(uint8_t* __restrict__ dst, const uint8_t* src, int nbytes, int t) {
  const int head = min(nbytes, (int)((4 - ((uintptr_t)dst & 3)) & 3));
  const int nd = (nbytes - head) >> 2;
  for (int i = t; i < head; i += AM_R_THREADS) dst[i] = src[i];
  uint32_t* d4 = reinterpret_cast<uint32_t*>(dst + head);
  if (head == 0) {
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);
    for (int k = t; k < nd; k += AM_R_THREADS) d4[k] = s4[k];
  } else {
    for (int k = t; k < nd; k += AM_R_THREADS) {
      const uint8_t* b = src + head + 4 * k;
      d4[k] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    }
  }
  for (int i = head + 4 * nd + t; i < nbytes; i += AM_R_THREADS) dst[i] = src[i];
}

// The small map and the colour table are staged in LDS.  Pass 1: min and max of the RESIZED map (half-pixel centres
// never sample a source extremum when upsampling, so the source's own extrema are not the figure's).  Pass 2: every
// pixel again, scaled and looked up; image, coloured map, overlay and the two white gaps of as many rows as fit are
// assembled in LDS and written out together (the rows of a figure are contiguous), the indices likewise.
__global__ __launch_bounds__(AM_R_THREADS) void actmap_render_kernel(ActmapRender a) {
  __shared__ float m[AM_MAX_P];
  __shared__ __attribute__((aligned(16))) uint8_t stage[AM_STAGE];
  __shared__ __attribute__((aligned(16))) uint8_t istage[AM_STAGE / 8];
  __shared__ uint8_t lut[768];
  __shared__ float s_mn[AM_R_WAVES], s_mx[AM_R_WAVES];
  const int n = blockIdx.x, t = threadIdx.x;
  const int hw = a.h * a.w, HW = a.height * a.width;
  for (int i = t; i < hw; i += AM_R_THREADS) m[i] = a.amap[(int64_t)n * hw + i];
  for (int i = t; i < 768; i += AM_R_THREADS) lut[i] = a.lut[i];
  __syncthreads();
  const float ry = (float)a.h / (float)a.height, rx = (float)a.w / (float)a.width;

  auto value = [&](int i, int& dy, int& dx) {
    dy = i / a.width;
    dx = i - dy * a.width;
    int y0, y1, x0, x1;
    float fy, fx;
    am_coord(dy, ry, a.h, y0, y1, fy);
    am_coord(dx, rx, a.w, x0, x1, fx);
    return am_sample(m, a.w, y0, y1, fy, x0, x1, fx);
  };

  float mn = __uint_as_float(0x7F800000u), mx = __uint_as_float(0xFF800000u);
  for (int i = t; i < HW; i += AM_R_THREADS) {
    int dy, dx;
    const float v = value(i, dy, dx);
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  if ((t & 63) == 0) { s_mn[t >> 6] = mn; s_mx[t >> 6] = mx; }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < AM_R_WAVES; ++i) { mn = fminf(mn, s_mn[i]); mx = fmaxf(mx, s_mx[i]); }
  const float den = (mx - mn) + 1e-12f;

  const int GW = 3 * a.width + 2 * AM_GAP, row_bytes = GW * 3, gap_bytes = AM_GAP * 3;
  const int R = min(a.height, AM_STAGE / row_bytes);   // rows per round; >= 1 (width <= AM_MAX_WIDTH), R * width <= AM_STAGE / 9
  uint8_t* grid = a.img ? a.grid + (int64_t)n * a.height * row_bytes : nullptr;
  for (int r0 = 0; r0 < a.height; r0 += R) {
    const int rows = min(R, a.height - r0);
    for (int j = t; j < rows * a.width; j += AM_R_THREADS) {
      int dy, dx;
      const float v = value(r0 * a.width + j, dy, dx);
      const float q = floorf(255.f * (v - mn) / den);
      const int idx = (int)fminf(fmaxf(q, 0.f), 255.f);   // (a NaN map gives index 0)
      istage[j] = (uint8_t)idx;
      if (!grid) continue;
      uint8_t* row = stage + (dy - r0) * row_bytes;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float x = a.img[((int64_t)(n * 3 + c) * a.height + dy) * a.width + dx];
        const float u = fminf(fmaxf(x * a.std[c] + a.mean[c], 0.f), 1.f);
        const int pix = (int)floorf(u * 255.f);
        const int col = lut[idx * 3 + c];
        const double ov = fmin(0.3 * (double)pix + 0.7 * (double)col, 255.0);
        row[dx * 3 + c] = (uint8_t)pix;
        row[(a.width + AM_GAP + dx) * 3 + c] = (uint8_t)col;
        row[(2 * a.width + 2 * AM_GAP + dx) * 3 + c] = (uint8_t)(int)ov;
      }
    }
    if (grid) {
      for (int j = t; j < rows * 2 * gap_bytes; j += AM_R_THREADS) {
        const int r = j / (2 * gap_bytes), g = j - r * 2 * gap_bytes;
        const int col_byte = g < gap_bytes ? a.width * 3 + g : (2 * a.width + AM_GAP) * 3 + (g - gap_bytes);
        stage[r * row_bytes + col_byte] = 255;
      }
    }
    __syncthreads();
    if (grid) am_copy_out(grid + (int64_t)r0 * row_bytes, stage, rows * row_bytes, t);
    if (a.index) am_copy_out(a.index + (int64_t)n * HW + (int64_t)r0 * a.width, istage, rows * a.width, t);
    __syncthreads();
  }
}

}  // namespace ieee

using namespace ieee;

extern "C" int ieee_actmap_energy(const void* x, int dtype, int64_t N, int64_t P, int64_t C, float* out, void* stream) {
  IEEE_REQUIRE(dtype == IEEE_F32 || dtype == IEEE_BF16, "actmap_energy: dtype %d is neither IEEE_F32 nor IEEE_BF16", dtype);
  IEEE_REQUIRE(N >= 0 && N < (1ll << 31), "actmap_energy: N = %ld out of range", (long)N);
  IEEE_REQUIRE(P >= 1 && P <= AM_MAX_P, "actmap_energy: P = %ld out of range [1, %d]", (long)P, AM_MAX_P);
  IEEE_REQUIRE(C >= 8 && C % 8 == 0 && C < (1ll << 24), "actmap_energy: C = %ld must be a multiple of 8", (long)C);
  if (N == 0) return IEEE_OK;
  IEEE_REQUIRE(x && out, "actmap_energy: null pointer");
  IEEE_REQUIRE(((uintptr_t)x & 15) == 0, "actmap_energy: x must be 16-byte aligned");
  if (dtype == IEEE_BF16)
    actmap_energy_kernel<bf16><<<(int)N, AM_E_THREADS, 0, (hipStream_t)stream>>>((const bf16*)x, (int)P, (int)C, out);
  else
    actmap_energy_kernel<float><<<(int)N, AM_E_THREADS, 0, (hipStream_t)stream>>>((const float*)x, (int)P, (int)C, out);
  return launch_status("actmap_energy");
}

extern "C" int ieee_actmap_render(const float* amap, int64_t h, int64_t w, const float* img, const float* mean3,
                                  const float* std3, const uint8_t* lut, int64_t N, int64_t height, int64_t width,
                                  uint8_t* grid_out, uint8_t* index_out, void* stream) {
  IEEE_REQUIRE(N >= 0 && N < (1ll << 29), "actmap_render: N = %ld out of range", (long)N);
  IEEE_REQUIRE(h >= 1 && w >= 1 && h * w <= AM_MAX_P, "actmap_render: map %ld x %ld (at most %d positions)", (long)h, (long)w,
               AM_MAX_P);
  IEEE_REQUIRE(height >= 1 && height < (1ll << 18) && width >= 1 && width <= AM_MAX_WIDTH,
               "actmap_render: figure %ld x %ld out of range (width at most %d)", (long)height, (long)width, AM_MAX_WIDTH);
  if (N == 0) return IEEE_OK;
  IEEE_REQUIRE(amap && lut, "actmap_render: null map or colour table");
  IEEE_REQUIRE(img ? (grid_out && mean3 && std3) : index_out != nullptr,
               "actmap_render: with an image grid_out, mean3 and std3 are needed, without one index_out");
  ActmapRender a;
  a.amap = amap; a.img = img; a.lut = lut; a.grid = grid_out; a.index = index_out;
  a.h = (int)h; a.w = (int)w; a.height = (int)height; a.width = (int)width;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = img ? mean3[c] : 0.f;
    a.std[c] = img ? std3[c] : 1.f;
  }
  actmap_render_kernel<<<(int)N, AM_R_THREADS, 0, (hipStream_t)stream>>>(a);
  return launch_status("actmap_render");
}
