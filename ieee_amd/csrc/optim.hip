// Element-wise optimizer updates over flat fp32 ranges: RMSprop and the reference's RAdam (gfx950 / MI355X only).
// Both have the shape of sgd_nesterov_kernel (head.hip): 16 bytes per lane when every pointer allows it, a scalar form with
// the same per-element arithmetic otherwise and for the tail, a grid-stride loop under a capped grid.  Division and square
// root are the compiler's default (correctly rounded) forms.
#include <math.h>
#include <stdlib.h>

#include "common.h"

namespace ieee {

// torch.optim.RMSprop(alpha, eps, weight_decay, momentum, centered=False), torch/optim/rmsprop.py::_single_tensor_rmsprop
// (reference optim/optimizer.py:140-147)
__device__ __forceinline__ void rmsprop_one(float& w, float g, float& sq, float& buf, float lr, float alpha, float eps, float wd,
                                            float momentum) {
  const float d = g + wd * w;
  const float s = alpha * sq + (1.f - alpha) * d * d;
  sq = s;
  const float q = d / (sqrtf(s) + eps);
  if (momentum != 0.f) {
    const float b = momentum * buf + q;
    buf = b;
    w = w - lr * b;
  } else {
    w = w - lr * q;
  }
}

__global__ void rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq,
                               float* __restrict__ buf, int64_t n, float lr, float alpha, float eps, float wd, float momentum,
                               int vec) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  int64_t done = 0;
  if (vec) {
    const int64_t n4 = n >> 2;
    for (int64_t i = tid; i < n4; i += nth) {
      float4 w = ((float4*)p)[i];
      const float4 gg = ((const float4*)g)[i];
      float4 s = ((float4*)sq)[i];
      float4 b = momentum != 0.f ? ((float4*)buf)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      rmsprop_one(w.x, gg.x, s.x, b.x, lr, alpha, eps, wd, momentum);
      rmsprop_one(w.y, gg.y, s.y, b.y, lr, alpha, eps, wd, momentum);
      rmsprop_one(w.z, gg.z, s.z, b.z, lr, alpha, eps, wd, momentum);
      rmsprop_one(w.w, gg.w, s.w, b.w, lr, alpha, eps, wd, momentum);
      ((float4*)sq)[i] = s;
      if (momentum != 0.f) ((float4*)buf)[i] = b;
      ((float4*)p)[i] = w;
    }
    done = n4 << 2;
  }
  for (int64_t i = done + tid; i < n; i += nth) {
    float w = p[i], s = sq[i], b = momentum != 0.f ? buf[i] : 0.f;
    rmsprop_one(w, g[i], s, b, lr, alpha, eps, wd, momentum);
    sq[i] = s;
    if (momentum != 0.f) buf[i] = b;
    p[i] = w;
  }
}

// The reference's vendored RAdam.step (optim/radam.py:82-129, degenerated_to_sgd=True).  branch: 2 = rectified (N_sma >= 5,
// :113-122), 1 = the SGD-like form below the threshold (:123-129), 0 = moments only.  wd_lr = weight_decay * lr (decoupled decay,
// applied only in a branch that updates, :114-117 / :124-127); step_lr = step_size * lr.
__device__ __forceinline__ void radam_one(float& w, float g, float& m, float& v, float b1, float b2, float eps, float wd_lr,
                                          float step_lr, int branch) {
  const float vi = b2 * v + (1.f - b2) * g * g;
  const float mi = b1 * m + (1.f - b1) * g;
  v = vi;
  m = mi;
  if (branch == 0) return;
  float x = w;
  if (wd_lr != 0.f) x = x - wd_lr * x;
  if (branch == 2) x = x - step_lr * (mi / (sqrtf(vi) + eps));
  else x = x - step_lr * mi;
  w = x;
}

__global__ void radam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                             int64_t n, float b1, float b2, float eps, float wd_lr, float step_lr, int branch, int vec) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  int64_t done = 0;
  if (vec) {
    const int64_t n4 = n >> 2;
    for (int64_t i = tid; i < n4; i += nth) {
      float4 w = ((float4*)p)[i];
      const float4 gg = ((const float4*)g)[i];
      float4 mm = ((float4*)m)[i];
      float4 vv = ((float4*)v)[i];
      radam_one(w.x, gg.x, mm.x, vv.x, b1, b2, eps, wd_lr, step_lr, branch);
      radam_one(w.y, gg.y, mm.y, vv.y, b1, b2, eps, wd_lr, step_lr, branch);
      radam_one(w.z, gg.z, mm.z, vv.z, b1, b2, eps, wd_lr, step_lr, branch);
      radam_one(w.w, gg.w, mm.w, vv.w, b1, b2, eps, wd_lr, step_lr, branch);
      ((float4*)m)[i] = mm;
      ((float4*)v)[i] = vv;
      if (branch != 0) ((float4*)p)[i] = w;
    }
    done = n4 << 2;
  }
  for (int64_t i = done + tid; i < n; i += nth) {
    float w = p[i], mm = m[i], vv = v[i];
    radam_one(w, g[i], mm, vv, b1, b2, eps, wd_lr, step_lr, branch);
    m[i] = mm;
    v[i] = vv;
    if (branch != 0) p[i] = w;
  }
}

// the grid cap of head.hip's element-wise launches (same environment switch)
static int ewb(int64_t n) {
  static const int64_t cap = getenv("IEEE_HEAD_EW_BLOCKS") ? atoll(getenv("IEEE_HEAD_EW_BLOCKS")) : 2048;
  int64_t b = (n + 255) / 256;
  return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}

}  // namespace ieee

using namespace ieee;

extern "C" int ieee_rmsprop_step(float* params, const float* grads, float* square_avg, float* momentum_buf, int64_t n, float lr,
                                 float alpha, float eps, float weight_decay, float momentum, void* stream) {
  IEEE_REQUIRE(params && grads && square_avg && (momentum == 0.f || momentum_buf), "rmsprop_step: null pointer");
  IEEE_REQUIRE(n >= 0, "rmsprop_step: n = %ld", (long)n);
  if (n == 0) return IEEE_OK;
  const uintptr_t bits = (uintptr_t)params | (uintptr_t)grads | (uintptr_t)square_avg | (momentum != 0.f ? (uintptr_t)momentum_buf : 0);
  const int vec = (bits & 15) == 0 ? 1 : 0;
  rmsprop_kernel<<<ewb(vec ? (n + 3) / 4 : n), 256, 0, (hipStream_t)stream>>>(params, grads, square_avg, momentum_buf, n, lr,
                                                                              alpha, eps, weight_decay, momentum, vec);
  return launch_status("rmsprop_kernel");
}

extern "C" int ieee_radam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                               float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream) {
  IEEE_REQUIRE(params && grads && exp_avg && exp_avg_sq, "radam_step: null pointer");
  IEEE_REQUIRE(n >= 0, "radam_step: n = %ld", (long)n);
  IEEE_REQUIRE(step >= 1, "radam_step: step counts from 1");
  if (n == 0) return IEEE_OK;
  // radam.py:94-110 in double, as the reference's Python floats (its ten-slot buffer only caches these per step)
  const double b1 = beta1, b2 = beta2, t = (double)step;
  const double beta2_t = pow(b2, t);
  const double n_sma_max = 2.0 / (1.0 - b2) - 1.0;
  const double n_sma = n_sma_max - 2.0 * t * beta2_t / (1.0 - beta2_t);
  double step_size;
  int branch;
  if (n_sma >= 5.0) {
    step_size = sqrt((1.0 - beta2_t) * (n_sma - 4.0) / (n_sma_max - 4.0) * (n_sma - 2.0) / n_sma * n_sma_max / (n_sma_max - 2.0)) /
                (1.0 - pow(b1, t));
    branch = 2;
  } else {
    step_size = 1.0 / (1.0 - pow(b1, t));       // degenerated_to_sgd=True (:106-107)
    branch = 1;
  }
  const float wd_lr = (float)((double)weight_decay * (double)lr), step_lr = (float)(step_size * (double)lr);
  const uintptr_t bits = (uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq;
  const int vec = (bits & 15) == 0 ? 1 : 0;
  radam_kernel<<<ewb(vec ? (n + 3) / 4 : n), 256, 0, (hipStream_t)stream>>>(params, grads, exp_avg, exp_avg_sq, n, beta1, beta2,
                                                                            eps, wd_lr, step_lr, branch, vec);
  return launch_status("radam_kernel");
}
