// DBSCAN on the device (ieee_amd/cluster.py; the reference has no such step).  The neighbour relation
//   R(i, j)  iff  i == j  or  D[i][j] <= thr  or  D[j][i] <= thr        (fp32 compares; a NaN is never a neighbour)
// is built as two CSR structures over the N points and nothing of size N x N is allocated here:
//   A   the directed lists {j != i : D[i][j] <= thr}, columns ascending: cluster_eps_kernel over every [block, slab]
//       distance buffer, a count sweep and, after the caller's exclusive sum, a fill sweep;
//   X   the OR closure: for an edge i -> j of A that has no edge j -> i, list j of X gains i (cluster_mirror_kernel, a
//       binary search in the sorted list j of A; count, exclusive sum, fill).  Order inside a list of X is arbitrary.
// A point is core when 1 + |A_i| + |X_i| >= min_samples.  The clusters are the connected components of R on the core
// points: hook and shortcut in rounds (cluster_cc_round_kernel), one launch per round; a round reads the previous
// round's parent array only and lowers a copy of it with integer atomicMin, so the next array is a function of the
// previous one whatever the order of the workgroups.  Labels: the roots (f[u] == u, the smallest index of a component)
// are numbered in ascending order by the caller's exclusive sum; a border point takes the smallest number among the core
// entries of both of its lists.  Integer atomics only, and none decides more than a minimum or a slot in an unordered
// list: the same result on every call.
#include "rank_common.h"

namespace ieee {

constexpr int CL_CHUNK = 1024;   // columns a workgroup handles between two scans: one float4 per thread

// One 256-thread workgroup per buffer row.  The row is `row0 + blockIdx.x` of the whole problem, the buffer's column c
// is point col0 + c.  Thread t of a chunk owns four consecutive columns, so the exclusive scan of the per-thread hit
// counts puts a chunk's hits in ascending column order; chunks, and the slabs of successive launches, follow each
// other through cursor[row].  A row belongs to one workgroup per launch and launches are stream-ordered: deg[row] and
// cursor[row] are read and written without atomics.  VEC: 16-byte loads (the caller has checked pointer and stride);
// the ragged end of a row, and every row of an unaligned buffer, goes through the scalar form.
template <bool FILL, bool VEC>
__global__ __launch_bounds__(256) void cluster_eps_kernel(const float* __restrict__ dist, int64_t ldd, int64_t cols,
                                                          int64_t row0, int64_t col0, float thr,
                                                          int64_t* __restrict__ deg, const int64_t* __restrict__ rowptr,
                                                          int32_t* __restrict__ cursor, int32_t* __restrict__ col,
                                                          int64_t cap) {
  __shared__ uint32_t wsum[4];
  const int t = threadIdx.x;
  const int64_t row = row0 + blockIdx.x;
  const float* __restrict__ drow = dist + (int64_t)blockIdx.x * ldd;
  const int64_t self = row - col0;                 // the buffer column of the point itself (maybe outside the slab)
  uint32_t count = 0;                              // COUNT: this thread's hits;  FILL: the row's hits so far
  int64_t base = 0, end = 0;
  if (FILL) {
    base = rowptr[row] + cursor[row];
    end = min(rowptr[row + 1], cap);
  }
  for (int64_t chunk = 0; chunk < cols; chunk += CL_CHUNK) {   // 64-bit: cols may come within a pass of 2^31
    const int64_t c = chunk + 4 * t;
    float v[4];
    bool hit[4] = {false, false, false, false};
    if (c < cols) {
      if (VEC && c + 3 < cols) {
        const float4 q = *(const float4*)(drow + c);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = c + e < cols ? drow[c + e] : __builtin_nanf("");
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) hit[e] = v[e] <= thr && c + e != self;
    }
    const uint32_t mine = (uint32_t)hit[0] + hit[1] + hit[2] + hit[3];
    if (!FILL) {
      count += mine;
      continue;
    }
    if (!__syncthreads_or((int)mine)) continue;    // the same answer in every thread: most chunks hold no neighbour
    uint32_t total;
    int64_t pos = base + count + block_scan_excl(mine, wsum, &total);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (hit[e]) {
        if (pos < end) col[pos] = (int32_t)(col0 + c + e);
        ++pos;
      }
    count += total;
  }
  if (FILL) {
    if (t == 0) cursor[row] += (int32_t)count;
    return;
  }
  uint32_t total;
  block_scan_excl(count, wsum, &total);
  if (t == 0) deg[row] += total;
}

// One wave per point i: for every edge i -> j of A, is i in the sorted list j of A?  Where it is not, list j of X
// gains i.  COUNT adds to cnt[j]; FILL draws the slot from cursor[j] (gs_tcount_kernel / gs_tfill_kernel's scheme).
template <bool FILL>
__global__ __launch_bounds__(256) void cluster_mirror_kernel(const int64_t* __restrict__ rowptr,
                                                             const int32_t* __restrict__ col, int N,
                                                             int64_t* __restrict__ cnt, const int64_t* __restrict__ xptr,
                                                             int32_t* __restrict__ cursor, int32_t* __restrict__ xcol,
                                                             int64_t cap) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  for (int64_t p = rowptr[i] + (threadIdx.x & 63); p < rowptr[i + 1]; p += 64) {
    const int j = min(max(col[p], 0), N - 1);
    int64_t lo = rowptr[j], hi = rowptr[j + 1];    // the first entry of list j that is >= i
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (col[mid] < (int32_t)i) lo = mid + 1; else hi = mid;
    }
    if (lo < rowptr[j + 1] && col[lo] == (int32_t)i) continue;
    if (!FILL) {
      atomicAdd((unsigned long long*)(cnt + j), 1ull);
    } else {
      const int64_t q = xptr[j] + atomicAdd(cursor + j, 1);
      if (q < min(xptr[j + 1], cap)) xcol[q] = (int32_t)i;
    }
  }
}

// core[u] = 1 + |A_u| + |X_u| >= min_samples;  the first parent array: every point its own root
__global__ void cluster_core_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ xptr, int N,
                                    int64_t min_samples, uint8_t* __restrict__ core, int32_t* __restrict__ f) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= N) return;
  core[u] = 1 + (rowptr[u + 1] - rowptr[u]) + (xptr[u + 1] - xptr[u]) >= min_samples ? 1 : 0;
  f[u] = (int32_t)u;
}

__device__ __forceinline__ int cl_parent(const int32_t* __restrict__ f, int v, int N) { return min(max(f[v], 0), N - 1); }

// One round, one wave per core point u.  fnext arrives as a copy of f.  Everything read for a decision comes from f, the
// previous round's array: g = f[f[v]] of every core neighbour v lowers fnext[f[u]] (hook on the parent) and fnext[u]
// (hook on the vertex); f[f[u]] lowers fnext[u] (shortcut).  What atomicMin returns is used for the flag alone, and the
// flag ends as 1 exactly when fnext differs from f.
__global__ __launch_bounds__(256) void cluster_cc_round_kernel(const int64_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ col,
                                                               const int64_t* __restrict__ xptr,
                                                               const int32_t* __restrict__ xcol,
                                                               const uint8_t* __restrict__ core, int N,
                                                               const int32_t* __restrict__ f, int32_t* __restrict__ fnext,
                                                               int32_t* __restrict__ changed) {
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= N || !core[u]) return;
  const int lane = threadIdx.x & 63;
  const int fu = cl_parent(f, (int)u, N);
  int best = cl_parent(f, fu, N);                  // the shortcut
  for (int side = 0; side < 2; ++side) {
    const int64_t* __restrict__ ptr = side ? xptr : rowptr;
    const int32_t* __restrict__ lst = side ? xcol : col;
    for (int64_t p = ptr[u] + lane; p < ptr[u + 1]; p += 64) {
      const int v = min(max(lst[p], 0), N - 1);
      if (!core[v]) continue;
      best = min(best, cl_parent(f, cl_parent(f, v, N), N));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
  if (lane != 0) return;
  bool lowered = false;
  if (best < fu) lowered = atomicMin(fnext + fu, best) > best;
  if (best < f[u]) lowered = (atomicMin(fnext + u, best) > best) || lowered;
  if (lowered) atomicOr(changed, 1);
}

// root[u] = 1 where u is core and its own parent: the smallest index of its component
__global__ void cluster_roots_kernel(const uint8_t* __restrict__ core, const int32_t* __restrict__ f, int N,
                                     int64_t* __restrict__ root) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= N) return;
  root[u] = core[u] && f[u] == (int32_t)u ? 1 : 0;
}

// One wave per point.  number[r] is the cluster number of root r (the exclusive sum of the root flags).  Core: the
// number of its root.  Otherwise the smallest number among the core entries of both lists, or -1.
__global__ __launch_bounds__(256) void cluster_labels_kernel(const int64_t* __restrict__ rowptr,
                                                             const int32_t* __restrict__ col,
                                                             const int64_t* __restrict__ xptr,
                                                             const int32_t* __restrict__ xcol,
                                                             const uint8_t* __restrict__ core,
                                                             const int32_t* __restrict__ f,
                                                             const int64_t* __restrict__ number, int N,
                                                             int64_t* __restrict__ labels) {
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= N) return;
  const int lane = threadIdx.x & 63;
  if (core[u]) {
    if (lane == 0) labels[u] = number[cl_parent(f, (int)u, N)];
    return;
  }
  int64_t best = INT64_MAX;
  for (int side = 0; side < 2; ++side) {
    const int64_t* __restrict__ ptr = side ? xptr : rowptr;
    const int32_t* __restrict__ lst = side ? xcol : col;
    for (int64_t p = ptr[u] + lane; p < ptr[u + 1]; p += 64) {
      const int v = min(max(lst[p], 0), N - 1);
      if (core[v]) best = min(best, number[cl_parent(f, v, N)]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t other = __shfl_xor(best, o);
    best = min(best, other);
  }
  if (lane == 0) labels[u] = best == INT64_MAX ? -1 : best;
}

static inline bool cl_aligned16(const void* p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

static int cl_check_buffer(const char* who, const float* dist, int64_t ldd, int64_t rows, int64_t cols, int64_t row0,
                           int64_t col0, int64_t N) {
  IEEE_REQUIRE(N >= 1 && N < (1ll << 31) - 1, "%s: N %ld out of range [1, 2^31 - 1)", who, (long)N);
  IEEE_REQUIRE(rows >= 0 && cols >= 0 && row0 >= 0 && col0 >= 0 && row0 + rows <= N && col0 + cols <= N,
               "%s: rows [%ld, +%ld) or columns [%ld, +%ld) outside the %ld points", who, (long)row0, (long)rows,
               (long)col0, (long)cols, (long)N);
  IEEE_REQUIRE(ldd >= cols, "%s: row stride %ld below the %ld columns", who, (long)ldd, (long)cols);
  IEEE_REQUIRE(rows == 0 || cols == 0 || dist, "%s: null pointer", who);
  return IEEE_OK;
}

}  // namespace ieee

using namespace ieee;

extern "C" int ieee_cluster_eps_count(const float* dist, int64_t ldd, int64_t rows, int64_t cols, int64_t row0,
                                      int64_t col0, int64_t N, float thr, int64_t* deg, void* stream) {
  IEEE_TRY(cl_check_buffer("cluster_eps_count", dist, ldd, rows, cols, row0, col0, N));
  if (rows == 0 || cols == 0) return IEEE_OK;
  IEEE_REQUIRE(deg, "cluster_eps_count: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (cl_aligned16(dist, ldd))
    cluster_eps_kernel<false, true><<<(unsigned)rows, 256, 0, st>>>(dist, ldd, cols, row0, col0, thr, deg, nullptr,
                                                                    nullptr, nullptr, 0);
  else
    cluster_eps_kernel<false, false><<<(unsigned)rows, 256, 0, st>>>(dist, ldd, cols, row0, col0, thr, deg, nullptr,
                                                                     nullptr, nullptr, 0);
  return launch_status("cluster_eps_count");
}

extern "C" int ieee_cluster_eps_fill(const float* dist, int64_t ldd, int64_t rows, int64_t cols, int64_t row0,
                                     int64_t col0, int64_t N, float thr, const int64_t* rowptr, int32_t* cursor,
                                     int32_t* col, int64_t cap, void* stream) {
  IEEE_TRY(cl_check_buffer("cluster_eps_fill", dist, ldd, rows, cols, row0, col0, N));
  IEEE_REQUIRE(cap >= 0, "cluster_eps_fill: cap %ld", (long)cap);
  if (rows == 0 || cols == 0) return IEEE_OK;
  IEEE_REQUIRE(rowptr && cursor && (col || cap == 0), "cluster_eps_fill: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (cl_aligned16(dist, ldd))
    cluster_eps_kernel<true, true><<<(unsigned)rows, 256, 0, st>>>(dist, ldd, cols, row0, col0, thr, nullptr, rowptr,
                                                                   cursor, col, cap);
  else
    cluster_eps_kernel<true, false><<<(unsigned)rows, 256, 0, st>>>(dist, ldd, cols, row0, col0, thr, nullptr, rowptr,
                                                                    cursor, col, cap);
  return launch_status("cluster_eps_fill");
}

#define CL_REQUIRE_N(who)                                                                                    \
  IEEE_REQUIRE(N >= 1 && N < (1ll << 31) - 1, who ": N %ld out of range [1, 2^31 - 1)", (long)N)

extern "C" int ieee_cluster_mirror_count(const int64_t* rowptr, const int32_t* col, int64_t N, int64_t* cnt, void* stream) {
  CL_REQUIRE_N("cluster_mirror_count");
  IEEE_REQUIRE(rowptr && cnt, "cluster_mirror_count: null pointer");
  cluster_mirror_kernel<false><<<(unsigned)((N + 3) / 4), 256, 0, (hipStream_t)stream>>>(rowptr, col, (int)N, cnt, nullptr,
                                                                                       nullptr, nullptr, 0);
  return launch_status("cluster_mirror_count");
}

extern "C" int ieee_cluster_mirror_fill(const int64_t* rowptr, const int32_t* col, int64_t N, const int64_t* xptr,
                                        int32_t* cursor, int32_t* xcol, int64_t cap, void* stream) {
  CL_REQUIRE_N("cluster_mirror_fill");
  IEEE_REQUIRE(cap >= 0, "cluster_mirror_fill: cap %ld", (long)cap);
  IEEE_REQUIRE(rowptr && xptr && cursor && (xcol || cap == 0), "cluster_mirror_fill: null pointer");
  cluster_mirror_kernel<true><<<(unsigned)((N + 3) / 4), 256, 0, (hipStream_t)stream>>>(rowptr, col, (int)N, nullptr, xptr,
                                                                                      cursor, xcol, cap);
  return launch_status("cluster_mirror_fill");
}

extern "C" int ieee_cluster_core(const int64_t* rowptr, const int64_t* xptr, int64_t N, int64_t min_samples, uint8_t* core,
                                 int32_t* f, void* stream) {
  CL_REQUIRE_N("cluster_core");
  IEEE_REQUIRE(min_samples >= 1, "cluster_core: min_samples %ld", (long)min_samples);
  IEEE_REQUIRE(rowptr && xptr && core && f, "cluster_core: null pointer");
  cluster_core_kernel<<<(unsigned)((N + 255) / 256), 256, 0, (hipStream_t)stream>>>(rowptr, xptr, (int)N, min_samples, core, f);
  return launch_status("cluster_core");
}

extern "C" int ieee_cluster_cc_round(const int64_t* rowptr, const int32_t* col, const int64_t* xptr, const int32_t* xcol,
                                     const uint8_t* core, int64_t N, const int32_t* f, int32_t* fnext, int32_t* changed,
                                     void* stream) {
  CL_REQUIRE_N("cluster_cc_round");
  IEEE_REQUIRE(rowptr && xptr && core && f && fnext && changed, "cluster_cc_round: null pointer");
  IEEE_REQUIRE(f != fnext, "cluster_cc_round: a round writes a second array");
  hipStream_t st = (hipStream_t)stream;
  IEEE_HIP(hipMemcpyAsync(fnext, f, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  IEEE_HIP(hipMemsetAsync(changed, 0, sizeof(int32_t), st));
  cluster_cc_round_kernel<<<(unsigned)((N + 3) / 4), 256, 0, st>>>(rowptr, col, xptr, xcol, core, (int)N, f, fnext, changed);
  return launch_status("cluster_cc_round");
}

extern "C" int ieee_cluster_roots(const uint8_t* core, const int32_t* f, int64_t N, int64_t* root, void* stream) {
  CL_REQUIRE_N("cluster_roots");
  IEEE_REQUIRE(core && f && root, "cluster_roots: null pointer");
  cluster_roots_kernel<<<(unsigned)((N + 255) / 256), 256, 0, (hipStream_t)stream>>>(core, f, (int)N, root);
  return launch_status("cluster_roots");
}

extern "C" int ieee_cluster_labels(const int64_t* rowptr, const int32_t* col, const int64_t* xptr, const int32_t* xcol,
                                   const uint8_t* core, const int32_t* f, const int64_t* number, int64_t N, int64_t* labels,
                                   void* stream) {
  CL_REQUIRE_N("cluster_labels");
  IEEE_REQUIRE(rowptr && xptr && core && f && number && labels, "cluster_labels: null pointer");
  cluster_labels_kernel<<<(unsigned)((N + 3) / 4), 256, 0, (hipStream_t)stream>>>(rowptr, col, xptr, xcol, core, f, number,
                                                                                (int)N, labels);
  return launch_status("cluster_labels");
}
