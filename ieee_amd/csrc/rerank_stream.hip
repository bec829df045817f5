// k-reciprocal re-ranking from descriptors: the algorithm, the float steps and the output bits of rerank_sparse.hip,
// with no Q x Q, G x G or (Q+G)^2 input either.  The virtual matrix orig = [[qq, qg], [qg^T, gg]] reaches these
// kernels block by block: the caller runs the distance GEMM (ieee_sqeuclid_distmat) on a strip of owner columns I and a
// slab of rows A, both on one side of Q, into one reused buffer, and hands the buffer to ieee_rerank_stream_block:
//   pass 0   A   colmax[I] |= max over A (unsigned max of the bits of the squares)
//   pass 1   B   the running K-lists of I (keys bits(D) << 32 | j) merged with the K smallest over A; colmax[I] must be
//                complete, so every strip is swept twice
// then ieee_rerank_stream_sets (rank from the lists; C1: the set logic, members ascending, and the position each had in
// E, which fixes the order of the weight sum), the caller's ieee_distmat_member_pairs (C2: Vv[i][pos] = orig[e][i] for
// the members e = Vi[i][pos], from the gathered-operand GEMM of evaluator.hip, each with the matrix's bits) and
// ieee_rerank_stream_rows (C3: weights, their sum in the dense kernel's association, the division; D: the query
// expansion).  Steps E and F go gallery range by gallery range
// (ieee_rerank_stream_range): an inverted index of the range's rows, then the Jaccard sums in ascending c and the combine
// with the range's Q x w distances.  Kernels shared with rerank_sparse.hip are templates on the view (rerank_sparse.h).
#include "rerank_sparse.h"

namespace ieee {

// C1: the set logic of rs_krecip_kernel without its distances.  Vi[i][pos] = the unique members ascending, Vp[i][pos] =
// the position p of the member's first occurrence in E: the dense kernel's lane p % 64 adds it, in ascending p.
__global__ __launch_bounds__(64) void rst_sets_kernel(const int* __restrict__ rank, int K, int Kh, int capV,
                                                      int* __restrict__ Vn, int* __restrict__ Vi, int* __restrict__ Vp) {
  __shared__ RsSets sets;
  const int i = blockIdx.x, t = threadIdx.x;
  const int ne = rs_krecip_sets(sets, rank, i, K, Kh);
  for (int p = t; p < ne; p += 64) {
    const int e = sets.E[p];
    bool first = true;
    for (int u = 0; u < p; ++u) first &= sets.E[u] != e;
    sets.F[p] = first;
    if (first) atomicAdd(&sets.nU, 1);
  }
  __syncthreads();
  for (int p = t; p < ne; p += 64) {
    if (!sets.F[p]) continue;
    const int e = sets.E[p];
    int pos = 0;
    for (int u = 0; u < ne; ++u) pos += sets.F[u] && sets.E[u] < e;
    if (pos < capV) {
      Vi[(int64_t)i * capV + pos] = e;
      Vp[(int64_t)i * capV + pos] = p;
    }
  }
  if (t == 0) Vn[i] = min(sets.nU, capV);
}

// C3: Vv[i][pos] holds orig[e][i] on entry and V[i][e] on exit.  Lane t adds the weights of positions p = t, t + 64, ...
// of E that are first occurrences, in ascending p, then the 64-lane tree: the sum rs_krecip_kernel forms.
__global__ __launch_bounds__(64) void rst_weights_kernel(const unsigned* __restrict__ colmax, const int* __restrict__ Vn,
                                                         const int* __restrict__ Vp, int capV, float* __restrict__ Vv) {
  __shared__ float W[RS_MAXE];
  __shared__ unsigned char F[RS_MAXE];
  __shared__ float wsum[64];
  const int i = blockIdx.x, t = threadIdx.x;
  for (int p = t; p < RS_MAXE; p += 64) F[p] = 0;
  __syncthreads();
  const int n = Vn[i];
  const float ci = __uint_as_float(colmax[i]);
  for (int pos = t; pos < n; pos += 64) {
    const int p = Vp[(int64_t)i * capV + pos];
    const float v = Vv[(int64_t)i * capV + pos];
    W[p] = expf(-(v * v / ci));
    F[p] = 1;
  }
  __syncthreads();
  float local = 0.f;
  for (int p = t; p < RS_MAXE; p += 64)
    if (F[p]) local += W[p];
  wsum[t] = local;
  __syncthreads();
  for (int s = 32; s > 0; s >>= 1) { if (t < s) wsum[t] += wsum[t + s]; __syncthreads(); }
  const float total = wsum[0];
  for (int pos = t; pos < n; pos += 64) {
    const int p = Vp[(int64_t)i * capV + pos];
    Vv[(int64_t)i * capV + pos] = 1.f * W[p] / total;
  }
}

// The sparse plan with the union region laid out for the streamed lives: B's running lists [N][K] and the chunk lists of
// one strip, C's positions [N][capV], D's scratch, and the inverted index of one gallery range.
struct RstPlan {
  RsPlan s;
  int64_t W, Wg, keys, parts, vp, total;
};

static bool rst_plan(int64_t Q, int64_t G, int64_t k1, int64_t k2, int64_t slab, RstPlan& p) {
  if (slab < 1 || !rs_plan(Q, G, k1, k2, p.s)) return false;
  RsPlan& s = p.s;
  p.W = std::min(slab, s.N);
  p.Wg = std::min(slab, G);
  const int64_t keys = align256(s.N * s.K * 8), parts = RS_MAXS * p.W * s.K * 8;
  const int64_t vp = s.N * s.capV * 4;
  const int64_t scr = k2 != 1 ? s.P * s.sstride * 4 : 0;
  const int64_t inv = align256(p.Wg * s.capUse * 4) * 2;
  p.keys = p.vp = s.uni;
  p.parts = s.uni + keys;
  s.invv = s.uni + align256(p.Wg * s.capUse * 4);
  p.total = s.uni + align256(std::max({keys + parts, vp, scr, inv})) + 256;
  return true;
}

// chunks of a block's rows, as rs_plan cuts the whole matrix: enough workgroups, at most RS_MAXS lists, >= 256 rows each
static void rst_chunks(int64_t rows, int64_t cols, int64_t& S, int64_t& per) {
  const int64_t strips = (cols + 63) / 64;
  S = std::max<int64_t>(1, std::min<int64_t>({(8192 + strips - 1) / strips, (int64_t)RS_MAXS, rows / 256}));
  per = (rows + S - 1) / S;
  S = (rows + per - 1) / per;
}

}  // namespace ieee

using namespace ieee;

#define RST_PLAN(who)                                                                                                   \
  RstPlan p;                                                                                                            \
  IEEE_REQUIRE(rst_plan(Q, G, k1, k2, slab, p), who ": arguments out of range (Q, G >= 1; 1 <= k1 <= %d, k1+1 <= Q+G "   \
               "< 2^31; 1 <= k2 <= k1+1; slab >= 1)", RS_MAXK - 1);                                                    \
  IEEE_REQUIRE(work, who ": null pointer");                                                                             \
  IEEE_REQUIRE(work_bytes >= p.total, who ": workspace too small (%ld < %ld bytes)", (long)work_bytes, (long)p.total); \
  hipStream_t st = (hipStream_t)stream;                                                                                 \
  char* w = (char*)work;                                                                                                \
  const int64_t N = p.s.N;                                                                                              \
  const int K = (int)p.s.K;                                                                                             \
  (void)st; (void)w; (void)N; (void)K

extern "C" int64_t ieee_rerank_stream_workspace_bytes(int64_t Q, int64_t G, int64_t k1, int64_t k2, int64_t slab) {
  RstPlan p;
  if (!rst_plan(Q, G, k1, k2, slab, p)) {
    set_error(IEEE_ERR_BAD_ARG, "rerank_stream: arguments out of range (Q, G >= 1; 1 <= k1 <= %d, k1+1 <= Q+G < 2^31; "
              "1 <= k2 <= k1+1; slab >= 1)", RS_MAXK - 1);
    return -1;
  }
  return p.total;
}

extern "C" int ieee_rerank_stream_layout(int64_t Q, int64_t G, int64_t k1, int64_t k2, int64_t slab, int64_t* fields) {
  RstPlan p;
  IEEE_REQUIRE(fields, "rerank_stream_layout: null pointer");
  IEEE_REQUIRE(rst_plan(Q, G, k1, k2, slab, p), "rerank_stream_layout: arguments out of range");
  const RsPlan& s = p.s;
  const int64_t v[] = {s.K, s.capV, s.capQ, s.rank, s.vn, s.vi, s.vv, s.qn, s.qi, s.qv, s.colmax, p.keys, p.W, p.Wg};
  for (int k = 0; k < 14; ++k) fields[k] = v[k];
  return IEEE_OK;
}

extern "C" int ieee_rerank_stream_begin(int64_t Q, int64_t G, int64_t k1, int64_t k2, int64_t slab, void* work,
                                        int64_t work_bytes, void* stream) {
  RST_PLAN("rerank_stream_begin");
  IEEE_HIP(hipMemsetAsync(w + p.s.colmax, 0, sizeof(unsigned) * (size_t)N, st));
  IEEE_HIP(hipMemsetAsync(w + p.keys, 0xff, sizeof(uint64_t) * (size_t)(N * K), st));
  return IEEE_OK;
}

extern "C" int ieee_rerank_stream_block(int64_t pass, const float* buf, int64_t sa, int64_t si, int64_t a0, int64_t a1,
                                        int64_t i0, int64_t i1, int64_t Q, int64_t G, int64_t k1, int64_t k2,
                                        int64_t slab, void* work, int64_t work_bytes, void* stream) {
  RST_PLAN("rerank_stream_block");
  IEEE_REQUIRE(buf, "rerank_stream_block: null pointer");
  IEEE_REQUIRE(pass == 0 || pass == 1, "rerank_stream_block: pass %ld (0 column maxima, 1 nearest lists)", (long)pass);
  IEEE_REQUIRE(0 <= a0 && a0 < a1 && a1 <= N && a1 - a0 <= slab && 0 <= i0 && i0 < i1 && i1 <= N && i1 - i0 <= p.W,
               "rerank_stream_block: rows [%ld, %ld), columns [%ld, %ld) of %ld, slab %ld", (long)a0, (long)a1, (long)i0,
               (long)i1, (long)N, (long)slab);
  IEEE_REQUIRE((sa == 1 && si >= a1 - a0) || (si == 1 && sa >= i1 - i0),
               "rerank_stream_block: strides (%ld, %ld): one is 1, the other at least the buffer's row length", (long)sa,
               (long)si);
  unsigned* colmax = (unsigned*)(w + p.s.colmax);
  RsBlockView o{buf, sa, si, (int)a0, (int)a1, (int)i0, (int)i1};
  const int64_t rows = a1 - a0, cols = i1 - i0;
  int64_t S, per;
  rst_chunks(rows, cols, S, per);
  const dim3 grid((unsigned)cdiv(cols, 64), (unsigned)S);
  if (pass == 0) {
    rs_colmax_kernel<<<grid, 64, 0, st>>>(o, (int)per, colmax);
    return launch_status("rs_colmax_kernel");
  }
  uint64_t* keys = (uint64_t*)(w + p.keys);
  uint64_t* parts = (uint64_t*)(w + p.parts);
  rs_select_kernel<RsBlockView, true><<<grid, 64, sizeof(uint64_t) * 64 * (K + 2 * RS_U), st>>>(o, colmax, (int)per, K,
                                                                                                 parts, keys);
  IEEE_TRY(launch_status("rs_select_kernel"));
  rs_merge_kernel<true><<<(unsigned)cols, 64, 0, st>>>(parts, (int)S, (int)cols, K, nullptr, keys, (int)i0);
  return launch_status("rs_merge_kernel");
}

extern "C" int ieee_rerank_stream_sets(int64_t Q, int64_t G, int64_t k1, int64_t k2, int64_t slab, void* work,
                                       int64_t work_bytes, void* stream) {
  RST_PLAN("rerank_stream_sets");
  int* rank = (int*)(w + p.s.rank);
  // the running lists are the one chunk list of every column; rank is written before Vp takes the lists' place
  rs_merge_kernel<false><<<(unsigned)N, 64, 0, st>>>((const uint64_t*)(w + p.keys), 1, (int)N, K, rank, nullptr, 0);
  IEEE_TRY(launch_status("rs_merge_kernel"));
  rst_sets_kernel<<<(unsigned)N, 64, 0, st>>>(rank, K, (int)p.s.Kh, (int)p.s.capV, (int*)(w + p.s.vn), (int*)(w + p.s.vi),
                                              (int*)(w + p.vp));
  return launch_status("rst_sets_kernel");
}

extern "C" int ieee_rerank_stream_rows(int64_t Q, int64_t G, int64_t k1, int64_t k2, int64_t slab, void* work,
                                       int64_t work_bytes, void* stream) {
  RST_PLAN("rerank_stream_rows");
  const RsPlan& s = p.s;
  int *Vn = (int*)(w + s.vn), *Vi = (int*)(w + s.vi);
  float* Vv = (float*)(w + s.vv);
  rst_weights_kernel<<<(unsigned)N, 64, 0, st>>>((const unsigned*)(w + s.colmax), Vn, (const int*)(w + p.vp), (int)s.capV, Vv);
  IEEE_TRY(launch_status("rst_weights_kernel"));
  if (k2 != 1) {
    float* scr = (float*)(w + s.scr);
    IEEE_HIP(hipMemsetAsync(scr, 0, sizeof(float) * (size_t)(s.P * s.sstride), st));
    rs_expand_kernel<<<(unsigned)s.P, 256, 0, st>>>((const int*)(w + s.rank), (int)N, K, (int)k2, Vn, Vi, Vv, (int)s.capV,
                                                     (int)s.capQ, scr, s.sstride, (int*)(w + s.qn), (int*)(w + s.qi),
                                                     (float*)(w + s.qv));
    IEEE_TRY(launch_status("rs_expand_kernel"));
  }
  return IEEE_OK;
}

extern "C" int ieee_rerank_stream_range(const float* dist, int64_t ldd, int64_t g0, int64_t g1, double lambda_value,
                                        float* out, int64_t ldo, int64_t Q, int64_t G, int64_t k1, int64_t k2,
                                        int64_t slab, void* work, int64_t work_bytes, void* stream) {
  RST_PLAN("rerank_stream_range");
  const RsPlan& s = p.s;
  IEEE_REQUIRE(dist && out, "rerank_stream_range: null pointer");
  IEEE_REQUIRE(0 <= g0 && g0 < g1 && g1 <= G && g1 - g0 <= p.Wg && ldd >= g1 - g0 && ldo >= g1 - g0,
               "rerank_stream_range: range [%ld, %ld) of %ld, slab %ld, ldd %ld, ldo %ld", (long)g0, (long)g1, (long)G,
               (long)slab, (long)ldd, (long)ldo);
  const int *n = (const int*)(w + (k2 != 1 ? s.qn : s.vn)), *idx = (const int*)(w + (k2 != 1 ? s.qi : s.vi));
  const float* val = (const float*)(w + (k2 != 1 ? s.qv : s.vv));
  int* cnt = (int*)(w + s.cnt);
  int64_t* off = (int64_t*)(w + s.off);
  int* inv_j = (int*)(w + s.invj);
  float* inv_v = (float*)(w + s.invv);
  const int wd = (int)(g1 - g0), j0 = (int)(Q + g0);
  IEEE_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)N, st));
  rs_inv_count_kernel<<<(unsigned)wd, 256, 0, st>>>(n, idx, (int)s.capUse, j0, cnt);
  IEEE_TRY(launch_status("rs_inv_count_kernel"));
  rs_scan_kernel<<<1, 1024, 0, st>>>(cnt, (int)N, off);
  IEEE_TRY(launch_status("rs_scan_kernel"));
  rs_inv_fill_kernel<<<(unsigned)wd, 256, 0, st>>>(n, idx, val, (int)s.capUse, j0, off, cnt, inv_j, inv_v);
  IEEE_TRY(launch_status("rs_inv_fill_kernel"));
  RsRangeView o{dist, ldd, ldo, j0, wd};
  rs_jaccard_kernel<<<(unsigned)Q, 256, 0, st>>>(o, (const unsigned*)(w + s.colmax), n, idx, val, (int)s.capUse, off, inv_j,
                                                  inv_v, (float)(1.0 - lambda_value), (float)lambda_value, out);
  return launch_status("rs_jaccard_kernel");
}
