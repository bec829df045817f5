// k-reciprocal re-ranking without N x N work matrices (N = Q + G): the same algorithm and the same bits as the dense
// ieee_rerank (rerank.hip), for galleries the dense form cannot hold.  Steps, on the virtual all-pairs matrix
// orig = [[qq, qg], [qg^T, gg]] (never formed); row i of the reference's normalised matrix is column i of orig:
//   A  colmax[i] = max_a orig[a][i]^2                                  one streaming pass (column strips x row chunks)
//   B  rank[i][0..K) = the K = k1+1 smallest (D[i][j], j), D[i][j] = fl(orig[j][i]^2) / colmax[i]
//                                                                      second streaming pass + a merge of the chunks
//   C  V[i] = exp(-D[i][e]) / sum over the expanded k-reciprocal set     sparse rows (ascending column, value)
//   D  Vq[i] = (sum_t V[rank[i][t]]) / k2, t < k2                        sparse rows, t order, one division
//   E  inverted index of the gallery rows of Vq (V when k2 = 1)        count, scan, fill
//   F  out[i][g] = (1 - t/(2-t))(1-lambda) + D[i][Q+g] lambda, t = sum_c min(Vq[i][c], Vq[Q+g][c]), c ascending
// Every float step is the dense kernel's, in its order: the terms the dense path adds and this one skips are zeros.
#include "rerank_sparse.h"

using namespace ieee;

extern "C" int64_t ieee_rerank_sparse_workspace_bytes(int64_t Q, int64_t G, int64_t k1, int64_t k2) {
  RsPlan p;
  if (!rs_plan(Q, G, k1, k2, p)) {
    set_error(IEEE_ERR_BAD_ARG, "rerank_sparse: arguments out of range (Q, G >= 1; 1 <= k1 <= %d, k1+1 <= Q+G < 2^31; "
              "1 <= k2 <= k1+1)", RS_MAXK - 1);
    return -1;
  }
  return p.total;
}

extern "C" int ieee_rerank_sparse_layout(int64_t Q, int64_t G, int64_t k1, int64_t k2, int64_t* fields) {
  RsPlan p;
  IEEE_REQUIRE(fields, "rerank_sparse_layout: null pointer");
  IEEE_REQUIRE(rs_plan(Q, G, k1, k2, p), "rerank_sparse_layout: arguments out of range");
  const int64_t v[] = {p.K, p.capV, p.capQ, p.rank, p.vn, p.vi, p.vv, p.qn, p.qi, p.qv, p.colmax};
  for (int k = 0; k < 11; ++k) fields[k] = v[k];
  return IEEE_OK;
}

extern "C" int ieee_rerank_sparse(const float* q_g_dist, const float* q_q_dist, const float* g_g_dist, int64_t Q,
                                  int64_t G, int64_t k1, int64_t k2, double lambda_value, float* out, void* work,
                                  int64_t work_bytes, void* stream) {
  IEEE_REQUIRE(q_g_dist && q_q_dist && g_g_dist && out && work, "rerank_sparse: null pointer");
  IEEE_REQUIRE(Q > 0 && G > 0, "rerank_sparse: empty query or gallery set");
  const int64_t N = Q + G;
  IEEE_REQUIRE(N < ((int64_t)1 << 31), "rerank_sparse: Q+G = %ld must stay below 2^31", (long)N);
  IEEE_REQUIRE(k1 >= 1 && k1 + 1 <= RS_MAXK && k1 + 1 <= N, "rerank_sparse: k1 %ld out of range (1..%d, < Q+G)",
               (long)k1, RS_MAXK - 1);
  IEEE_REQUIRE(k2 >= 1 && k2 <= k1 + 1, "rerank_sparse: k2 %ld out of range (1..k1+1)", (long)k2);
  RsPlan p;
  rs_plan(Q, G, k1, k2, p);
  IEEE_REQUIRE(work_bytes >= p.total, "rerank_sparse: workspace too small (%ld < %ld bytes)", (long)work_bytes,
               (long)p.total);
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)work;
  unsigned* colmax = (unsigned*)(w + p.colmax);
  int* rank = (int*)(w + p.rank);
  int *Vn = (int*)(w + p.vn), *Vi = (int*)(w + p.vi);
  float* Vv = (float*)(w + p.vv);
  int *Qn = (int*)(w + p.qn), *Qi = (int*)(w + p.qi);
  float* Qv = (float*)(w + p.qv);
  int* cnt = (int*)(w + p.cnt);
  int64_t* off = (int64_t*)(w + p.off);
  const int K = (int)p.K;
  RsView o{q_g_dist, q_q_dist, g_g_dist, (int)Q, (int)G};
  const dim3 strips((unsigned)cdiv(N, 64), (unsigned)p.S);

  IEEE_HIP(hipMemsetAsync(colmax, 0, sizeof(unsigned) * (size_t)N, st));
  rs_colmax_kernel<<<strips, 64, 0, st>>>(o, (int)p.rows, colmax);
  IEEE_TRY(launch_status("rs_colmax_kernel"));
  uint64_t* part = (uint64_t*)(w + p.part);
  rs_select_kernel<RsView, false><<<strips, 64, sizeof(uint64_t) * 64 * (K + 2 * RS_U), st>>>(o, colmax, (int)p.rows, K, part,
                                                                                          nullptr);
  IEEE_TRY(launch_status("rs_select_kernel"));
  rs_merge_kernel<false><<<(unsigned)N, 64, 0, st>>>(part, (int)p.S, (int)N, K, rank, nullptr, 0);
  IEEE_TRY(launch_status("rs_merge_kernel"));
  rs_krecip_kernel<<<(unsigned)N, 64, 0, st>>>(o, colmax, rank, (int)N, K, (int)p.Kh, (int)p.capV, Vn, Vi, Vv);
  IEEE_TRY(launch_status("rs_krecip_kernel"));
  const int *n = Vn, *idx = Vi;
  const float* val = Vv;
  if (k2 != 1) {
    float* scr = (float*)(w + p.scr);
    IEEE_HIP(hipMemsetAsync(scr, 0, sizeof(float) * (size_t)(p.P * p.sstride), st));
    rs_expand_kernel<<<(unsigned)p.P, 256, 0, st>>>(rank, (int)N, K, (int)k2, Vn, Vi, Vv, (int)p.capV, (int)p.capQ, scr,
                                                     p.sstride, Qn, Qi, Qv);
    IEEE_TRY(launch_status("rs_expand_kernel"));
    n = Qn; idx = Qi; val = Qv;
  }
  int* inv_j = (int*)(w + p.invj);
  float* inv_v = (float*)(w + p.invv);
  IEEE_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)N, st));
  rs_inv_count_kernel<<<(unsigned)G, 256, 0, st>>>(n, idx, (int)p.capUse, (int)Q, cnt);
  IEEE_TRY(launch_status("rs_inv_count_kernel"));
  rs_scan_kernel<<<1, 1024, 0, st>>>(cnt, (int)N, off);
  IEEE_TRY(launch_status("rs_scan_kernel"));
  rs_inv_fill_kernel<<<(unsigned)G, 256, 0, st>>>(n, idx, val, (int)p.capUse, (int)Q, off, cnt, inv_j, inv_v);
  IEEE_TRY(launch_status("rs_inv_fill_kernel"));
  rs_jaccard_kernel<<<(unsigned)Q, 256, 0, st>>>(o, colmax, n, idx, val, (int)p.capUse, off, inv_j, inv_v,
                                                  (float)(1.0 - lambda_value), (float)lambda_value, out);
  return launch_status("rs_jaccard_kernel");
}
