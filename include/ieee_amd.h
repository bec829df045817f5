/*
 * ieee_amd — C ABI of the MI355X (gfx950) implementation of the IEEE3modalPart
 * hot path (ziwang1121/IEEE).  This is the drop-in boundary: plain pointers and
 * sizes, no torch / C++ types.  Every entry point returns an int status
 * (IEEE_OK == 0, negative on error; text via ieee_last_error()), never throws,
 * never allocates or frees caller-visible memory, never synchronises the host
 * unless stated, and enqueues all work on the caller's hipStream_t (passed as
 * void*; NULL = default stream).  All data pointers are DEVICE pointers unless
 * a parameter is documented as host.
 *
 * The reference has no FFI of its own (it is pure PyTorch + one disabled Cython
 * module), so each entry point cites the reference Python function whose
 * arithmetic it replaces (file:line under the reference repo root).  The
 * ctypes binding a maintainer would add is shown in INTEGRATION.md and lives in
 * ieee_amd/_lib.py.
 *
 * Layouts: activations NHWC; modality-batched tensors carry a leading
 * modality axis of size 3 in the order [RGB, NI, TI]
 * (reference torchreid/data/datasets/dataset.py:338-340).
 */
#ifndef IEEE_AMD_H
#define IEEE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IEEE_OK 0
#define IEEE_ERR_BAD_ARG (-1)
#define IEEE_ERR_HIP (-2)
#define IEEE_ERR_UNSUPPORTED (-3)
#define IEEE_ERR_NO_VALID_QUERY (-4) /* rank.py:165 "all query identities do not appear in gallery" */

#define IEEE_F32 0
#define IEEE_BF16 1

#define IEEE_MAX_GROUPS 18 /* pointer-table capacity of the grouped head kernels (3 modalities x 6 parts) */

/* ---- library ---------------------------------------------------------- */
const char* ieee_last_error(void); /* thread-local text of the last failure */
int ieee_version(void);            /* ABI version, currently 1 */
/* 1 if the current HIP device is gfx950, 0 otherwise (host query) */
int ieee_device_is_gfx950(void);

/* ---- evaluator: distance matrix ---------------------------------------- */
/* torchreid/metrics/distance.py:49-64 euclidean_squared_distance:
 *   out[i][j] = |q_i|^2 + |g_j|^2 - 2 q_i.g_j      (squared, may be slightly < 0)
 * q [m][d], g [n][d] row-major, dtype IEEE_F32 (exact fp32 MFMA, k-ordered fma
 * chain) or IEEE_BF16 (inputs already bf16; fp32 accumulate).  out [m][n] fp32,
 * row stride ldo elements.  d % 8 == 0.  work: >= (m+n)*4 bytes of scratch
 * (row norms).  metric: 0 euclidean, 1 cosine (distance.py:67-80: rows are
 * L2-normalised with eps 1e-12 and out = 1 - q^.g^), 2 negated inner product
 * (out = -q_i.g_j, no norms: what ieee_gnn_rerank ranks). */
int ieee_sqeuclid_distmat(const void* q, const void* g, int64_t m, int64_t n, int64_t d, int dtype,
                          int metric, float* out, int64_t ldo, void* work, void* stream);
/* Single elements of that matrix (dtype IEEE_F32), each with the bits ieee_sqeuclid_distmat gives it: out[p] = the
 * element (idx1[p], idx2[p]) of the matrix of x1 [m][d] (rows) and x2 [n][d] (columns), p < pairs.  A gathered-operand
 * GEMM: sixteen pairs per wave go through the same v_mfma_f32_16x16x4_f32 sequence as the matrix's tiles (the same k
 * to the same lane group, ascending, one accumulator per element), with the same row norms and the same epilogue.
 * idx1, idx2: int32 on the device, every index inside its operand (not checked: they are device data).  work: >=
 * (m+n)*4 bytes.
 * ieee_distmat_member_pairs: the same for the members of owner rows of the all-pairs matrix orig = [[qq, qg], [qg^T,
 * gg]] over x = [queries; gallery] [rows][d], split = the number of queries: out[i][p] = orig[e][i], e = members[i][p],
 * p < counts[i] (members, out: [rows][cap]).  Every element has the row operand the matrix path gives it: e, but the
 * query where e is a gallery row and i a query.  metric 0 or 1.  work: >= rows*4 bytes. */
int ieee_distmat_pairs(const float* x1, const float* x2, int64_t m, int64_t n, int64_t d, const int32_t* idx1,
                       const int32_t* idx2, int64_t pairs, int metric, float* out, void* work, void* stream);
int ieee_distmat_member_pairs(const float* x, int64_t rows, int64_t d, int64_t split, const int32_t* counts,
                              const int32_t* members, int64_t cap, int metric, float* out, void* work, void* stream);
/* the same matrix from fp32 rows on the 16-bit matrix cores: every value is split into 16-bit pieces that sum to it
 * and q.g becomes ONE 16-bit GEMM over the piece products, smallest first, accumulated in fp32 (each product is exact
 * there).  scheme:
 *   IEEE_SPLIT_BF16X3  three bf16 pieces (all 24 mantissa bits), six products hi.hi hi.mid mid.hi mid.mid hi.lo lo.hi;
 *                      what is dropped is below 2^-24 of the result
 *   IEEE_SPLIT_F16X2   two fp16 pieces (22 bits) of the row scaled by a power of two (undone in the epilogue), three
 *                      products hi.hi hi.lo lo.hi: 2^-22, half the matrix work of BF16X3
 *   IEEE_SPLIT_BF16X2  two bf16 pieces, three products: ~2^-16
 * Row norms come from the fp32 rows as above.  work: ieee_sqeuclid_distmat_split_workspace_bytes() bytes. */
#define IEEE_SPLIT_BF16X3 6
#define IEEE_SPLIT_BF16X2 3
#define IEEE_SPLIT_F16X2 2
int64_t ieee_sqeuclid_distmat_split_workspace_bytes(int64_t m, int64_t n, int64_t d, int64_t scheme);
int ieee_sqeuclid_distmat_split(const float* q, const float* g, int64_t m, int64_t n, int64_t d, int64_t scheme,
                                int metric, float* out, int64_t ldo, void* work, int64_t work_bytes, void* stream);

/* ---- evaluator: CMC / mAP ----------------------------------------------- */
/* torchreid/metrics/rank.py:103-171 eval_market1501 (and the disabled native
 * rank_cylib/rank_cy.pyx:156-243).  distmat [num_q][num_g] fp32 (row stride
 * ldd), pids / camids int32 device arrays.  Tie order is (distance, gallery
 * index) ascending.  Outputs (device):
 *   ap        [num_q] float64   average precision per query (-1 when skipped)
 *   first_pos [num_q] int32     0-based rank of the first true match among kept
 *   summary   [max_rank+2] int64: cmc hit counts per rank, then num_valid_q,
 *             then (bit pattern of) the float64 sum of AP over valid queries
 * The host shim forms cmc = float32(counts)/float32(num_valid) and
 * mAP = ap_sum/num_valid as rank.py:167-169 does.  No host sync inside. */
int ieee_rank_market1501(const float* distmat, int64_t ldd, int64_t num_q, int64_t num_g,
                         const int32_t* q_pids, const int32_t* g_pids, const int32_t* q_camids,
                         const int32_t* g_camids, int64_t max_rank, double* ap, int32_t* first_pos,
                         int64_t* summary, void* stream);
/* The same evaluation with a workspace of ieee_rank_workspace_bytes(num_g) bytes (device, 4-byte aligned): the gallery is
 * bucketed by identity once per call, so a query collects its true matches and its same-camera entries from one bucket
 * instead of scanning all num_g identities.  Same results, bit for bit. */
int64_t ieee_rank_workspace_bytes(int64_t num_g);
int ieee_rank_market1501_ws(const float* distmat, int64_t ldd, int64_t num_q, int64_t num_g,
                            const int32_t* q_pids, const int32_t* g_pids, const int32_t* q_camids,
                            const int32_t* g_camids, int64_t max_rank, double* ap, int32_t* first_pos,
                            int64_t* summary, void* work, int64_t work_bytes, void* stream);
/* Ranked retrieval: the k nearest gallery entries of every query, what torchreid/utils/reidtools.py:49 gets from
 * np.argsort(distmat, axis=1) on the host.  distmat [num_q][num_g] fp32 (row stride ldd >= num_g) on the device.
 * With exclude_same_cam != 0 the four int32 label arrays are read and an entry with the query's identity AND camera is
 * skipped (reidtools.py:110-112, rank.py:136-137); otherwise they may be null.  Outputs, [num_q][k] row-major:
 * out_idx int32 gallery indices and out_dist fp32 distances, ascending in (distance, gallery index) -- a stable
 * argsort of the kept row, -0.0 equal to +0.0, NaN after +inf.  A row with fewer than k kept entries is padded with
 * idx -1 and dist +inf.  1 <= k <= 1024, else IEEE_ERR_BAD_ARG before any launch.  No workspace, no host sync. */
int ieee_rank_topk(const float* distmat, int64_t ldd, int64_t num_q, int64_t num_g,
                   const int32_t* q_pids, const int32_t* g_pids, const int32_t* q_camids,
                   const int32_t* g_camids, int exclude_same_cam, int64_t k, int32_t* out_idx,
                   float* out_dist, void* stream);
/* ieee_rank_topk continued from a previous result: gallery search without the whole [num_q][num_g] matrix.
 * slab [num_q][slab_g] fp32 (row stride ldd >= slab_g) holds the distances to gallery entries g_base ... g_base +
 * slab_g - 1; slab_g_pids / slab_g_camids are the labels of those entries only (indexed by the slab's column).
 * state_idx int32 / state_dist fp32, [num_q][k] row-major, hold the list so far and are updated in place: each row
 * ascending in (distance, GLOBAL gallery index), unused places idx -1 / dist +inf at the end.  A search starts from a
 * state filled with -1 / +inf.  Precondition (not checked): every index in the state is < g_base.  After the slabs of
 * any partition of a matrix's columns have been merged in ascending g_base order the state equals ieee_rank_topk's
 * result for the whole matrix bit for bit: ties go to the smaller global index, and a distance that entered the list
 * slabs ago comes back with its own bits (-0.0, NaN payloads).  1 <= k <= 1024, g_base >= 0 and
 * g_base + slab_g < 2^31 - 6144, else IEEE_ERR_BAD_ARG before any launch; num_q == 0 or slab_g == 0 is a no-op.
 * No workspace, no host sync, no atomics on global memory: the same bits on every call. */
int ieee_rank_topk_merge(const float* slab, int64_t ldd, int64_t num_q, int64_t slab_g, int64_t g_base,
                         const int32_t* q_pids, const int32_t* slab_g_pids, const int32_t* q_camids,
                         const int32_t* slab_g_camids, int exclude_same_cam, int64_t k, int32_t* state_idx,
                         float* state_dist, void* stream);
/* ieee_rank_market1501 without the whole [num_q][num_g] matrix: the gallery's distances arrive in column slabs, in two
 * passes, and the result is the whole-matrix call's -- CMC counts, num_valid_q and every first_pos equal; the AP of a
 * query with at most 1024 true matches and at most 1024 removed entries equal as bits (and so the AP sum, when every
 * query is of that kind); the AP of a larger query within nb * 2^-52 (nb true matches: the same nb terms in another
 * association).  Order: the raw IEEE order of the distances, ties to the smaller GLOBAL gallery index.
 * The plan comes from the host, which has all four label arrays, as two CSR lists over the queries (device arrays):
 *   m_off / r_off  int64 [num_q + 1]  segment starts; m_off[num_q] = total_match_keys, r_off[num_q] = total_removed_keys
 *   m_idx / r_idx  int32 [total]      GLOBAL gallery indices of the query's true matches (same identity, other camera)
 *                                     and of its removed entries (same identity, same camera), each once
 *   m_pos / r_pos  int32 [total]      the place of that gallery index in match_columns, the ascending list of the
 *                                     gallery indices that occur in either list
 * state: ieee_rank_stream_workspace_bytes(num_q, total_match_keys, total_removed_keys) bytes (device, 8-byte aligned),
 * the same three numbers in every call: the keys of both lists (uint64), a running count per match key (uint32), ap
 * and first.  -1 for a negative argument.  The calls of one evaluation, all on one stream:
 *   collect  slab [num_q][slab_cols] fp32 (row stride ldd >= slab_cols) holds the distances to the gallery entries
 *            match_columns[col_base ... col_base + slab_cols - 1].  Writes the (distance, global index) key of every
 *            planned entry whose place falls into the slab.  Every place is collected exactly once, in any order.
 *   seal     after the last collect: sorts every query's match keys and removed keys ascending, clears the counts.
 *   count    slab [num_q][slab_g] fp32 (row stride ldd >= slab_g) holds the distances to gallery entries g_base ...
 *            g_base + slab_g - 1, ALL of them, not only match_columns.  Adds, for every match key, the slab's entries
 *            with key <= it.  Every gallery column is counted exactly once, in any order (counts add; not checked).
 *            It reads no labels: removed entries are counted like any entry and leave through their sorted keys -- for a
 *            query within both 1024 limits here, from the slots they were counted in (what the whole-matrix kernel does
 *            for such a query), for a larger query in finish.
 *   finish   after the last count: rank_i = count_i - 1 - #{removed keys < match key i}, AP and first per query in
 *            ieee_rank_market1501's association, then its summary kernel.  ap [num_q] float64 / first_pos [num_q]
 *            int32 (device) may be null: the state's own arrays are used.  summary [max_rank + 2] int64 as
 *            ieee_rank_market1501's; max_rank is NOT clamped to the gallery's size here (the caller does that).
 *            May be called again (it changes no keys or counts).
 * 0 <= col_base, col_base + slab_cols < 2^31; 0 <= g_base, g_base + slab_g < 2^31; 1 <= max_rank <= 1024; a state that
 * is null, misaligned or too small: IEEE_ERR_BAD_ARG before any launch.  num_q == 0, slab_cols == 0 or slab_g == 0 is a
 * no-op (finish with num_q == 0 writes a zero summary).  No host sync, no atomics on global memory, no floating-point
 * atomics: the same bits on every call. */
int64_t ieee_rank_stream_workspace_bytes(int64_t num_q, int64_t total_match_keys, int64_t total_removed_keys);
int ieee_rank_stream_collect(const float* slab, int64_t ldd, int64_t num_q, int64_t slab_cols, int64_t col_base,
                             const int64_t* m_off, const int32_t* m_pos, const int32_t* m_idx,
                             const int64_t* r_off, const int32_t* r_pos, const int32_t* r_idx,
                             int64_t total_match_keys, int64_t total_removed_keys, void* state,
                             int64_t state_bytes, void* stream);
int ieee_rank_stream_seal(int64_t num_q, const int64_t* m_off, const int64_t* r_off, int64_t total_match_keys,
                          int64_t total_removed_keys, void* state, int64_t state_bytes, void* stream);
int ieee_rank_stream_count(const float* slab, int64_t ldd, int64_t num_q, int64_t slab_g, int64_t g_base,
                           const int64_t* m_off, const int64_t* r_off, int64_t total_match_keys,
                           int64_t total_removed_keys, void* state, int64_t state_bytes, void* stream);
int ieee_rank_stream_finish(int64_t num_q, const int64_t* m_off, const int64_t* r_off, int64_t total_match_keys,
                            int64_t total_removed_keys, void* state, int64_t state_bytes, int64_t max_rank,
                            double* ap, int32_t* first_pos, int64_t* summary, void* stream);
/* CUHK03 single-gallery-shot protocol, torchreid/metrics/rank.py:24-100 (eval_cuhk03 with the time-id filter): the
 * EXPECTED curve of the protocol's random draw (one gallery image per identity, uniformly), not a 10-sample estimate
 * of it.  distmat [num_q][num_g] fp32 (row stride ldd >= num_g); q_pids / g_pids int32; q_keys / g_keys int32, one
 * word per (camera, time id) pair, equal pairs equal words on both sides.  Per query the gallery is ordered on
 * (distance, gallery index), -0.0 equal to +0.0, NaN after +inf; entries with the query's identity AND key are dropped;
 * a query without a kept true match is skipped.  With T the kept true matches and, for every other identity j of n_j
 * images, c_j(t) of them before true match t:
 *   cmc[r] = (1 / |T|) sum_t P(sum_j B_j(t) <= r),  B_j(t) ~ Bernoulli(c_j(t) / n_j) independent,
 * by the recurrence pmf'[k] = pmf[k](1 - p) + pmf[k-1] p over the identities in ascending-pid order, in float64.
 * A query that sees fewer than max_rank identities has 1.0 in the tail of its curve.  Outputs (device):
 *   cmc     [num_q][max_rank] float64   the per-query curve (zeros when skipped)
 *   ap      [num_q] float64             average precision of the kept list (-1 when skipped)
 *   summary [max_rank+2] float64        the curves summed over the valid queries, num_valid_q, the AP sum
 * The host shim forms cmc = float32(sum / num_valid) and mAP = ap_sum / num_valid.  Every sum has one fixed order and
 * there are no floating-point atomics: two calls give the same bits.  work: ieee_rank_cuhk03_workspace_bytes(num_g)
 * bytes (device, 4-byte aligned), the gallery grouped by identity.  1 <= max_rank <= 1024 (not clamped to num_g),
 * ldd >= num_g and a large enough workspace, else IEEE_ERR_BAD_ARG before any launch.  No host sync inside. */
int64_t ieee_rank_cuhk03_workspace_bytes(int64_t num_g);
int ieee_rank_cuhk03(const float* distmat, int64_t ldd, int64_t num_q, int64_t num_g,
                     const int32_t* q_pids, const int32_t* g_pids, const int32_t* q_keys,
                     const int32_t* g_keys, int64_t max_rank, double* cmc, double* ap, double* summary,
                     void* work, int64_t work_bytes, void* stream);

/* ---- activation maps (tools/visualize_actmap.py) --------------------------- */
/* tools/visualize_actmap.py:84-88: outputs = (outputs**2).sum(1); F.normalize(outputs.view(b, h*w), p=2, dim=1).
 * x [N][P][C], NHWC (P = h*w positions, C channels innermost), IEEE_F32 or IEEE_BF16, 16-byte aligned; out fp32 [N][P]:
 *   E[n][p] = sum_c x[n][p][c]^2 in fp32,   out[n][p] = E[n][p] / max(||E[n][:]||_2, 1e-12)
 * (F.normalize's eps: an all-zero map gives zeros, not NaN).  One workgroup per image; the order of every sum is fixed
 * (lane, shuffle butterfly, LDS in wave order) and there are no atomics, so two calls give the same bits.
 * C % 8 == 0 and 1 <= P <= 4096, else IEEE_ERR_BAD_ARG before any launch.  No workspace, no host sync. */
int ieee_actmap_energy(const void* x, int dtype, int64_t N, int64_t P, int64_t C, float* out, void* stream);
/* tools/visualize_actmap.py:119-146: the three-panel figure of every image of a batch, finished bytes only.
 * amap fp32 [N][h][w] (h*w <= 4096).  img: the normalised network input, fp32 NCHW [N][3][height][width], or NULL -- then
 * only index_out is written.  mean3 / std3: HOST pointers to three floats (read during the call; :119-120).  lut: uint8
 * [256][3] RGB colour table on the device (:131 uses COLORMAP_JET).  grid_out uint8 [N][height][3*width + 20][3] RGB, left
 * to right the de-normalised image, the coloured map, the overlay, with two 10-pixel white gaps (:138-146; the reference
 * builds the figure in BGR for cv2.imwrite and adds the RGB image to the BGR map in its overlay, :134 -- here the overlay
 * adds like channels).  index_out uint8 [N][height][width]: the colour index before the table, or NULL.  Arithmetic,
 * fp32 without fused multiply-adds unless stated:
 *   resize (:126, cv2.resize INTER_LINEAR positions): sx = (dx + 0.5) * (w / width) - 0.5, x0 = floor(sx), fx = sx - x0;
 *     x0 < 0 -> x0 = 0, fx = 0; x0 >= w - 1 -> x0 = w - 1, fx = 0; x1 = min(x0 + 1, w - 1); the same in y; rows y0 and y1
 *     are interpolated horizontally, then the two results vertically, each step a + (b - a) * f
 *   index (:127-130): floor(255 * (v - min) / ((max - min) + 1e-12f)), min / max over the RESIZED map of the image
 *   image (:119-121): c = clamp(x * std + mean, 0, 1), byte = floor(c * 255)
 *   overlay (:134-136): trunc(min(0.3 * image + 0.7 * colour, 255)) in double
 * One workgroup per image, two passes over the figure (min / max, then the bytes); width <= 2048 (a figure row is
 * assembled on chip), else IEEE_ERR_BAD_ARG before any launch.  No workspace, no host sync. */
int ieee_actmap_render(const float* amap, int64_t h, int64_t w, const float* img, const float* mean3, const float* std3,
                       const uint8_t* lut, int64_t N, int64_t height, int64_t width, uint8_t* grid_out,
                       uint8_t* index_out, void* stream);

/* ---- convolution as implicit GEMM over NHWC (MFMA) ------------------------ */
/* These replace torch's conv2d forward / backward as dispatched by the
 * reference's Bottleneck.forward (torchreid/models/resnet.py:164-184), the
 * ResNetIEEE stem (:496-501, :622-631) and the CIM 1x1 convs
 * (torchreid/models/ieee3modalPart.py:28-48, 427-435).  `groups` independent
 * problems (the three modality streams) run in one launch; *_gs are the
 * per-group strides in ELEMENTS.  dtype IEEE_F32 (exact fp32 MFMA, parity
 * mode) or IEEE_BF16 (bf16 storage, fp32 accumulate).  Activations NHWC. */

/* row length (elements) of a packed weight matrix: R*S*inner rounded up to the k-tile */
int64_t ieee_conv_packed_ld(int dtype, int64_t inner_channels, int64_t R, int64_t S);

/* fp32 OIHW parameters (the reference's state_dict layout) -> GEMM operand.
 * mode 0: forward  dst[co][(r*S+s)*Ci+ci]; mode 1: dgrad dst[ci][(r*S+s)*Co+co] */
int ieee_pack_conv_weight(const float* w_oihw, void* dst, int dtype, int mode, int64_t groups, int64_t Co,
                          int64_t Ci, int64_t R, int64_t S, int64_t w_gs, int64_t dst_gs, void* stream);

/* same, zero-padding the input-channel, kernel-height and kernel-width axes to (Ci, R, S) >= (Ci_src, R_src, S_src);
 * and its inverse for the weight gradient (dw_padded [Co][Ci][R][S] -> dw [Co][Ci_src][R_src][S_src]) */
int ieee_pack_conv_weight_padded(const float* w_oihw, void* dst, int dtype, int mode, int64_t groups, int64_t Co,
                                 int64_t Ci_src, int64_t R_src, int64_t S_src, int64_t Ci, int64_t R, int64_t S,
                                 int64_t w_gs, int64_t dst_gs, void* stream);
int ieee_unpad_weight_grad(const float* dw_padded, float* dw, int64_t groups, int64_t Co, int64_t Ci, int64_t R,
                           int64_t S, int64_t Ci_src, int64_t R_src, int64_t S_src, int64_t dwp_gs, int64_t dw_gs,
                           int accumulate, void* stream);

/* every conv weight of the network in ONE launch: `descs` is a device array of packing descriptors built by
 * the executor (ieee_pack_desc_bytes() each); offsets are elements relative to `params` / `ws_base` */
int64_t ieee_pack_desc_bytes(void);
int ieee_pack_all_weights(const float* params, void* ws_base, const void* descs, int64_t ndesc,
                          int64_t total_blocks, int dtype, void* stream);

/* y[N,Ho,Wo,Co] = conv(x[N,Hi,Wi,Ci], w), no bias (every conv on the path is bias-free) */
int ieee_conv2d_fwd(const void* x, const void* w_packed, void* y, int dtype, int64_t groups, int64_t N,
                    int64_t Hi, int64_t Wi, int64_t Ci, int64_t Co, int64_t R, int64_t S, int64_t stride,
                    int64_t pad, int64_t x_gs, int64_t w_gs, int64_t y_gs, float* bn_partial, void* stream);
/* bn_partial (bf16 vector path only, else NULL): the conv also emits, per group, [2][Co][rblocks] per-channel
 * sum / sum-of-squares of the stored outputs, rblocks = ieee_conv2d_fwd_stats_rblocks(); hand the same buffer
 * and rblocks to ieee_bn2d_fwd(stats_rblocks) and the separate statistics pass disappears */
int64_t ieee_conv2d_fwd_stats_rblocks(int64_t N, int64_t Ho, int64_t Wo);
/* inference: conv + eval-mode BatchNorm (+ residual) (+ ReLU) in one launch -- Bottleneck.forward / the stem in eval
 * mode (resnet.py:164-184, 622-626).  bn_stats: that BN's [groups][4][Co] statistics as ieee_bn2d_fwd(training = 0,
 * out = NULL) leaves them (scale at 2*Co, shift at 3*Co); out = [relu](conv(x)*scale + shift [+ residual]). */
int ieee_conv2d_fwd_bn_eval(const void* x, const void* w_packed, void* out, const void* residual,
                            const float* bn_stats, int relu, int dtype, int64_t groups, int64_t N, int64_t Hi,
                            int64_t Wi, int64_t Ci, int64_t Co, int64_t R, int64_t S, int64_t stride, int64_t pad,
                            int64_t x_gs, int64_t w_gs, int64_t out_gs, void* stream);

/* dx[N,Hi,Wi,Ci] = conv_transpose(dy) (+ addend, same layout as dx, may be NULL): the
 * residual-branch gradient of Bottleneck (resnet.py:181 `out += identity`) is folded in here */
int ieee_conv2d_dgrad(const void* dy, const void* w_packed_d, void* dx, const void* addend, int dtype,
                      int64_t groups, int64_t N, int64_t Hi, int64_t Wi, int64_t Ci, int64_t Co, int64_t R,
                      int64_t S, int64_t stride, int64_t pad, int64_t dy_gs, int64_t w_gs, int64_t dx_gs,
                      float* bn_partial, const void* bn_y, const void* bn_mask, const float* bn_stats,
                      int bn_mask_bits, int addend_stride, void* stream);
/* The same dgrad with the sums of a SECOND BatchNorm that is fed by the same gradient (the downsample branch of the block whose
 * output this dgrad differentiates; torchreid/models/resnet.py:176-181): bn_y2 = that BatchNorm's input (shape and group stride of
 * bn_y), bn_partial2 = its own partial block of ieee_conv2d_fwd_stats_rblocks(N, Hi, Wi) * 2 * Ci floats per group, which
 * receives sum g and sum g*y2 -- its ieee_bn2d_bwd(stats_rblocks > 0) then needs no reduction pass either.  bf16 fused form only. */
int ieee_conv2d_dgrad2(const void* dy, const void* w_packed_d, void* dx, const void* addend, int dtype,
                      int64_t groups, int64_t N, int64_t Hi, int64_t Wi, int64_t Ci, int64_t Co, int64_t R,
                      int64_t S, int64_t stride, int64_t pad, int64_t dy_gs, int64_t w_gs, int64_t dx_gs,
                      float* bn_partial, const void* bn_y, const void* bn_mask, const float* bn_stats,
                      int bn_mask_bits, int addend_stride, const void* bn_y2,
                      float* bn_partial2, void* stream);
/* bn_partial != NULL (bf16 only): dx is the gradient w.r.t. the output of a BN(+ReLU) whose input is bn_y; the
 * dgrad epilogue also emits that BN's backward sums [2][Ci][rblocks] (sum g, sum g*y; g = dx * [mask], mask from
 * bn_mask > 0, or from bn_y*scale+shift > 0 with bn_stats = that BN's [4][Ci] stats, or none), rblocks =
 * ceil(N*Hi*Wi/128): pass it to ieee_bn2d_bwd(stats_rblocks) and the separate reduction pass disappears.
 * With bn_mask (the ReLU behind a residual add, resnet.py:181-182) dx is stored ALREADY MASKED, dx = g: the
 * BatchNorm backward that follows then takes out_mask = NULL and reads g and y only.  bn_mask_bits = 1: bn_mask is
 * the packed form ieee_bn2d_fwd(relu_bits) wrote (one byte per 8 channels, 1/16 of the bytes), else the activation.
 * addend_stride = 2 (with bn_partial, stride 1, power-of-two Hi / Wi): addend is [N, Hi/2, Wi/2, Ci] and belongs to the
 * pixels with even row and column -- what the stride-2 1x1 downsample branch of a block (resnet.py:548-556) sends back;
 * that branch's dgrad is then a dense 1x1 stride-1 dgrad over the (Ho, Wo) grid instead of a 3/4-zero full-size map */

/* dw (fp32, OIHW, the layout of param.grad) = or += sum over pixels; deterministic split-K:
 * partial slabs in `work` (size from the query below) are reduced in a fixed order */
int64_t ieee_conv2d_wgrad_workspace_bytes(int dtype, int64_t groups, int64_t N, int64_t Ho, int64_t Wo,
                                          int64_t Ci, int64_t Co, int64_t R, int64_t S);
int ieee_conv2d_wgrad(const void* dy, const void* x, float* dw_oihw, void* work, int dtype, int64_t groups,
                      int64_t N, int64_t Hi, int64_t Wi, int64_t Ci, int64_t Co, int64_t R, int64_t S,
                      int64_t stride, int64_t pad, int64_t dy_gs, int64_t x_gs, int64_t dw_gs, int accumulate,
                      void* stream);
/* The same weight gradient with the split-K fold INSIDE the launch (round 6; same semantics: autograd of
 * torchreid/models/resnet.py:164-184's convs).  The workgroups of an output tile store their fp32 partial tiles write-through,
 * take a ticket, and the one that completes the count adds the tiles up IN SPLIT ORDER (two levels for more than 16 splits) and
 * writes the OIHW gradient: bit-reproducible from run to run (no float atomics), no reduction launch, no second pass over the
 * slabs from a cold cache.  The association differs from ieee_conv2d_wgrad's (groups of ~sqrt(nsplit) splits instead of 16
 * strided lanes), so the two agree to fp32 rounding, not bit for bit.
 * tickets: ieee_conv2d_wgrad_fold_ticket_words() int32 words, ZERO before the first call; every completed launch leaves them
 * zero, so consecutive calls on one stream may share them (calls on different streams may not).  `work` as for
 * ieee_conv2d_wgrad (the query covers the level-1 slabs).  Shapes the fold does not cover (fp32, the stem, a single split,
 * unaligned gradients) take ieee_conv2d_wgrad's path and leave the tickets untouched. */
int64_t ieee_conv2d_wgrad_fold_ticket_words(void);
int ieee_conv2d_wgrad_fold(const void* dy, const void* x, float* dw_oihw, void* work, int32_t* tickets, int dtype,
                           int64_t groups, int64_t N, int64_t Hi, int64_t Wi, int64_t Ci, int64_t Co, int64_t R, int64_t S,
                           int64_t stride, int64_t pad, int64_t dy_gs, int64_t x_gs, int64_t dw_gs, int accumulate,
                           void* stream);
/* The same weight gradient with its slab reduction DEFERRED: the launch leaves the split-K slabs in `work` (which must then
 * stay untouched until the reduction has run) and describes the reduction in *reduce; ieee_wgrad_reduce_batch runs the
 * reductions of many weight gradients in ONE launch.  Usage: collect the descriptors of a group of layers, drop those
 * with kind == 0 (nothing left to reduce), set block_begin to the running sum of `blocks`, copy the table to the device
 * and call ieee_wgrad_reduce_batch(table, n, sum of blocks, groups, stream) on the stream the gradients were launched on.
 * Same arithmetic, same fixed summation order as the immediate form (bit-identical gradients). */
typedef struct ieee_wgrad_reduce_desc {
  const float* slab;        /* device: [groups][nsplit][Co][RS * Ci] */
  float* dw;                /* device: OIHW gradient, group stride dw_gs */
  int64_t slab_gs, dw_gs;
  int32_t nsplit, Co, Ci, RS;
  int32_t kind;             /* 0 nothing to do, 1 / 2 split-lane form (16-byte / scalar), 3 LDS-transposed 3x3 form */
  int32_t sl_log2, blocks;  /* workgroups per group */
  int32_t accumulate;
  int32_t block_begin;      /* filled by the caller: first blockIdx.x of this entry in the batched launch */
  int32_t reserved_;
} ieee_wgrad_reduce_desc;
int ieee_conv2d_wgrad_deferred(const void* dy, const void* x, float* dw_oihw, void* work, int dtype, int64_t groups,
                      int64_t N, int64_t Hi, int64_t Wi, int64_t Ci, int64_t Co, int64_t R, int64_t S,
                      int64_t stride, int64_t pad, int64_t dy_gs, int64_t x_gs, int64_t dw_gs, int accumulate,
                      ieee_wgrad_reduce_desc* reduce, void* stream);
int ieee_wgrad_reduce_batch(const ieee_wgrad_reduce_desc* device_descs, int64_t n, int64_t total_blocks, int64_t groups,
                            void* stream);

/* Which kernel form a conv call of this shape runs, WITHOUT running it: host arithmetic only (no HIP call, works on a machine
 * without a GPU), computed by the functions the launchers themselves call, so a test can assert "this shape runs that form" and
 * notices a retune.  No reference counterpart (torch picks its own algorithms).  (Hi, Wi, Ci, Co, R, S, stride, pad) are the
 * FORWARD conv's, as in the calls above.  Pointers are taken as 16-byte aligned, dw_gs as Co*Ci*R*S.
 * op: which entry point; flags: the options of that call that change the choice. */
#define IEEE_CONV_OP_FWD 0          /* ieee_conv2d_fwd(_ex) */
#define IEEE_CONV_OP_FWD_BN_EVAL 1  /* ieee_conv2d_fwd_bn_eval */
#define IEEE_CONV_OP_DGRAD 2        /* ieee_conv2d_dgrad(2, _ex) */
#define IEEE_CONV_OP_WGRAD 3        /* ieee_conv2d_wgrad(_fold, _deferred) */
#define IEEE_PLAN_F_BN_SUMS 1       /* bn_partial != NULL (forward: MODE 1, dgrad: MODE 2) */
#define IEEE_PLAN_F_ADDEND_S2 2     /* dgrad: addend_stride == 2 */
#define IEEE_PLAN_F_BN2 4           /* dgrad: bn_y2 / bn_partial2 given */
#define IEEE_PLAN_F_TICKETS 8       /* wgrad: ieee_conv2d_wgrad_fold */
#define IEEE_PLAN_F_DEFERRED 16     /* wgrad: ieee_conv2d_wgrad_deferred */
#define IEEE_PLAN_F_ACCUMULATE 32   /* wgrad: accumulate = 1 */
#define IEEE_PLAN_F_ADDEND 64       /* dgrad addend / eval residual != NULL */
/* indices into fields[] (entries a family does not have are 0) */
#define IEEE_PLAN_FAMILY 0          /* forward / dgrad: 0 gather, 1 3x3 patch, 2 direct stem; wgrad: 0 TN, 1 3x3 patch, 2 direct stem */
#define IEEE_PLAN_BN 1              /* output-channel tile width: 64 / 128 / 256 */
#define IEEE_PLAN_PIPE 2
#define IEEE_PLAN_MODE 3            /* epilogue: 0 store(+addend), 1 BN sums, 2 masked gradient + BN-backward sums, 3 eval BN */
#define IEEE_PLAN_VAR 4             /* 1 parity-class rows, 2 compact stride-2 addend, 3 second BatchNorm */
#define IEEE_PLAN_SLOW 5            /* element-gather loaders */
#define IEEE_PLAN_WLOG 6            /* patch forms: log2 of the map width */
#define IEEE_PLAN_STYLE 7           /* patch forward / dgrad: 0 two weight stages, 1 one */
#define IEEE_PLAN_LOADER 8          /* 0 plain 1x1 matrix, 1 im2col, 2 im2col over parity-class rows */
#define IEEE_PLAN_TILES_M 9
#define IEEE_PLAN_TILES_N 10
#define IEEE_PLAN_HALF_M 11         /* wgrad: 64-row tile */
#define IEEE_PLAN_FOLD 12           /* wgrad: split-K fold inside the launch */
#define IEEE_PLAN_NSPLIT 13
#define IEEE_PLAN_KCHUNK 14         /* pixels per split */
#define IEEE_PLAN_LEAN 15           /* wgrad TN: clamped lean loaders */
#define IEEE_PLAN_XCD_GROUP 16
#define IEEE_PLAN_DIRECT 17         /* wgrad: one split written straight into dw */
#define IEEE_PLAN_RADIX 18          /* fold: splits per level-0 group */
#define IEEE_PLAN_N1 19             /* fold: level-0 groups (1 = one level) */
#define IEEE_PLAN_REDUCE 20         /* slab reduction launch: 0 none, 1 vec4, 2 taps, 3 scalar */
#define IEEE_PLAN_SL_LOG2 21
#define IEEE_PLAN_NFIELDS 22
/* writes min(nfields, IEEE_PLAN_NFIELDS) entries; IEEE_ERR_UNSUPPORTED (with ieee_last_error) where the call itself refuses */
int ieee_conv_plan(int op, int dtype, int64_t groups, int64_t N, int64_t Hi, int64_t Wi, int64_t Ci, int64_t Co,
                   int64_t R, int64_t S, int64_t stride, int64_t pad, int64_t flags, int64_t* fields, int64_t nfields);


/* ---- BatchNorm2d (+ residual, + ReLU) over NHWC maps [M][C] ------------------ */
/* torch.nn.BatchNorm2d as the reference instantiates it (resnet.py:151,164-184;
 * ieee3modalPart.py:38): eps/momentum passed in, biased variance to normalise,
 * unbiased for running_var.  groups x [M][C] activations, stride act_gs;
 * gamma/beta at param_gs, running stats at buf_gs.
 * stats  : out, groups x [4][C] = mean, invstd, scale, shift (kept for backward)
 * partial: scratch of groups * ieee_bn_partial_floats() floats; with stats_rblocks > 0 it already holds the
 *          [2][C][stats_rblocks] sums emitted by ieee_conv2d_fwd and the statistics kernel is skipped;
 *          stats_rblocks < 0 (training): `stats` is final as the caller hands it in, the apply pass only
 * out = [relu]( y*scale + shift [+ residual] ); out NULL = statistics only.  training=0 uses running stats. */
int64_t ieee_bn_partial_floats(int dtype, int64_t M, int64_t C);
int ieee_bn2d_fwd(const void* y, const void* residual, void* out, int dtype, int64_t groups, int64_t M,
                  int64_t C, int64_t act_gs, const float* gamma, const float* beta, int64_t param_gs,
                  float* running_mean, float* running_var, int64_t buf_gs, float* stats, float* partial,
                  float momentum, float eps, int training, int relu, int64_t stats_rblocks, void* relu_bits,
                  void* stream);
/* backward of out = [relu](bn(y) [+ residual]): g = dout * [out_mask > 0] (out_mask NULL = no ReLU, or,
 * with mask_from_y = 1, the mask is recomputed as [y*scale+shift > 0], valid when there was no residual);
 * dy = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)); g_out (optional) receives g, which is also
 * the gradient of the residual branch.  dgamma/dbeta fp32 at grad_gs (NULL to skip).
 * coef: scratch groups x [3][C]. */
int ieee_bn2d_bwd(const void* dout, const void* out_mask, const void* y, void* dy, void* g_out, int dtype,
                  int64_t groups, int64_t M, int64_t C, int64_t act_gs, const float* gamma, int64_t param_gs,
                  const float* stats, float* dgamma, float* dbeta, int64_t grad_gs, float* partial,
                  float* coef, int accumulate, int mask_from_y, int64_t stats_rblocks, void* stream);
/* the same with `done_event` (a hipEvent_t or NULL): signalled when the call's last kernel completes, carried by that
 * dispatch itself instead of a separate event record behind it (a record is a barrier packet in the queue: +5 us
 * before the next kernel of the stream).  The executor forks its weight-gradient stream from these events. */
int ieee_bn2d_bwd_ev(const void* dout, const void* out_mask, const void* y, void* dy, void* g_out, int dtype,
                  int64_t groups, int64_t M, int64_t C, int64_t act_gs, const float* gamma, int64_t param_gs,
                  const float* stats, float* dgamma, float* dbeta, int64_t grad_gs, float* partial,
                  float* coef, int accumulate, int mask_from_y, int64_t stats_rblocks, void* done_event, void* stream);
/* BatchNorm statistics as order-independent TOTALS (round 4; no reference counterpart: autograd's batch_norm computes its
 * statistics in one kernel, torchreid/models/resnet.py:164-184 only calls it).  ieee_conv_next_bn_totals arms the NEXT
 * ieee_conv2d_fwd (with fused statistics) or ieee_conv2d_dgrad / _dgrad2 (with fused backward sums) issued by the calling
 * thread: instead of one float per (channel, 128-row tile) in bn_partial, every tile ADDS its per-channel sums, as 64-bit
 * fixed point (2^24 forward: sum y, sum y^2; 2^40 backward: sum g, sum g*y), to totals[group][2][C] with no-return global
 * atomics.  Integer adds commute: the totals are bit-reproducible whatever the arrival order; nothing inside the conv waits.
 * The caller zeroes the totals beforehand.  ieee_bn2d_fwd_totals / ieee_bn2d_bwd_totals then finalize AND apply in one
 * launch (every workgroup derives its channels' coefficients from the 2 x C integers in its prologue; workgroup 0 publishes
 * stats / running statistics / d(gamma), d(beta)), i.e. the separate finalize launch of ieee_bn2d_fwd / ieee_bn2d_bwd
 * disappears.  bf16 only, C / 8 must divide 256.  Same results as the partial-sum path up to the last bit of a float sum.
 * Range and resolution of the fixed point: totals stay inside +-2^62 units -- forward sums up to 2.7e11 with 6e-8 absolute
 * resolution (a 131 072-row map reaches that at an rms of 1 400 per channel), backward sums up to 4.2e6 with 9e-13 (finer than
 * the float tile sum itself above 1.5e-5).  Range guard: a tile contributes at most 2^62 / (row tiles of the launch) units, so
 * the total of all tiles and replicas can NEVER wrap; a tile sum beyond that share, or a NaN one, is clamped and REPORTED:
 * `overflow` (may be NULL) points to 4 ints the caller owns -- device or host-mapped memory, zero before the step -- and
 * overflow[0] = 1: a forward tile sum was clamped, [1]: a backward one, [2] / [3]: a forward / backward total beyond half
 * the range (2^61; written by ieee_bn2d_fwd_totals / _bwd_totals).  Any non-zero word means the statistics of that step are
 * not the reference's (torch's fp32 batch_norm, torchreid/models/resnet.py:164-184, returns finite numbers or inf there):
 * the executor raises through ieee_net_bn_overflow; the per-tile partial-sum path (ieee_bn2d_fwd / ieee_bn2d_bwd) has no
 * such limit.
 * `replicas` (a power of two <= 64; 1 = plain) spreads the adders: totals[replica][group][2][C] (group_stride = 2 * C), row
 * tile t adds to replica t % replicas, and the BatchNorm passes add the replicas up in their prologue -- same-address atomics
 * retire at ~23 ns each, so a launch of 1 024 row tiles pays +24 us with one copy and +3 us with eight. */
int ieee_conv_next_bn_totals(void* totals, int64_t group_stride, int replicas, int* overflow);   /* DEPRECATED: see ieee_conv_extras */
/* EXPLICIT-ARGUMENT forms (round 6; SURVEY.md section 8b: "stateless, re-entrant, all work on the caller-supplied stream").
 * ieee_conv_next_bn_totals / ieee_conv_profile_events change what the NEXT conv call of the thread does -- hidden per-thread
 * state a binding cannot express as one call.  ieee_conv2d_fwd_ex / ieee_conv2d_dgrad_ex take the same options as one struct
 * (NULL = none) and leave nothing behind; the executor calls these.  The two arming entry points stay as thin deprecated
 * wrappers over the same mechanism (they are disarmed on every return path of the next conv call, as before).
 *   totals / group_stride / replicas / overflow : as ieee_conv_next_bn_totals (totals NULL = per-tile partials in bn_partial)
 *   start / stop : hipEvent_t pair (timing enabled) the launch carries as its own start / stop signals, or NULL, NULL */
typedef struct ieee_conv_extras {
  void* totals;
  int64_t group_stride;
  int32_t replicas;
  int32_t reserved_;        /* 0 */
  int* overflow;
  void* start;
  void* stop;
} ieee_conv_extras;
int ieee_conv2d_fwd_ex(const void* x, const void* w_packed, void* y, int dtype, int64_t groups, int64_t N, int64_t Hi,
                       int64_t Wi, int64_t Ci, int64_t Co, int64_t R, int64_t S, int64_t stride, int64_t pad, int64_t x_gs,
                       int64_t w_gs, int64_t y_gs, float* bn_partial, const ieee_conv_extras* extras, void* stream);
int ieee_conv2d_dgrad_ex(const void* dy, const void* w_packed_d, void* dx, const void* addend, int dtype,
                         int64_t groups, int64_t N, int64_t Hi, int64_t Wi, int64_t Ci, int64_t Co, int64_t R,
                         int64_t S, int64_t stride, int64_t pad, int64_t dy_gs, int64_t w_gs, int64_t dx_gs,
                         float* bn_partial, const void* bn_y, const void* bn_mask, const float* bn_stats,
                         int bn_mask_bits, int addend_stride, const void* bn_y2, float* bn_partial2,
                         const ieee_conv_extras* extras, void* stream);
int ieee_bn2d_fwd_totals(const void* y, const void* residual, void* out, int dtype, int64_t groups, int64_t M,
                         int64_t C, int64_t act_gs, const float* gamma, const float* beta, int64_t param_gs,
                         float* running_mean, float* running_var, int64_t buf_gs, float* stats, const void* totals,
                         int replicas, float momentum, float eps, int relu, void* relu_bits, int* overflow, void* stream);
int ieee_bn2d_bwd_totals(const void* dout, const void* out_mask, const void* y, void* dy, void* g_out, int dtype,
                         int64_t groups, int64_t M, int64_t C, int64_t act_gs, const float* gamma, int64_t param_gs,
                         const float* stats, float* dgamma, float* dbeta, int64_t grad_gs, const void* totals,
                         int replicas, int mask_from_y, int* overflow, void* done_event, void* stream);
/* ieee_bn2d_bwd_totals for the LAST BatchNorm of a bottleneck block with a downsample branch (out = relu(bn3(y3) + bn_ds(y_ds)),
 * torchreid/models/resnet.py:164-184: both BatchNorm backwards see the same masked gradient g = dout): dy = the backward of
 * bn3 as above (no mask, no g output), and -- while g streams by -- the branch's backward sums, sum g and sum g*y_ds, are ADDED to
 * totals_ds [replicas_ds][groups][2][C] (2^40 fixed point, zero beforehand; same range guard: overflow[1] / [3]), so that the
 * branch's BatchNorm backward is one ieee_bn2d_bwd_totals launch without a reduction pass or a finalize launch. */
int ieee_bn2d_bwd_totals_ds(const void* dout, const void* y, const void* y_ds, void* dy, int dtype, int64_t groups, int64_t M,
                            int64_t C, int64_t act_gs, const float* gamma, int64_t param_gs, const float* stats,
                            float* dgamma, float* dbeta, int64_t grad_gs, const void* totals, int replicas, void* totals_ds,
                            int replicas_ds, int* overflow, void* done_event, void* stream);
/* backward through a FROZEN BatchNorm2d (module.eval() while the rest trains: open_specified_layers, utils/torchtools.py:
 * 183-221): `stats` holds the running-statistics scale / shift of the forward (ieee_bn2d_fwd with training = 0), the map
 * is a fixed affine one and dy = scale * g, g = dout * mask as in ieee_bn2d_bwd; no parameter gradient is produced. */
int ieee_bn2d_bwd_frozen(const void* dout, const void* out_mask, const void* y, void* dy, void* g_out, int dtype,
                         int64_t groups, int64_t M, int64_t C, int64_t act_gs, const float* stats, float* coef,
                         int mask_from_y, void* done_event, void* stream);
/* `done_event` above is never hipEventRecord-ed: it is the stop event of hipExtLaunchKernelGGL, and a consumer orders
 * another stream behind it with hipStreamWaitEvent.  HIP does not document that such an event orders a second stream, so
 * the dependency is MEASURED once per process before it is relied on: a ~300 us spinning kernel carries a pooled
 * hipEventDisableTiming event on stream_a, stream_b waits on it and reads the flag the kernel sets last (three rounds, one
 * 8-byte allocation, host-synchronous on both streams -- the only place the library waits for the device).  The executor
 * passes its launch and side stream; the check creates no streams of its own (doing so in the middle of a step disturbed
 * the runtime's hardware-queue assignment: the side stream stopped overlapping the launch stream).  Returns 0 when the
 * event rides (cached for the process), non-zero otherwise; the executor then falls back to hipEventRecord
 * (IEEE_EVENT_RIDE=0 forces that).  Replaces nothing in the reference (its streams are torch's). */
int ieee_event_ride_selfcheck(void* stream_a, void* stream_b);

/* ---- stem plumbing ----------------------------------------------------------- */
/* three fp32 NCHW image tensors (batch dict 'img' = [RGB, NI, TI], dataset.py:338-351) ->
 * [3][B][H+2*pad][W+2*pad][Cpad], channels C..Cpad-1 and the `pad`-pixel border zero.  The executor's stem uses
 * Cpad = 4, pad = 3: conv1 (7x7/2, pad 3; resnet.py:622) then is an 8x8/2 convolution WITHOUT padding over 4
 * channels (8th filter row / column and 4th channel zero), whose k-tile of 64 is two filter rows of 8 contiguous
 * pixels and needs no bounds tests */
int ieee_nchw_to_nhwc3(const float* x_rgb, const float* x_ni, const float* x_ti, void* out, int dtype,
                       int64_t B, int64_t C, int64_t H, int64_t W, int64_t Cpad, int64_t pad, void* stream);
/* nn.MaxPool2d(3, 2, 1) (resnet.py:501); argmax holds the window-local index of the first maximum */
int ieee_maxpool3x3s2_fwd(const void* x, void* out, uint8_t* argmax, int dtype, int64_t groups, int64_t B,
                          int64_t Hi, int64_t Wi, int64_t C, void* stream);
/* The stem's BatchNorm apply + ReLU + max-pool in one pass (training forward): pooled = maxpool(relu(y * scale + shift)) with
 * scale / shift from `stats` ([groups][4][C]: mean, invstd, scale, shift, as ieee_bn2d_fwd leaves them) and the activation
 * rounded to the storage type before the comparison -- out / argmax are bit-identical to ieee_bn2d_fwd(out = a, relu) followed
 * by ieee_maxpool3x3s2_fwd(a), without the full-resolution activation ever being written (torchreid/models/resnet.py:622-626). */
int ieee_bn_relu_maxpool3x3s2_fwd(const void* y, const float* stats, void* out, uint8_t* argmax, int dtype, int64_t groups,
                                  int64_t B, int64_t Hi, int64_t Wi, int64_t C, void* stream);

int ieee_maxpool3x3s2_bwd(const void* dout, const uint8_t* argmax, void* dx, int dtype, int64_t groups,
                          int64_t B, int64_t Hi, int64_t Wi, int64_t C, void* stream);

/* backward of maxpool(relu(bn(y))) w.r.t. y in two passes (the stem, resnet.py:622-626 reversed): the max-pool
 * backward of dpool [groups][B][Ho][Wo][C] is gathered on the fly, masked by [y*scale+shift > 0] and pushed through
 * the BatchNorm backward (same dgamma / dbeta / coef / partial contract as ieee_bn2d_bwd, M = B*Hi*Wi) */
int ieee_bn2d_bwd_pooled(const void* dpool, const uint8_t* argmax, const void* y, void* dy, int dtype,
                         int64_t groups, int64_t B, int64_t Hi, int64_t Wi, int64_t C, const float* gamma,
                         int64_t param_gs, const float* stats, float* dgamma, float* dbeta, int64_t grad_gs,
                         float* partial, float* coef, int accumulate, void* stream);

/* ---- Cross-modal Interacting Module tail (ieee3modalPart.py:266-282, 427-455) -- */
/* F [3][B][H*W][C]: S_m = F_a + F_b (the two other modalities; S may be NULL), Gp_m = mean over positions
 * (AdaptiveAvgPool2d((1,1)) of the raw trunk map, :449-451) */
int ieee_gpool_sum_others(const void* F, void* S, float* Gp, int dtype, int64_t B, int64_t H, int64_t W,
                          int64_t C, void* stream);
/* ChannelAttention pools of rest = relu(bn(y2)): avg / max over positions at avg|mx + m*pool_gs + b*C + c,
 * argmax [3][B][C] */
int ieee_ca_pool(const void* y2, const float* stats2, float* avg, float* mx, int64_t pool_gs, int32_t* argmax,
                 int dtype, int64_t B, int64_t H, int64_t W, int64_t C, void* stream);
/* parts_out[3][B][parts][C] = AdaptiveAvgPool2d((parts,1)) of relu(bn(y1)) + relu(bn(y2))*(1+att);
 * mode 0 full CIM, 1 attention off, 2 interaction off (pool y1 as is) */
int ieee_cim_tail_fwd(const void* y1, const void* y2, const float* stats1, const float* stats2,
                      const float* att, float* parts_out, int dtype, int64_t B, int64_t H, int64_t W,
                      int64_t C, int64_t parts, int mode, void* stream);
int ieee_cim_tail_bwd_datt(const float* dparts, const void* y2, const float* stats2, float* datt, int dtype,
                           int64_t B, int64_t H, int64_t W, int64_t C, int64_t parts, void* stream);
int ieee_cim_tail_bwd_g(const float* dparts, const void* y1, const void* y2, const float* stats1,
                        const float* stats2, const float* att, const float* davg, const float* dmax,
                        int64_t pool_gs, const int32_t* argmax, void* g1, void* g2, int dtype, int64_t B,
                        int64_t H, int64_t W, int64_t C, int64_t parts, int mode, float* bn_partial1,
                        float* bn_partial2, void* stream);
/* bn_partial1/2 (both or neither; modes 0/1): also emit the BatchNorm-backward sums of convOne / convAvgRest as
 * [3][2][C][B] per-sample partials (sum g, sum g*y of the stored g1 / g2): ieee_bn2d_bwd(stats_rblocks = B) then
 * skips its reduction pass */
/* dF_m = D1_m + DS_a + DS_b + dGp_m / (H*W) */
int ieee_cim_bwd_combine(const void* D1, const void* DS, const float* dG, void* dF, int dtype, int64_t B,
                         int64_t H, int64_t W, int64_t C, int mode, void* stream);

/* ---- embedding head, fp32, grouped through host pointer tables (<= IEEE_MAX_GROUPS) ---- */
/* C[g](m,n) = act(alpha * sum_k A[g](m,k)*B[g](n,k) + bias[g](n)) (+ C[g] when accumulate);
 * A(m,k) = A + m*sam + k*sak, B(n,k) = B + n*sbn + k*sbk: nn.Linear / 1x1 conv on pooled vectors and
 * their backward GEMMs (ieee3modalPart.py:54-56, 272-274, 335-340, 396-424, 374-391) */
int ieee_sgemm_grouped(int64_t groups, const void* const* A, const void* const* B, void* const* C,
                       const void* const* bias, int64_t M, int64_t N, int64_t K, int64_t sam, int64_t sak,
                       int64_t sbn, int64_t sbk, int64_t ldc, float alpha, int relu, int accumulate,
                       void* stream);
/* same, with a scratch buffer: long-K problems with few 64x64 tiles (the pooled-vector GEMMs: K = 2048 reduce
 * conv / CA fc1, K = 768 REM / fc heads) are split along K into `work` slabs that a second kernel adds in a fixed
 * order (deterministic); work == NULL or too small = no split.  16 MiB covers every GEMM of the head. */
int ieee_sgemm_grouped_ws(int64_t groups, const void* const* A, const void* const* B, void* const* C,
                          const void* const* bias, int64_t M, int64_t N, int64_t K, int64_t sam, int64_t sak,
                          int64_t sbn, int64_t sbk, int64_t ldc, float alpha, int relu, int accumulate, void* work,
                          int64_t work_bytes, void* stream);
/* TWO uniform problem sets in ONE launch (round 6): the independent GEMM pairs of a head phase -- dW and dX of one nn.Linear /
 * 1x1 conv (ieee3modalPart.py:54-56, 396-424, 484-511 through autograd), the reduce_layer applied to the global vector and
 * to the six parts (:449-455) -- each set described as ieee_sgemm_grouped's arguments.  Every output has the bits of the
 * separate ieee_sgemm_grouped_ws call made with HALF of `work_bytes` (each set plans its split-K against its half of `work`).
 * The two sets must not write overlapping outputs. */
typedef struct ieee_sgemm_set {
  int64_t groups;
  const void* const* A;
  const void* const* B;
  void* const* C;
  const void* const* bias;      /* may be NULL */
  int64_t M, N, K, sam, sak, sbn, sbk, ldc;
  float alpha;
  int32_t relu, accumulate;
} ieee_sgemm_set;
int ieee_sgemm_grouped_pair_ws(const ieee_sgemm_set* s0, const ieee_sgemm_set* s1, void* work, int64_t work_bytes,
                               void* stream);
/* zero `count` (<= IEEE_MAX_GROUPS) float spans in one launch */
int ieee_zero_spans(int64_t count, void* const* ptrs, const int64_t* floats, void* stream);
int ieee_colsum_grouped(int64_t groups, const void* const* X, void* const* out, int64_t M, int64_t N,
                        int64_t ldx, int accumulate, void* stream);
/* BatchNorm over the rows of [R][C] (+ReLU): BatchNorm2d on [B,C,1,1] / [B,C,6,1] (reduce_layer, applied
 * twice per step :449-455) and BatchNorm1d of the 18 fc heads (:417).  save[g] = [2][C] mean, invstd */
int ieee_rowbn_fwd(int64_t groups, const void* const* x, void* const* out, const void* const* gamma,
                   const void* const* beta, void* const* running_mean, void* const* running_var,
                   void* const* save, int64_t R, int64_t C, int64_t ldx, int64_t ldo, float momentum,
                   float eps, int training, int relu, void* stream);
/* backward: relu bit 0 = the forward applied ReLU; bit 1 = FROZEN BatchNorm (the forward ran with training = 0, e.g. a
 * child outside `open_layers` during the fixbase epochs, utils/torchtools.py:183-221): dx = gamma * invstd * g and
 * dgamma / dbeta are left untouched */
int ieee_rowbn_bwd(int64_t groups, const void* const* dout, const void* const* out, const void* const* x,
                   const void* const* gamma, const void* const* save, void* const* dx, void* const* dgamma,
                   void* const* dbeta, int64_t R, int64_t C, int64_t lddo, int64_t ldo, int64_t ldx,
                   int64_t lddx, int relu, int accumulate, void* stream);
/* ChannelAttention glue: h [3][2B][hidden] (avg rows then max rows, ReLU applied) -> hs = h_avg + h_max */
int ieee_ca_mix_fwd(const float* h, float* hs, int64_t B, int64_t hidden, void* stream);
int ieee_ca_mix_bwd(const float* dhs, const float* h, float* dh, int64_t B, int64_t hidden, void* stream);
int ieee_sigmoid_fwd(float* x, int64_t n, void* stream);
int ieee_sigmoid_bwd(const float* datt, const float* att, float* dz, int64_t n, void* stream);
/* REM closed form (nonLocal.forward, ieee3modalPart.py:60-80): out = part + 2*param*r, r = W_p g + b_p */
int ieee_rem_fwd(const float* part, const float* r, const float* param, int64_t param_gs, float* out,
                 int64_t B, int64_t parts, int64_t D, void* stream);
int ieee_rem_bwd(const float* dout, const float* r, const float* param, int64_t param_gs, float* dr,
                 float* dparam, int64_t grad_gs, float* work, int64_t B, int64_t parts, int64_t D,
                 int accumulate, void* stream);
/* F.normalize(p=2, dim=1, eps=1e-12) (:519) */
int ieee_l2norm_fwd(const float* x, float* y, float* norms, int64_t rows, int64_t D, void* stream);
int ieee_l2norm_bwd(const float* dy, const float* y, const float* norms, float* dx, int64_t rows, int64_t D,
                    int accumulate, void* stream);

/* ---- losses and optimizer ------------------------------------------------------- */
/* label-smoothed CE (torchreid/losses/cross_entropy_loss.py:36-50) over `heads` logits tensors [B][C];
 * head_loss[h] = (-t*logp).mean(0).sum(), head_acc[h] = top-1 % (metrics/accuracy.py);
 * dlogits (optional) = d(sum_h head_loss)/dlogits * grad_scale.  work: heads*B*2 floats. */
int ieee_ce_ls_fwd_bwd(const float* logits, const int64_t* targets, float* dlogits, float* head_loss,
                       float* head_acc, float* work, int64_t heads, int64_t B, int64_t C, float eps,
                       float grad_scale, void* stream);
/* 3M loss (torchreid/losses/multi_modal_margin_loss_new.py:19-40); feats [3][B][D] = R,N,T;
 * out3 = {loss, label_num, chunks torch.chunk would yield}; dfeats optional; work: B+3 floats */
int ieee_margin3m_fwd_bwd(const float* feats, const int64_t* pids, float* dfeats, float* out3, float* work,
                          int64_t B, int64_t D, float margin, float grad_scale, void* stream);
/* Batch-hard triplet loss (torchreid/losses/hard_mine_triplet_loss.py:23-48), forward and backward, 2 launches.
 * x [parts][B][D] fp32: the descriptor of row i is the concatenation over parts of x[p][i][0..D) (parts = 1: a plain
 * [B][D] matrix; parts = 3: the executor's feats tensor).  d_ij = sqrt(max(d2_ij, 1e-12)) with d2 formed from DIFFERENCES,
 * sum (x_i - x_j)^2: exactly 0 on the diagonal and for duplicate rows.  (The reference's Gram expansion in fp32 leaves
 * +-6.6e-7 on the diagonal at D = 2304.)  Hardest positive = max over the same identity, the row itself included; hardest
 * negative = min over the others; loss = mean over anchors of max(0, margin + d_ap - d_an).
 * out[4] = {loss, mean d_ap, mean d_an, anchors with a positive hinge}.  dx (optional, layout of x) = the exact gradient *
 * grad_scale, written (accumulate = 0) or added to what is there (accumulate = 1): pairs with d2 < 1e-12 contribute
 * nothing, exactly equal maxima / minima share their anchor's gradient evenly, an anchor whose hinge is <= 0 contributes
 * nothing.  Gather form, fixed summation order, no atomics: the same bits on every call.  Identities need not be
 * contiguous.  A batch with one identity has no negatives: d_an = +inf, every hinge 0 (callers raise before the launch).
 * 1 <= B <= 4096, D >= 1, 1 <= parts <= 64, else IEEE_ERR_BAD_ARG before any launch.  work: B*B + 5*B floats. */
int ieee_triplet_hard_fwd_bwd(const float* x, int64_t parts, const int64_t* pids, float* dx, float* out, float* work,
                              int64_t B, int64_t D, float margin, float grad_scale, int accumulate, void* stream);
/* Per-identity-chunk centre losses, feats [M][B][D] fp32, torch.chunk semantics as ieee_margin3m_fwd_bwd has them;
 * out3 = {loss, label_num, chunks torch.chunk would yield}; dfeats optional (written, or added to with accumulate = 1);
 * work: B+3 floats.
 *   mode IEEE_CENTER_HETERO (torchreid/losses/hcloss.py:18-39, M = 2), summed over the chunks:
 *     IEEE_DIST_L2 |sum_k (c1-c2)^2|, IEEE_DIST_L1 |mean_k |c1-c2||, IEEE_DIST_COS max(0, 1 - cos(c1, c2)) (eps 1e-8);
 *     `margin` is not used (the reference stores and ignores it).
 *   mode IEEE_CENTER_MARGIN3M (multi_modal_margin_loss_new.py:19-40, M = 3): max(|m-d12|, |m-d23|, |m-d13|), the first
 *     maximal argument in that order, d = IEEE_DIST_L2 (the bits of ieee_margin3m_fwd_bwd) or IEEE_DIST_L1 (nn.L1Loss:
 *     the MEAN of absolute differences; sign(0) = 0).  IEEE_DIST_COS: IEEE_ERR_BAD_ARG (the reference's branch never
 *     assigns its distance). */
#define IEEE_DIST_L2 0
#define IEEE_DIST_L1 1
#define IEEE_DIST_COS 2
#define IEEE_CENTER_HETERO 0
#define IEEE_CENTER_MARGIN3M 1
int ieee_center_pairs_fwd_bwd(const float* feats, int64_t M, const int64_t* pids, float* dfeats, float* out3,
                              float* work, int64_t B, int64_t D, int dist_type, int mode, float margin,
                              float grad_scale, int accumulate, void* stream);
/* torch.optim.SGD(momentum, weight_decay, dampening=0, nesterov) as configured by the reference
 * (torchreid/optim/optimizer.py:130-138) over a flat fp32 range */
/* The same update with two options (either may be NULL; round 6).  Reference: torchreid/optim/optimizer.py:130-138.
 *  shadow_bf16: ALSO write the bf16 image of the updated parameters (round-to-nearest-even, the conversion the weight packing
 *    uses) to shadow_bf16[i], i in [0, n) -- the slice of a bf16 SHADOW of the flat parameter buffer.  With ieee_net_set_shadow
 *    the training forward reads the GEMM operands of the 1x1 convolutions straight from that shadow (Wf[co][ci] of a 1x1 conv
 *    is its OIHW weight), so the once-per-step weight packing loses 64 % of the conv parameters; 2 B/param of optimizer writes.
 *  skip_flags: the executor's range-guard words (device memory, ieee_net_bn_flags_offset).  When [0] or [1] is set -- a
 *    BatchNorm tile sum of THIS step left the fixed-point range, so its gradients are not the reference's -- the launch
 *    changes nothing: parameters, momentum and shadow stay as they were (the step is skipped, like an overflow step of a loss
 *    scaler) and training can go on from an undamaged state once the engine has switched to the partial-sum path. */
int ieee_sgd_nesterov_step_ex(float* params, const float* grads, float* momentum_buf, int64_t n, float lr, float momentum,
                              float weight_decay, int nesterov, void* shadow_bf16, const int* skip_flags, void* stream);
/* running statistics under the same guard: flags[0] set (a forward tile sum of this step was clamped) -> buffers[i] =
 * backup[i], the values before the step; else backup[i] = buffers[i].  One launch per step behind the forward. */
int ieee_guard_buffers(const int* flags, float* buffers, float* backup, int64_t n, void* stream);
int ieee_sgd_nesterov_step(float* params, const float* grads, float* momentum_buf, int64_t n, float lr,
                           float momentum, float weight_decay, int nesterov, void* stream);
/* Gradient exchange in bf16 ("219 MB in bf16"; opt-in, IEEE_DP_GRAD_DTYPE=bf16): the slice of the flat
 * fp32 gradient a rank is about to all-reduce, rounded to nearest even into a bf16 staging range, and the reduced bf16
 * values widened back (exact).  The reference reduces fp32 gradients (nn.DataParallel's reduce_add,
 * scripts/mainMultiModal.py:219-220): the default stays fp32. */
int ieee_grad_pack_bf16(const float* grads, void* out_bf16, int64_t n, void* stream);
int ieee_grad_unpack_bf16(const void* in_bf16, float* grads, int64_t n, void* stream);
/* torch.optim.Adam / Adam(amsgrad=True) as the reference builds them for optim = 'adam' / 'amsgrad'
 * (torchreid/optim/optimizer.py:113-128): L2 weight decay, bias correction with `step` (1-based);
 * max_exp_avg_sq == NULL = plain Adam */
int ieee_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                   int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                   void* stream);
/* torch.optim.RMSprop(alpha, eps, weight_decay, momentum, centered=False) as the reference builds it for optim = 'rmsprop'
 * (torchreid/optim/optimizer.py:140-147; it passes `momentum` through, eps stays torch's 1e-8) over a flat fp32 range:
 * g += wd*p; sq = alpha*sq + (1-alpha)*g*g; buf = momentum*buf + g/(sqrt(sq)+eps); p -= lr*buf.  momentum == 0:
 * momentum_buf may be NULL and p -= lr*g/(sqrt(sq)+eps).  16 bytes per lane when every pointer is 16-byte aligned,
 * else a scalar form with the same per-element arithmetic.  n < 0 or a NULL pointer: IEEE_ERR_BAD_ARG. */
int ieee_rmsprop_step(float* params, const float* grads, float* square_avg, float* momentum_buf, int64_t n, float lr,
                      float alpha, float eps, float weight_decay, float momentum, void* stream);
/* The reference's own RAdam.step (torchreid/optim/radam.py:51-130, degenerated_to_sgd=True; built at
 * torchreid/optim/optimizer.py:149-155) -- NOT torch.optim.RAdam: decoupled decay p -= wd*lr*p only where an update
 * follows, the rectified branch from N_sma >= 5 with denominator sqrt(v)+eps, below it p -= lr*exp_avg/(1-beta1^t).
 * N_sma and step_size are derived from `step` (1-based) in double on every call (radam.py:94-110; the reference's
 * ten-slot buffer only caches them), so the call keeps no state.  step < 1, n < 0 or a NULL pointer: IEEE_ERR_BAD_ARG. */
int ieee_radam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int64_t step, void* stream);

/* ---- re-ranking ----------------------------------------------- */
/* k-reciprocal re-ranking, torchreid/utils/rerank.py:31-113 (engine/engine.py:402-406): device matrices
 * q_g_dist [Q][G], q_q_dist [Q][Q], g_g_dist [G][G] fp32 -> out [Q][G] fp32.  Dense like the reference (three
 * (Q+G)^2 fp32 work matrices: Q+G < 46000); rank ties are broken by index.  k1+1 <= 64.
 * For Q+G >= 46000 use ieee_rerank_sparse below: same arguments, same output bits, no (Q+G)^2 workspace. */
int64_t ieee_rerank_workspace_bytes(int64_t Q, int64_t G, int64_t k1);
int ieee_rerank(const float* q_g_dist, const float* q_q_dist, const float* g_g_dist, int64_t Q, int64_t G,
                int64_t k1, int64_t k2, double lambda_value, float* out, void* work, int64_t work_bytes,
                void* stream);
/* The same re-ranking in sparse form: the same arguments and bit-identical output to ieee_rerank wherever that runs,
 * with no N x N workspace (N = Q+G).  Bounds: Q, G >= 1, 1 <= k1 <= 63, k1+1 <= N < 2^31, 1 <= k2 <= k1+1.  The
 * inputs are read in two streaming passes (column maxima, then the k1+1 nearest of every column); the k-reciprocal
 * weights V and their query expansion Vq are stored as sparse rows, and the Jaccard sum walks an inverted index.
 * Workspace contract: ieee_rerank_sparse_workspace_bytes(Q, G, k1, k2) is a data-independent upper bound (no host
 * read-back, no allocation in the library): rows of V hold at most min(K(1+Kh), N) entries, rows of Vq at most
 * min(k2 K(1+Kh), N), K = k1+1, Kh = round_half_even(k1/2)+1.  It returns -1 (and sets the error text) for arguments
 * out of range.  About 2.8 GB at Q = 10000, G = 100000, k1 = 20, k2 = 6.  Inputs are taken to be finite; any bits
 * are memory-safe. */
int64_t ieee_rerank_sparse_workspace_bytes(int64_t Q, int64_t G, int64_t k1, int64_t k2);
int ieee_rerank_sparse(const float* q_g_dist, const float* q_q_dist, const float* g_g_dist, int64_t Q, int64_t G,
                       int64_t k1, int64_t k2, double lambda_value, float* out, void* work, int64_t work_bytes,
                       void* stream);
/* Where the intermediates of ieee_rerank_sparse lie in its workspace, for inspection after a call: fields[11] =
 * {K, capV, capVq, then byte offsets of rank [N][K] int32, V counts [N] int32, V columns [N][capV] int32, V values
 * [N][capV] fp32, Vq counts, Vq columns [N][capVq], Vq values, column maxima [N] (bits of fp32)}.  Vq is absent
 * (capVq = 0) when k2 = 1.  Row r of V holds counts[r] entries in ascending column order. */
int ieee_rerank_sparse_layout(int64_t Q, int64_t G, int64_t k1, int64_t k2, int64_t* fields);
/* The same re-ranking from descriptors (ieee_amd/csrc/rerank_stream.hip): ieee_rerank_sparse's steps and output bits
 * with no Q x Q, G x G or (Q+G)^2 input.  The virtual matrix orig = [[qq, qg], [qg^T, gg]] (N = Q+G rows and columns)
 * reaches the library block by block: the caller runs ieee_sqeuclid_distmat on the descriptors of a slab of rows
 * [a0, a1) and a strip of columns [i0, i1), each on one side of Q and at most `slab` long, into a buffer of its own and
 * hands that to ieee_rerank_stream_block.  Element (a, i) is buf[(a - a0) * sa + (i - i0) * si]: (sa, si) = (ld, 1), or
 * (1, ld) where the Q x G block -- always produced with the query as the row operand, as the matrix path produces it --
 * serves as orig[a in G][i in Q].  The order of calls, all on one stream, every one with the same Q, G, k1, k2, slab:
 *   ieee_rerank_stream_begin;
 *   for every strip: pass 0 over all its slabs (column maxima), then pass 1 over all its slabs (the k1+1 nearest of
 *     every column, as running lists that any number of slabs merge into; needs the strip's maxima complete);
 *   ieee_rerank_stream_sets (the ranking from the lists; the members of every row's expanded k-reciprocal set, counts
 *     and ascending members where ieee_rerank_stream_layout says V's are);
 *   ieee_distmat_member_pairs on those counts and members, writing into V's values (the members' distances);
 *   ieee_rerank_stream_rows (the weights V from those distances, and their query expansion Vq);
 *   ieee_rerank_stream_range for gallery ranges [g0, g1), g1 - g0 <= slab, in any order: dist holds the range's Q x
 *     (g1 - g0) distances (row stride ldd), and row i of the re-ranked distances goes to out + i * ldo.
 * Bounds as ieee_rerank_sparse, and slab >= 1.  The workspace is that of ieee_rerank_sparse with the inverted index
 * sized for one range: a data-independent bound, -1 for arguments out of range.  ieee_rerank_stream_layout: fields[14] =
 * the 11 of ieee_rerank_sparse_layout, then the byte offset of the running lists [N][k1+1] uint64 (bits(D) << 32 | j,
 * valid between pass 1 and ieee_rerank_stream_sets), the longest strip and the longest gallery range. */
int64_t ieee_rerank_stream_workspace_bytes(int64_t Q, int64_t G, int64_t k1, int64_t k2, int64_t slab);
int ieee_rerank_stream_layout(int64_t Q, int64_t G, int64_t k1, int64_t k2, int64_t slab, int64_t* fields);
int ieee_rerank_stream_begin(int64_t Q, int64_t G, int64_t k1, int64_t k2, int64_t slab, void* work, int64_t work_bytes,
                             void* stream);
int ieee_rerank_stream_block(int64_t pass, const float* buf, int64_t sa, int64_t si, int64_t a0, int64_t a1, int64_t i0,
                             int64_t i1, int64_t Q, int64_t G, int64_t k1, int64_t k2, int64_t slab, void* work,
                             int64_t work_bytes, void* stream);
int ieee_rerank_stream_sets(int64_t Q, int64_t G, int64_t k1, int64_t k2, int64_t slab, void* work, int64_t work_bytes,
                            void* stream);
int ieee_rerank_stream_rows(int64_t Q, int64_t G, int64_t k1, int64_t k2, int64_t slab, void* work, int64_t work_bytes,
                            void* stream);
int ieee_rerank_stream_range(const float* dist, int64_t ldd, int64_t g0, int64_t g1, double lambda_value, float* out,
                             int64_t ldo, int64_t Q, int64_t G, int64_t k1, int64_t k2, int64_t slab, void* work,
                             int64_t work_bytes, void* stream);
/* GNN re-ranking, torchreid/utils/GPU-Re-Ranking/gnn_reranking.py:27-59 with its build_adjacency_matrix and
 * gnn_propagate kernels: device features xq [Q][d], xg [G][d] fp32 (d % 8 == 0, nothing is normalised here) ->
 * out [Q][G] fp32 = 1 - sim, sim the cosine of the rows that two rounds of propagation leave, so that ascending out is
 * the reference's descending similarity.  With X_u = [xq; xg], N = Q + G: score = X_u X_u^T, (S, rank) = its k1 largest
 * per row; A = B + B^T with B[i][rank[i][j]] = 1; twice: A[i] = sum_{j<k2} S[i][j]^2 A[rank[i][j]] (j ascending, no
 * atomics: bitwise reproducible), rows L2-normalised and A + A^T formed between the rounds.  k2 = 1: out = 1 - (number
 * of shared k1-neighbours)/k1.  Defined where the reference is not: ties in rank are broken by the smaller index, and
 * a row of norm 0 gives similarity 0 (eps 1e-12), not NaN.  Bounds: Q, G >= 1, 1 <= k1 <= min(1024, N), 1 <= k2 <= k1,
 * else IEEE_ERR_BAD_ARG before any launch.  precision: 0 = fp32 MFMA, or IEEE_SPLIT_* for the two GEMMs (the scores
 * and the final product).  Workspace: two N x ld fp32 matrices (ld = N rounded up to 8), the two [N][k1] lists, [N]
 * row sums and the distance GEMM's scratch; ieee_gnn_rerank_workspace_bytes returns -1 (and sets the error text) for
 * arguments out of range.  Caller-owned memory, everything on `stream`, no host sync. */
int64_t ieee_gnn_rerank_workspace_bytes(int64_t Q, int64_t G, int64_t d, int64_t k1, int64_t k2, int precision);
int ieee_gnn_rerank(const float* xq, const float* xg, int64_t Q, int64_t G, int64_t d, int64_t k1, int64_t k2,
                    int precision, float* out, void* work, int64_t work_bytes, void* stream);
/* Where ieee_gnn_rerank keeps its intermediates, for inspection after a call: fields[7] = {ld, then byte offsets of
 * rank [N][k1] int32, S [N][k1] fp32 (the NEGATED scores, not squared: the propagation squares them as it loads),
 * row sums of squares [N] fp32 (of the last propagation), matrix M0 [N][ld], matrix M1 [N][ld], and the matrix whose
 * rows fed the final product (M1, the unnormalised second round; M0 = the binary B when k2 = 1)}. */
int ieee_gnn_rerank_layout(int64_t Q, int64_t G, int64_t d, int64_t k1, int64_t k2, int precision, int64_t* fields);

/* ---- GNN re-ranking on sparse rows: the algorithm of ieee_gnn_rerank with only the structural non-zeros stored, and
 * nothing of size N x N or Q x G allocated (N = Q + G).  A sparse matrix here is CSR: rowptr [N+1] int64, col int32
 * (strictly ascending inside a row), val fp32; every stage that makes one comes as a _count call, which writes the
 * output's rowptr (rowptr[N] = its number of entries, which the caller reads back to allocate col and val), and a _fill
 * call.  The caller owns all memory and runs the stages in this order (ieee_amd/rerank.py::_gnn_sparse):
 *   rank, S [N][k1] from ieee_rank_topk_merge over column slabs of -X_u X_u^T (metric 2), as ieee_gnn_rerank's;
 *   B = the CSR view of rank (rowptr[i] = i k1, col = rank, val = 1: the one input whose rows need not be sorted);
 *   M0 = symmetrise(B, transpose(B));  M1 = propagate(M0);  M0' = symmetrise(M1, transpose(M1), norms of M1);
 *   R = propagate(M0'), with its row norms;  per gallery range [g0, g1): T = transpose of rows Q+g0 .. Q+g1-1 of R,
 *   then ieee_gnn_sparse_cosine.  k2 = 1: R = symmetrise(B, an empty transposed side), i.e. B with sorted rows.
 * No floating-point atomics: every sum has a fixed order and two calls give the same bits.  Everything on `stream`, no
 * host sync.  Bad arguments (null pointers, the bounds below) give IEEE_ERR_BAD_ARG before any launch.
 *
 * scratch: the work rows of symmetrise and propagate, ieee_gnn_sparse_scratch_bytes(Q, G, k1, k2) bytes (at most 512
 * rows of N floats and N bits), ALL ZERO before the first call; every call leaves it all zero again.  The function
 * checks the whole call's bounds, those of ieee_gnn_rerank: Q, G >= 1 and < 2^30, 1 <= k2 <= k1 <= min(1024, N); it
 * returns -1 and sets the error text otherwise. */
int64_t ieee_gnn_sparse_scratch_bytes(int64_t Q, int64_t G, int64_t k1, int64_t k2);
/* Transpose of rows [r0, r1) of a CSR matrix with N rows and N columns: list c = tptr[c] .. tptr[c+1] holds, for
 * every entry (r, c, v) of those rows, trow = r and tval = v / max(norm[r], 1e-12) (v itself when norm is null), in no
 * particular order (the rows of one list are distinct).  tptr [N+1] int64, cursor [N] int32 (work), trow / tval with
 * room for cap entries: rowptr[r1] - rowptr[r0] are written, and nothing beyond cap. */
int ieee_gnn_sparse_transpose(const int64_t* rowptr, const int32_t* col, const float* val, const float* norm, int64_t N,
                              int64_t r0, int64_t r1, int32_t* cursor, int64_t* tptr, int32_t* trow, float* tval,
                              int64_t cap, void* stream);
/* out = A / n + (A / n)^T, n_r = max(norm[r], 1e-12) (n = 1 when norm is null): row i is the union of row i of A,
 * scaled, and list i of the (already scaled) transpose from ieee_gnn_sparse_transpose; a column both sides hold gets
 * their sum.  The rows of A need not be sorted; the output's are.  out_norm (may be null) receives the output's row
 * norms.  Nothing is written beyond cap entries. */
int ieee_gnn_sparse_symmetrise_count(const int64_t* rowptr, const int32_t* col, const int64_t* tptr, const int32_t* trow,
                                     int64_t N, void* scratch, int64_t scratch_bytes, int64_t* out_rowptr, void* stream);
int ieee_gnn_sparse_symmetrise_fill(const int64_t* rowptr, const int32_t* col, const float* val, const float* norm,
                                    const int64_t* tptr, const int32_t* trow, const float* tval, int64_t N, void* scratch,
                                    int64_t scratch_bytes, const int64_t* out_rowptr, int32_t* out_col, float* out_val,
                                    float* out_norm, int64_t cap, void* stream);
/* out[i] = sum_{j < k2} S[i][j]^2 A[rank[i][j]], per column in ascending j with one fma per term (the dense
 * gnn_propagate arithmetic without its zero terms); out_norm[i] = |out[i]| (not clamped).  Source rows of any length. */
int ieee_gnn_sparse_propagate_count(const int64_t* rowptr, const int32_t* col, const int32_t* rank, int64_t N, int64_t k1,
                                    int64_t k2, void* scratch, int64_t scratch_bytes, int64_t* out_rowptr, void* stream);
int ieee_gnn_sparse_propagate_fill(const int64_t* rowptr, const int32_t* col, const float* val, const int32_t* rank,
                                   const float* S, int64_t N, int64_t k1, int64_t k2, void* scratch, int64_t scratch_bytes,
                                   const int64_t* out_rowptr, int32_t* out_col, float* out_val, float* out_norm,
                                   int64_t cap, void* stream);
/* out[q][g - g0] = 1 - <R_q, R_{Q+g}> / (max(norm[q], 1e-12) max(norm[Q+g], 1e-12)) for q < Q, g0 <= g < g1: `out`
 * points at the range's first column, row stride ldo >= g1 - g0.  (tptr, trow, tval) is the transpose of rows Q+g0 ..
 * Q+g1-1 of R with norm null.  The sum of one pair runs over the shared columns in ascending order whatever the range,
 * so the bits do not depend on how the gallery is cut; a pair without a shared column, and a zero row, give exactly 1. */
int ieee_gnn_sparse_cosine(const int64_t* rowptr, const int32_t* col, const float* val, const float* norm,
                           const int64_t* tptr, const int32_t* trow, const float* tval, int64_t Q, int64_t G, int64_t g0,
                           int64_t g1, float* out, int64_t ldo, void* stream);

/* ---- query expansion / database augmentation (ieee_amd/expansion.py; not in the reference) ----------------------- */
/* out[i] = 1 / max(|x_i|, 1e-12) for the rows of x [rows][d] fp32, contiguous, 16-byte aligned, d % 4 == 0: the row
 * norm pass of ieee_sqeuclid_distmat with metric 1 (the same kernel, the same bits), F.normalize's clamp.  A zero row
 * gives 1e12.  Anything else is IEEE_ERR_BAD_ARG before any launch; rows == 0 is a no-op. */
int ieee_row_rinv(const float* x, int64_t rows, int64_t d, float* out, void* stream);
/* The weights of neighbour lists as ieee_rank_topk_merge leaves them: for each of `count` places
 *   idx < 0 (a padded place): w = 0;  alpha == 0: w = 1;  else w = s^alpha with s = fmaxf(1 - dist, 0) in fp32, formed by
 *   alpha - 1 multiplications left to right (a NaN distance gives s = 0, as +inf does).
 * 0 <= alpha <= 64, else IEEE_ERR_BAD_ARG before any launch; count == 0 is a no-op. */
int ieee_expand_weights(const int32_t* idx, const float* dist, int64_t count, int64_t alpha, float* w, void* stream);
/* out[i] = [self_rinv[i] * self_rows[i] +] sum_j (w[i][j] * rinv[idx[i][j]]) * src[idx[i][j]], i < n, j < k ascending,
 * then with normalize != 0 out[i] *= 1 / max(|out[i]|, 1e-12) (a zero sum stays a zero row).  All fp32 on the device:
 *   src [n_src][d] row stride ld_src;  rinv [n_src] or null (then the coefficient is w alone);
 *   idx int32 / w fp32 [n][k], row stride ld_list;  self_rows [n][d] row stride ld_self or null, self_rinv [n] or
 *   null (then the self row enters unscaled);  out [n][d] row stride ld_out.
 * An index outside [0, n_src) -- -1 is the padding of the lists -- adds nothing and nothing is read through it;
 * duplicates are summed as often as they occur.  Per output element the sum is ONE fp32 chain: the self term (a
 * product), then one fma per kept entry in list order; the squares are summed in float64, per thread ascending and then
 * in block_tree_sum's association.  One workgroup per row, no atomics, no workspace, no host sync: the same bits on
 * every call, however the rows are divided over calls and whether the 16-byte or the scalar loads are used (16-byte:
 * d % 4 == 0 and src, self_rows, out 16-byte aligned with strides that are multiples of 4).  Up to d = 4096 a row stays
 * in registers; beyond, it is stored unscaled and scaled in a second pass over out.
 * 1 <= k <= 1024, d >= 1, strides at least the row, out disjoint from src and from self_rows, else IEEE_ERR_BAD_ARG
 * before any launch; n == 0 is a no-op, n_src == 0 (src may be null) leaves the self term. */
int ieee_neighbour_sum(const float* src, int64_t ld_src, int64_t n_src, const float* rinv, const int32_t* idx,
                       const float* w, int64_t ld_list, int64_t n, int64_t k, const float* self_rows,
                       const float* self_rinv, int64_t ld_self, int64_t d, int normalize, float* out, int64_t ld_out,
                       void* stream);

/* ---- DBSCAN clustering (ieee_amd/cluster.py; not in the reference) --------------------------------- */
/* The neighbour relation of N points, R(i, j) iff i == j or D[i][j] <= thr or D[j][i] <= thr (fp32 compares of the
 * stored values, a NaN is never a neighbour), as two CSR structures; D arrives buffer by buffer and nothing of size
 * N x N is allocated.  Row pointers are int64 [N + 1], columns int32.  The caller owns all memory, forms the exclusive
 * sums between a _count and its _fill, and runs the stages in the order below; everything on `stream`, no host sync.
 * 1 <= N < 2^31 - 1, else IEEE_ERR_BAD_ARG before any launch, as for null pointers and ranges outside the N points.
 *
 * dist: one [rows][cols] fp32 buffer, row stride ldd >= cols, holding D[row0 + r][col0 + c].  _count adds to
 * deg[row0 + r] (zero before the first buffer) the columns with dist <= thr, the point's own column skipped whatever
 * it holds.  _fill writes their indices col0 + c, ascending, to col[rowptr[row] + cursor[row] ...] and advances
 * cursor[row] (zero before the first buffer): with the buffers of a row visited in ascending column order every list
 * of A is sorted.  Nothing is written at or beyond rowptr[row + 1] or cap.  One workgroup per buffer row, no atomics.
 * 16-byte loads where dist is 16-byte aligned and ldd % 4 == 0, scalar loads otherwise: the same lists. */
int ieee_cluster_eps_count(const float* dist, int64_t ldd, int64_t rows, int64_t cols, int64_t row0, int64_t col0,
                           int64_t N, float thr, int64_t* deg, void* stream);
int ieee_cluster_eps_fill(const float* dist, int64_t ldd, int64_t rows, int64_t cols, int64_t row0, int64_t col0,
                          int64_t N, float thr, const int64_t* rowptr, int32_t* cursor, int32_t* col, int64_t cap,
                          void* stream);
/* The OR closure X: for every edge i -> j of A (sorted lists) without an edge j -> i, list j of X gains i.  _count adds
 * to cnt[j] (zero before); _fill draws slots from cursor[j] (int32, zero before), so the order inside a list of X is
 * arbitrary; nothing is written at or beyond xptr[j + 1] or cap.  A symmetric D gives no entry. */
int ieee_cluster_mirror_count(const int64_t* rowptr, const int32_t* col, int64_t N, int64_t* cnt, void* stream);
int ieee_cluster_mirror_fill(const int64_t* rowptr, const int32_t* col, int64_t N, const int64_t* xptr, int32_t* cursor,
                             int32_t* xcol, int64_t cap, void* stream);
/* core[u] = (1 + |A_u| + |X_u| >= min_samples), one byte each; f[u] = u, the first parent array.  min_samples >= 1. */
int ieee_cluster_core(const int64_t* rowptr, const int64_t* xptr, int64_t N, int64_t min_samples, uint8_t* core,
                      int32_t* f, void* stream);
/* One hook-and-shortcut round over the core points: fnext = f (a copy), then for every core u and each of its core
 * neighbours v in A_u and X_u, g = f[f[v]] lowers fnext[f[u]] and fnext[u], and f[f[u]] lowers fnext[u] (integer
 * atomicMin).  Only f is read for a decision, so fnext is a function of f.  *changed (device int32, cleared by the
 * call) ends as 1 iff fnext != f.  Repeat with the arrays swapped until it stays 0: then f[u] is the smallest core
 * index of u's component for every core u.  f and fnext must be different arrays. */
int ieee_cluster_cc_round(const int64_t* rowptr, const int32_t* col, const int64_t* xptr, const int32_t* xcol,
                          const uint8_t* core, int64_t N, const int32_t* f, int32_t* fnext, int32_t* changed,
                          void* stream);
/* root[u] = 1 where u is core and f[u] == u, else 0 (int64: its exclusive sum is `number`, the cluster of root u). */
int ieee_cluster_roots(const uint8_t* core, const int32_t* f, int64_t N, int64_t* root, void* stream);
/* labels[u] = number[f[u]] for a core point; otherwise the smallest number[f[v]] over the core entries v of A_u and
 * X_u, or -1 where there is none. */
int ieee_cluster_labels(const int64_t* rowptr, const int32_t* col, const int64_t* xptr, const int32_t* xcol,
                        const uint8_t* core, const int32_t* f, const int64_t* number, int64_t N, int64_t* labels,
                        void* stream);

/* ---- descriptor t-SNE (torchreid/engine/engine.py:463-490, showPointMultiModal) ---------------------------------- */
/* Exact (dense, O(n^2)) t-SNE in 2 output dimensions, Student-t degree of freedom 1, what the reference gets from
 * sklearn.manifold.TSNE(n_components=2).  `batch` independent problems of the same n run per call, on a grid axis (the
 * three modalities are batch = 3).  Caller-owned memory, everything on `stream`, no host sync, no atomics, no graph
 * capture; every sum has a fixed order, so two calls give the same bits.  Bounds, checked before anything is launched
 * (IEEE_ERR_BAD_ARG, the error text names the function): 4 <= n <= 12288 (a distance row stays in LDS during the
 * search; P for batch = 3 is then 1.7 GiB and the workspace 21 MiB: under 2 GiB together), 1 <= batch <= 65535,
 * 0 < perplexity < n, ldd >= n, ldp >= n with ldp % 4 == 0 and P 16-byte aligned, Y 8-byte aligned, work_bytes >=
 * ieee_tsne_workspace_bytes(n, batch) (-1 and the error text for n or batch out of range; one size serves both calls). */
int64_t ieee_tsne_workspace_bytes(int64_t n, int64_t batch);
/* dist [batch][n][ldd] fp32 squared Euclidean distances (what ieee_sqeuclid_distmat(x, x) writes; tiny negatives are
 * fine) -> the joint matrix P [batch][n][ldp] fp32 and beta [batch][n] fp32.  Per row i, with d'_j = dist[i][j] -
 * min_{k != i} dist[i][k] (the shift changes neither the row nor its entropy and keeps exp from underflowing on
 * distances of 1e3..1e5; the diagonal takes no part): sklearn's _binary_search_perplexity -- beta = 1; H = log S +
 * beta sum_j d'_j e_j / S with e_j = exp(-beta d'_j), S = sum_j e_j; done when |H - log(perplexity)| <= 1e-5 or after
 * 100 steps; else beta moves to the middle of its bracket, doubling or halving while that side has no bound yet.
 * beta d'_j is formed in double and rounded once; sums are fp32.  p_{j|i} = e_j / S for the beta returned, and
 * P_ij = (p_{j|i} + p_{i|j}) / (2n): bitwise symmetric, diagonal 0, columns n..ldp-1 zero. */
int ieee_tsne_affinities(const float* dist, int64_t ldd, int64_t n, int64_t batch, double perplexity, float* P,
                         int64_t ldp, float* beta, void* work, int64_t work_bytes, void* stream);
/* Iterations iter0 .. iter0 + n_iter - 1 of sklearn's _gradient_descent schedule, all enqueued by the one call (two
 * launches each).  Y, update, gains [batch][n][2] fp32 are read and written, so a run can be resumed or stepped (start
 * with update = 0, gains = 1).  Per iteration, with w_ij = 1 / (1 + |y_i - y_j|^2) for i != j and Z = sum_{i != j} w_ij:
 *   g_i = 4 (alpha sum_j P_ij w_ij (y_i - y_j) - (sum_j w_ij^2 (y_i - y_j)) / Z)
 *   gains += 0.2 where update * g < 0, else gains *= 0.8; gains = max(gains, 0.01)
 *   update = momentum * update - learning_rate * (gains * g);  Y += update
 * alpha = early_exaggeration and momentum = 0.5 for iterations below exaggeration_iters, then 1 and 0.8.
 * history [batch][n_iter][2] or NULL: (KL = sum P log P + sum P log(1 + |y_i - y_j|^2) + (sum P) log Z of the plain P
 * at the iteration's Y before the update, zero entries of P contributing 0; the 2-norm of g).  There is NO early
 * stopping: sklearn's min_grad_norm and n_iter_without_progress checks would need a host read every 50 iterations. */
int ieee_tsne_run(const float* P, int64_t ldp, int64_t n, int64_t batch, float* Y, float* update, float* gains,
                  int64_t iter0, int64_t n_iter, int64_t exaggeration_iters, double early_exaggeration,
                  double learning_rate, float* history, void* work, int64_t work_bytes, void* stream);
/* Where ieee_tsne_run leaves its sums, for inspection after a call: fields[6] = {slabs (512 columns each), byte offset
 * of the slab partials [batch][slabs][6][n] fp32, byte offset of the per-row sums [batch][6][n] fp32 of the LAST
 * iteration (sum_j P w dx, sum_j P w dy, sum_j w^2 dx, sum_j w^2 dy, sum_j w, sum_j P log(1 + d^2); the last one only with a
 * history), byte offset of [batch][2][n] fp32 (sum_j P log P, sum_j P; only with a history), byte offset of
 * [batch][8] fp32 {Z, sum P log(1 + d^2), sum P log P, sum P, |g|^2, -, -, -}, 6}. */
int ieee_tsne_layout(int64_t n, int64_t batch, int64_t* fields);

/* ---- input pipeline ------------------------------------------ */
/* The reference's per-image chain Resize((Ho,Wo)) -> RandomHorizontalFlip -> ToTensor -> Normalize
 * (torchreid/data/transforms.py:233-326; dataset.py:335-351) for N decoded uint8 images of ONE source size:
 * src [N][Hs][Ws][3] (device) -> dst [N][3][Ho][Wo] fp32 (device).  The resize is Pillow's two-pass 8-bit bilinear
 * resampler, bit-exact: bounds_* [out][2] = (first source index, count), kk_* [out][ksize] = 22-bit fixed-point
 * weights, both computed on the host as Pillow does (ieee_amd/data/transforms.py) and resident on the device; a
 * table is NULL iff that axis keeps its size.  tmp: [N][tmp_rows][Wo][3] bytes for the horizontal pass, which only
 * covers source rows ybox_first .. ybox_first+tmp_rows (what the vertical pass reads).  flip [N] bytes or NULL;
 * mean3 / std3: HOST pointers to 3 floats. */
int ieee_resize_flip_normalize(const uint8_t* src, float* dst, uint8_t* tmp, int64_t N, int64_t Hs, int64_t Ws,
                               int64_t Ho, int64_t Wo, const int32_t* bounds_h, const int32_t* kk_h, int64_t ksize_h,
                               const int32_t* bounds_v, const int32_t* kk_v, int64_t ksize_v, int64_t ybox_first,
                               int64_t tmp_rows, const uint8_t* flip, const float* mean3, const float* std3,
                               void* stream);

/* The same chain with the reference's other train augmentations (transforms.py:12-106, 283-311), in its order:
 *   Resize -> flip -> random crop (Random2DTranslation) -> colour jitter (brightness, contrast) -> ToTensor -> Normalize
 *   -> random erase.
 * Arguments up to tmp_rows as above.  plan: DEVICE int32 [N][12], one row per image, drawn on the host
 * (ieee_amd/data/transforms.py, AugmentPlan.pack): {flip, crop flag, x1, y1, jitter order (0: brightness first),
 * bits of the brightness factor (float), bits of the contrast factor, erase r0, c0, h, w (h = 0: none), 0}; the last
 * word must arrive 0 and receives the image's integer sum of L (the contrast stage's grey level comes from it).
 * stages: bit 0 flip, 1 crop, 2 jitter, 3 erase; a stage whose bit is clear costs nothing and its plan words are ignored.
 * work: work_bytes >= (crop ? 3 : jitter ? 1 : 0) * N*Ho*Wo*3 bytes of device scratch (the flipped uint8 stage image,
 * the crop's horizontal intermediate, the cropped image), NULL when neither is on.  The crop enlarges the Ho x Wo stage
 * image to Hbig x Wbig (Pillow bilinear; tables big_* as above for Wo -> Wbig and Ho -> Hbig, both strictly larger) and
 * keeps the Ho x Wo window at (x1, y1); only that window is computed.  Every pixel step is Pillow's 8-bit arithmetic
 * (ImageEnhance / Image.blend for the jitter), the float expression is ieee_resize_flip_normalize's, the erase rectangle
 * is written as mean3[c].  Launches: 2 + (crop or jitter) + 2 * crop with a horizontal resize pass (5 with everything on),
 * one less without; no host synchronisation, no allocation.  launches: HOST int, receives that count, or NULL. */
int ieee_augment_normalize(const uint8_t* src, float* dst, uint8_t* tmp, int64_t N, int64_t Hs, int64_t Ws, int64_t Ho,
                           int64_t Wo, const int32_t* bounds_h, const int32_t* kk_h, int64_t ksize_h,
                           const int32_t* bounds_v, const int32_t* kk_v, int64_t ksize_v, int64_t ybox_first,
                           int64_t tmp_rows, int32_t* plan, int stages, uint8_t* work, int64_t work_bytes, int64_t Hbig,
                           int64_t Wbig, const int32_t* big_bounds_h, const int32_t* big_kk_h, int64_t big_ksize_h,
                           const int32_t* big_bounds_v, const int32_t* big_kk_v, int64_t big_ksize_v,
                           const float* mean3, const float* std3, int* launches, void* stream);

/* The resize chain above (no augmentation) for a RAGGED batch: N decoded uint8 RGB images, each with its own size, in ONE
 * launch and without host tables.  src: device bytes, src_bytes long; image i is the tightly packed [Hs_i][Ws_i][3] block at
 * byte offsets[i] (gaps between images are allowed); sizes [N][2] int32 = (Hs_i, Ws_i); flip [N] bytes or NULL: all three
 * DEVICE arrays.  host_offsets / host_sizes: HOST copies of the same two tables -- every image is checked against
 * 1 <= side <= 4096 and against src_bytes before anything is launched (a device table that disagrees with its host copy
 * leaves that image's output unwritten; nothing is read or written out of bounds).  dst [N][3][Ho][Wo] fp32; mean3 / std3:
 * HOST pointers to 3 floats.  Per image the arithmetic is ieee_resize_flip_normalize's, bit for bit: Pillow's two-pass
 * 8-bit bilinear resampler, horizontal pass first and only over the source rows the vertical pass reads, the intermediate
 * rounded to 8 bits, then flip, / 255, (x - mean) / std; an axis that keeps its size gets identity weight rows, which
 * return what skipping the pass returns.  Pillow's coefficients (precompute_coeffs + normalize_coeffs_8bpc: fp64, the
 * scale from the float32 of the size, weights trunc(+-0.5 + k * 2^22)) are computed on the device by every workgroup for
 * the rows and columns it needs.  One workgroup per (image, band of up to 16 output rows) keeps the band's horizontal
 * intermediate in LDS (at most 64 KiB with the tables; the band height is halved until one output row's window fits).
 * Returns IEEE_ERR_UNSUPPORTED before any launch for a source side above 4096 or tables that do not fit (a 1-row band of a
 * very wide output from very large sources), IEEE_ERR_BAD_ARG for anything malformed; N = 0 is IEEE_OK and launches
 * nothing.  1 launch whatever N and the sizes are; no workspace, no allocation, no host synchronisation.
 * launches: HOST int, receives the launch count, or NULL. */
int ieee_resize_normalize_ragged(const uint8_t* src, int64_t src_bytes, const int64_t* offsets, const int32_t* sizes,
                                 const uint8_t* flip, const int64_t* host_offsets, const int32_t* host_sizes, float* dst,
                                 int64_t N, int64_t Ho, int64_t Wo, const float* mean3, const float* std3, int* launches,
                                 void* stream);
/* The device coefficient function of ieee_resize_normalize_ragged run over a whole axis: bounds [out_size][2] int32 =
 * (first source index, count) and kk [out_size][ksize] int32 (22-bit fixed point, zero past count), both DEVICE; what
 * _axis_tables of ieee_amd/data/transforms.py computes on the host.  ksize must be ieee_resample_ksize(in_size, out_size)
 * (host only; 0 for sizes outside 1 .. 4096).  1 launch. */
int ieee_resample_ksize(int64_t in_size, int64_t out_size);
int ieee_resample_coeffs(int64_t in_size, int64_t out_size, int32_t* bounds, int32_t* kk, int64_t ksize, void* stream);

/* ---- whole-network executor --------------------------------------------------- */
/* One handle = IEEE3modalPart (ieee3modalPart.py:286-523) for a fixed batch / image size / dtype.
 * The caller owns three flat fp32 buffers laid out like the reference's state_dict: parameters,
 * their gradients, and BN running statistics.  ieee_net_slot_name() enumerates the tensor names the
 * executor needs (e.g. "backbone.0.layer1.0.conv1.weight"); ieee_net_bind() receives, in that order,
 * each tensor's element offset inside `params` (running_mean/var: inside `buffers`).
 * forward : x_* fp32 NCHW [B,3,H,W].  training: logits [18][B][C] (R0..5,N0..5,T0..5) and
 *           feats [3][B][768] = F.normalize(fc_{R,N,T}_all); eval: feats = fc_all [B][2304] (T,R,N).
 * backward: dlogits / dfeats in the same layouts; every parameter gradient is OVERWRITTEN in `grads`
 *           (REM.conv_query gets exact zeros, REM.conv_value and unused branches are not touched).
 * Streams: the dependent chain of a call (forward; dgrad / BatchNorm backward) is enqueued on the caller's `stream`.
 * The executor also owns two internal non-blocking streams per handle, created on first use: a low-priority SIDE
 * stream (every weight-gradient kernel + its slab reduction, and the packing of the layer3 / layer4 / CIM operands
 * during a training forward) and a BRANCH stream (the downsample branch of the first block of each stage).  They
 * are ordered against `stream` with events in both directions, and they are JOINED into `stream` before
 * ieee_net_forward, ieee_net_backward and ieee_net_backward_part return -- after those calls, synchronising (or
 * enqueuing behind) `stream` covers everything the call launched.  The one exception is
 * ieee_net_backward_part_async: weight gradients of the part may still run on the side stream when it returns; join
 * them with ieee_net_side_wait or ieee_net_sync_streams before reading gradients, destroying `stream` or the
 * workspace, or stepping the optimizer.  No call synchronises the host (ieee_net_profile(.., 0, ..) aside).
 * The workspace (ieee_net_workspace_bytes) keeps the activations between forward and backward. */
int ieee_net_create(int64_t batch, int64_t height, int64_t width, int64_t num_classes, int dtype,
                    int interaction, int attention, int using_rem, void** handle);
int ieee_net_destroy(void* handle);
int64_t ieee_net_num_slots(void* handle);
const char* ieee_net_slot_name(void* handle, int64_t i);
int64_t ieee_net_workspace_bytes(void* handle);
int ieee_net_bind(void* handle, float* params, float* grads, float* buffers, const int64_t* offsets,
                  int64_t num_offsets);
int ieee_net_forward(void* handle, void* workspace, const float* x_rgb, const float* x_ni, const float* x_ti,
                     int training, float* logits, float* feats, void* stream);
int ieee_net_backward(void* handle, void* workspace, const float* dlogits, const float* dfeats, void* stream);
/* the same backward in 5 consecutive parts (0: head + CIM, 1: layer4, 2: layer3, 3: layer2, 4: layer1 + stem; call
 * them in this order): after part p all gradients of that part are final, so a data-parallel caller overlaps
 * their all-reduce with the remaining parts (ieee_amd/engine.py) */
int ieee_net_backward_part(void* handle, void* workspace, const float* dlogits, const float* dfeats, int part,
                           void* stream);
/* Same, without blocking the launch stream at the end of the part: the part's weight gradients may still be running
 * on the executor's side stream when the call returns.  ieee_net_side_wait(waiting_stream, 0) makes ANOTHER stream
 * (e.g. the one a collective is issued from) wait for every weight gradient issued so far;
 * ieee_net_side_wait(launch_stream, 1) is the final join that must precede the optimizer step (it also retires
 * the executor's buffer-reuse bookkeeping, so pass the stream the parts were launched on). */
int ieee_net_backward_part_async(void* handle, void* workspace, const float* dlogits, const float* dfeats, int part,
                                 void* stream);
int ieee_net_side_wait(void* handle, void* workspace, void* waiting_stream, int is_launch_stream);
/* Make `stream` wait for everything the executor has enqueued on its internal streams so far (side + branch), without
 * knowing about them: after this, hipStreamSynchronize(stream) -- or any work enqueued on `stream` -- is ordered
 * behind every kernel of the preceding ieee_net_* calls.  A C caller that uses the _async parts calls this (on the
 * launch stream) where the Python engine calls ieee_net_side_wait(launch_stream, 1); it is a no-op when nothing is
 * pending.  Does not block the host. */
int ieee_net_sync_streams(void* handle, void* stream);
/* Frozen children (Engine.two_stepped_transfer_learning -> open_specified_layers, torchreid/utils/torchtools.py:183-221: the
 * children outside `open_layers` are put in eval() mode and stop requiring gradients for the first fixbase_epoch epochs).
 * mask: bit 0 backbone, 1 convOne, 2 convAvgRest, 3 reduce_layer, 4 fc_R, 5 fc_N, 6 fc_T (the children that own a
 * BatchNorm).  A frozen child's BatchNorms use their running statistics in a TRAINING forward, do not update them, and
 * the backward treats them as the fixed affine maps they then are (ieee_bn2d_bwd_frozen); gradients still flow through a
 * frozen child to whatever trains below it.  The caller keeps frozen parameters out of the optimizer step. */
#define IEEE_FROZEN_BACKBONE 1
#define IEEE_FROZEN_CONV_ONE 2
#define IEEE_FROZEN_CONV_REST 4
#define IEEE_FROZEN_REDUCE 8
#define IEEE_FROZEN_FC_R 16
#define IEEE_FROZEN_FC_N 32
#define IEEE_FROZEN_FC_T 64
int ieee_net_set_frozen(void* handle, int mask);
/* Range guard of the fixed-point BatchNorm totals (bf16 training; see ieee_conv_next_bn_totals): out4 receives, and the call
 * CLEARS, the four report words the kernels of the MOST RECENT training step have set -- [0] a forward tile sum was clamped
 * to its share of the int64 range (or was NaN), [1] a backward one, [2] / [3] a forward / backward total beyond half the
 * range.  The words are device memory at the head of the executor's totals region, zeroed by every training forward (round 6:
 * they were host-mapped words); this call is a blocking 16-byte copy -- synchronise with the step first.  All zero = the
 * statistics of that step are the partial-sum path's up to the last bit of a float sum.  Non-zero: they are NOT what torch's
 * fp32 batch_norm (torchreid/models/resnet.py:164-184) would have computed; a step whose words [0] / [1] are set is skipped by
 * ieee_sgd_nesterov_step_ex(skip_flags) / ieee_guard_buffers, and the engine switches to the partial-sum path. */
int ieee_net_bn_overflow(void* handle, int* out4);
/* byte offset of those four int32 words inside the workspace (they are device memory, zeroed by every training forward): the
 * engine copies them to the host with the step's summary, the optimizer takes them as `skip_flags` */
int64_t ieee_net_bn_flags_offset(void* handle);
/* on = 0: from the next forward on, every BatchNorm of this executor takes the per-tile partial-sum path (ieee_bn2d_fwd /
 * ieee_bn2d_bwd: fp32 sums without a range, as the reference's fp32 nn.BatchNorm2d, torchreid/models/resnet.py:151,164-184;
 * +104 finalize launches per step); on = 1: fixed-point totals again where IEEE_BN_TOTALS_TILES allows.  What the engine does
 * when ieee_net_bn_overflow reports a clamped tile: degrade, warn, keep training (IEEE_BN_STRICT=1: raise instead). */
int ieee_net_set_bn_totals(void* handle, int on);
/* shadow_bf16: a bf16 buffer with one element per element of the bound parameter buffer, element i = bf16(params[i]), that the
 * CALLER keeps current (ieee_sgd_nesterov_step_ex, or a plain conversion after any other write) -- every bf16 TRAINING
 * forward issued while it is set reads the forward operands of the 1x1 convolutions from it instead of packing them.  NULL
 * (the default): every operand is packed from the fp32 parameters at the start of the forward.  Inference is not affected. */
int ieee_net_set_shadow(void* handle, const void* shadow_bf16);
/* Inference cache: after an eval-mode ieee_net_forward the workspace holds the packed weights and every BatchNorm's
 * scale / shift; the next eval forward on the same workspace reuses them (no packing launch, no finalize launches)
 * unless ieee_net_eval_cache(handle, 0) was called in between.  The CALLER must call it whenever parameters or
 * running statistics may have changed outside ieee_net_forward(training = 1) (optimizer steps, state loading, ...). */
int ieee_net_eval_cache(void* handle, int keep);
/* measurement: enable=1 starts recording a HIP event pair around every conv launch of subsequent forward/backward
 * calls with ALL work on one ordered stream (the serialized pass: what each launch takes alone); enable=2 times the
 * launches with the executor's own streams left on -- every forward / dgrad launch carries its pair as its own start /
 * stop signals (ieee_conv_profile_events: nothing added to the queue), weight-gradient calls get an event record on each
 * side, on the side stream they run on: what a launch takes INSIDE the two-stream step; enable=0 stops, synchronises the device and returns
 * out6 = {ms, algorithmic FLOPs, launches} for [0] forward+dgrad (conv_gather / conv3x3_patch / stem_conv kernels) and
 * [1] wgrad (conv_wgrad / conv3x3_wgrad_patch / stem_wgrad kernels + their slab reductions) */
int ieee_net_profile(void* handle, int enable, double* out6);
/* measurement: the next conv forward / dgrad launch issued by the calling thread signals `start` when it begins and `stop`
 * when it ends (hipEvent_t with timing enabled; NULL, NULL cancels): the kernel's own duration by the GPU's timestamps,
 * without an event record in the queue.  ieee_net_profile(.., 2, ..) times the forward / dgrad family this way. */
int ieee_conv_profile_events(void* start, void* stop);
/* debugging / parity tests: location of a named intermediate inside the workspace */
int ieee_net_tensor(void* handle, const char* name, int64_t* byte_offset, int64_t* numel, int* dtype);
/* parity tests of the backward (what autograd keeps implicit in the reference, ieee3modalPart.py:439-523 under
 * loss.backward()): while `buffer` (device memory, `bytes` long) is set, ieee_net_backward* copies every gradient
 * tensor it produces into it before the buffer that held it is reused -- "<unit>.dy" (gradient of the conv output =
 * output of that unit's BatchNorm backward), "<unit>.dx" (what the unit's dgrad wrote: for a block's conv1 the masked
 * block-input gradient, residual branch added), "<unit>.g" for block-output units (dout * [out > 0]); a stride-2
 * downsample branch that returns its gradient compact taps "<unit>.dx_compact".  <unit> = the conv's state_dict
 * prefix, modality as {m}: "backbone.{m}.layer1.0.conv1".  buffer = NULL switches the taps off.
 * ieee_net_debug_tap: byte offset of a tap inside the buffer (after the backward that wrote it). */
int ieee_net_debug_taps(void* handle, void* buffer, int64_t bytes);
int ieee_net_debug_tap(void* handle, const char* name, int64_t* byte_offset, int64_t* numel, int* dtype);

#ifdef __cplusplus
}
#endif
#endif /* IEEE_AMD_H */
