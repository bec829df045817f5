// CUHK03 single-gallery-shot CMC and mAP, on the device.
// Reference: torchreid/metrics/rank.py:24-100 (eval_cuhk03, with this fork's time-id filter).  The reference draws
// one gallery image per identity at random, ten times per query, and averages the CMC curves it reads off the drawn
// lists: a Monte-Carlo estimate.  This file computes what it estimates.  For one query, with the gallery ordered on
// (distance, gallery index) and the entries of the query's identity AND key (camera, time id) dropped:
//   - the drawn true match is uniform over the kept true matches T;
//   - an other identity j with n_j images, c_j(t) of them before true match t, is drawn before t with probability
//     p = c_j(t) / n_j, independently of the others;
//   - so the rank of the drawn true match is a sum of independent Bernoulli variables and
//       cmc[r] = (1 / |T|) * sum_t P(sum_j B_j(t) <= r)
//     is a Poisson-binomial distribution function, built by pmf'[k] = pmf[k] * (1 - p) + pmf[k - 1] * p over the
//     identities in ascending-pid order, in float64, truncated at max_rank terms.
// AP is that of the kept list (rank.py:86-90), as in the Market protocol but with the three-way filter; the ranks it
// needs are sums of the same counts.  Nothing is sorted but the true matches, there are no atomics on floating-point
// data, and every sum has one fixed order: two calls give the same bits.
#include "rank_common.h"

namespace ieee {

constexpr int CK_THREADS = 256;
constexpr int CK_TCAP = 512;        // true matches per batch, at most
constexpr int CK_STATES = 2048;     // pmf states (true match x rank) per batch, double-buffered in LDS
constexpr int CK_SLOTS = 64;        // identities counted per round, at most
constexpr int CK_UNR = 8;           // images per thread in flight while counting
constexpr int CK_CNT = 8 * (CK_TCAP + 1);   // words of their histograms: a full batch still leaves 8 per round
constexpr int CK_MAX_RANK = 1024;

static_assert(CK_THREADS == 256, "block_scan_excl and block_tree_sum are written for 256 threads");

// this protocol orders on the folded order, a stable argsort's (rank_common.h says why)
__device__ __forceinline__ uint64_t ck_key(float d, uint32_t idx) { return order_key(order_word_folded(d), idx); }

// ---- the gallery grouped by identity, once per call: sidx = gallery indices ordered on (pid, index), spid their pids.
// The position of entry j is the number of entries before it in that order, counted against LDS tiles of the pids:
// quadratic, but 19 732^2 compares are some tens of microseconds of the device, and there is no sort to tune.  Workgroup
// (x, y) counts entries [x * 256, +256) against the y-th span of the gallery and adds its share to pos (integers: any
// order of the adds gives the same sum); pos is zero on entry.
__global__ __launch_bounds__(CK_THREADS) void cuhk03_order_kernel(const int32_t* __restrict__ g_pids, int num_g, int span,
                                                                  int32_t* __restrict__ pos) {
  __shared__ __attribute__((aligned(16))) int32_t tile[1024];
  const int t = threadIdx.x, j = blockIdx.x * CK_THREADS + t;
  const int32_t mine = j < num_g ? g_pids[j] : 0;
  const int64_t first = (int64_t)blockIdx.y * span;
  const int last = (int)min((int64_t)num_g, first + span);
  int count = 0;
  auto before = [&](int32_t p, int idx) { return (p < mine || (p == mine && idx < j)) ? 1 : 0; };
  for (int base = (int)first; base < last; base += 1024) {         // span is a multiple of 1024
    // past the end: the largest pid under an index beyond every j, which is before nothing
    for (int i = t; i < 1024; i += CK_THREADS) tile[i] = base + i < num_g ? g_pids[base + i] : 0x7fffffff;
    __syncthreads();
    const int n = min(1024, num_g - base);
    for (int i = 0; i < n; i += 4) {
      const int4 p = *(const int4*)&tile[i];      // one address per step: an LDS broadcast
      count += before(p.x, base + i) + before(p.y, base + i + 1) + before(p.z, base + i + 2) + before(p.w, base + i + 3);
    }
    __syncthreads();
  }
  if (j < num_g && count) atomicAdd(&pos[j], count);
}

__global__ __launch_bounds__(CK_THREADS) void cuhk03_scatter_kernel(const int32_t* __restrict__ g_pids, int num_g,
                                                                    const int32_t* __restrict__ pos,
                                                                    int32_t* __restrict__ sidx, int32_t* __restrict__ spid) {
  const int j = blockIdx.x * CK_THREADS + threadIdx.x;
  if (j < num_g) {
    const int p = pos[j];                         // a permutation of [0, num_g): (pid, index) is a total order
    sidx[p] = j;
    spid[p] = g_pids[j];
  }
}

// seg_start[s] = first position of the s-th identity (ascending pid) in sidx, seg_start[nseg] = num_g.  One workgroup.
__global__ __launch_bounds__(CK_THREADS) void cuhk03_segments_kernel(const int32_t* __restrict__ spid, int num_g,
                                                                     int32_t* __restrict__ seg_start, int32_t* nseg) {
  __shared__ uint32_t wsum[4];
  const int t = threadIdx.x;
  uint32_t carry = 0;
  for (int base = 0; base < num_g; base += CK_THREADS) {
    const int i = base + t;
    const uint32_t head = (i < num_g && (i == 0 || spid[i - 1] != spid[i])) ? 1u : 0u;
    uint32_t tot;
    const uint32_t ex = block_scan_excl(head, wsum, &tot);
    if (head) seg_start[carry + ex] = i;
    carry += tot;
  }
  if (t == 0) { seg_start[carry] = num_g; *nseg = (int32_t)carry; }
}

// One workgroup per query.  The kept true matches are taken from the query's own segment in batches of at most
// min(CK_TCAP, CK_STATES / max_rank), in segment order (a block scan, so the batches are the same on every launch), and
// sorted in LDS.  Per batch the identity segments are walked in ascending-pid order, up to CK_SLOTS at a time:
//   count   every image of the round's identities adds 1 to its identity's integer histogram over the sorted true-match
//           keys (slot = number of true keys <= the image's key, found by bisection); the inclusive prefix sum of a
//           histogram, a wave per identity, is c_j(t) for every true match t of the batch;
//   apply   the recurrence for all (true match, rank) states, one thread each, identity after identity, from one LDS
//           buffer into the other.  An identity with no image before the batch's last true match has p = 0 for every
//           state and is skipped (a ballot over the round's identities finds the others).  The query's own identity
//           gives the number of kept true matches before t instead.
// The curve of the batch is the running sum over ranks of the column sums of the pmf rows.
__global__ __launch_bounds__(CK_THREADS) void cuhk03_query_kernel(const float* __restrict__ distmat, int64_t ldd, int num_g,
                                                                  const int32_t* __restrict__ q_pids,
                                                                  const int32_t* __restrict__ q_keys,
                                                                  const int32_t* __restrict__ g_keys,
                                                                  const int32_t* __restrict__ sidx,
                                                                  const int32_t* __restrict__ spid,
                                                                  const int32_t* __restrict__ seg_start,
                                                                  const int32_t* __restrict__ nseg_p, int max_rank,
                                                                  double* __restrict__ cmc_out, double* __restrict__ ap_out) {
  __shared__ uint64_t tkeys[CK_TCAP];
  __shared__ double pmf[2][CK_STATES];
  __shared__ uint32_t cnt[CK_CNT];         // a round's histograms, nb + 1 words per identity
  __shared__ int32_t sb[CK_SLOTS + 1];     // the round's segment bounds
  __shared__ uint32_t others[CK_TCAP];     // kept entries of other identities before true match t
  __shared__ uint32_t before[CK_TCAP];     // kept true matches before true match t (all batches)
  __shared__ uint32_t wsum[4];
  __shared__ int32_t s_next;

  const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int R = max_rank, nseg = *nseg_p;
  const float* row = distmat + (int64_t)q * ldd;
  const int32_t qpid = q_pids[q], qkey = q_keys[q];
  double* cmc = cmc_out + (int64_t)q * R;

  // the query's own segment [oa, ob) of sidx: the numbers of sorted pids below and up to the query's, each from 256
  // evenly spaced probes and then the one gap the answer lies in (two loads deep instead of a bisection's chain)
  int oa, ob;
  {
    const int step = (num_g + CK_THREADS - 1) / CK_THREADS;
    const int64_t pi = (int64_t)t * step;
    const int32_t pv = pi < num_g ? spid[pi] : 0;
    const int c_lt = __syncthreads_count(pi < num_g && pv < qpid);
    const int c_le = __syncthreads_count(pi < num_g && pv <= qpid);
    // of the probes 0, step, 2 step, ... the first c hold and the next one, if there is one, does not
    auto refine = [&](int c, bool le) {
      const int lo = c ? (c - 1) * step + 1 : 0;
      const int hi = (int)min((int64_t)c * step, (int64_t)num_g);
      int n = lo;
      for (int b0 = lo; b0 < hi; b0 += CK_THREADS) {
        const int i = b0 + t;
        const int32_t v = i < hi ? spid[i] : 0;
        n += __syncthreads_count(i < hi && (le ? v <= qpid : v < qpid));
      }
      return n;
    };
    oa = refine(c_lt, false);
    ob = refine(c_le, true);
  }
  const uint32_t tcap = (uint32_t)min(CK_TCAP, CK_STATES / R);     // >= 2

  for (int k = t; k < R; k += CK_THREADS) cmc[k] = 0.0;            // rank k is this thread's from here to the end
  double ap_sum = 0.0;
  int64_t nt_total = 0;
  int cursor = oa;
  while (cursor < ob) {
    // ---- the next batch of kept true matches, in segment order
    uint32_t nb = 0;
    while (cursor < ob && nb < tcap) {
      if (t == 0) s_next = min(cursor + CK_THREADS, ob);
      __syncthreads();
      const int i = cursor + t;
      int j = 0;
      uint32_t kept = 0;
      if (i < ob) {
        j = sidx[i];
        kept = g_keys[j] != qkey ? 1u : 0u;
      }
      uint32_t tot;
      const uint32_t pos = nb + block_scan_excl(kept, wsum, &tot);
      if (kept) {
        if (pos < tcap) tkeys[pos] = ck_key(row[j], (uint32_t)j);
        else if (pos == tcap) s_next = i;                          // the first one that does not fit opens the next batch
      }
      __syncthreads();
      cursor = s_next;
      nb = min(nb + tot, tcap);
      __syncthreads();
    }
    if (nb == 0) break;                                            // the rest of the segment was removed entries
    // ---- the batch's pmf rows and counts start over (under the sort's first barrier), the true matches are sorted
    const uint32_t nstates = nb * (uint32_t)R;
    for (uint32_t st = t; st < nstates; st += CK_THREADS) pmf[0][st] = (st % (uint32_t)R) == 0 ? 1.0 : 0.0;
    for (uint32_t i = t; i < nb; i += CK_THREADS) { others[i] = 0; before[i] = 0; }
    lds_bitonic_sort<CK_THREADS>(tkeys, nb);
    const uint64_t kmax = tkeys[nb - 1];
    int cur = 0;
    const uint32_t stride = nb + 1;                                // words of one identity's histogram
    const int slots = min(CK_SLOTS, CK_CNT / (int)stride);         // identities per round, >= 8
    for (int base = 0; base < nseg; base += slots) {
      const int ns = min(slots, nseg - base);
      for (int i = t; i <= ns; i += CK_THREADS) sb[i] = seg_start[base + i];
      for (uint32_t i = t; i < (uint32_t)ns * stride; i += CK_THREADS) cnt[i] = 0;
      __syncthreads();
      // ---- count: the round's images over all threads, CK_UNR index loads and then CK_UNR distance gathers in flight
      // per thread before the first is used (the chain index -> distance is what a round waits for)
      const int p1 = sb[ns];
      for (int i0 = sb[0] + t; i0 < p1; i0 += CK_UNR * CK_THREADS) {
        int jj[CK_UNR];
        float dd[CK_UNR];
#pragma unroll
        for (int u = 0; u < CK_UNR; ++u) {
          const int i = i0 + u * CK_THREADS;
          jj[u] = i < p1 ? sidx[i] : -1;
        }
#pragma unroll
        for (int u = 0; u < CK_UNR; ++u) dd[u] = jj[u] >= 0 ? row[jj[u]] : 0.f;
#pragma unroll
        for (int u = 0; u < CK_UNR; ++u) {
          const int i = i0 + u * CK_THREADS, j = jj[u];
          if (j < 0) continue;
          const uint64_t key = ck_key(dd[u], (uint32_t)j);
          if (key > kmax) continue;                                // after every true match of the batch
          int sl = 0, sh = ns;                                     // sb[sl] <= i < sb[sh]
          while (sh - sl > 1) {
            const int mid = (sl + sh) >> 1;
            if (sb[mid] <= i) sl = mid; else sh = mid;
          }
          if (sb[sl] == oa && g_keys[j] == qkey) continue;         // removed: the filter of the collection above
          uint32_t lo = 0, hi = nb;                                // number of true keys <= key
          while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (tkeys[mid] <= key) lo = mid + 1; else hi = mid;
          }
          atomicAdd(&cnt[sl * stride + lo], 1u);                   // lo == nb (the last true match itself): before none
        }
      }
      __syncthreads();
      // ---- inclusive prefix sums, a wave per identity: c[i] = images of the identity before true match i
      for (int sl = wave; sl < ns; sl += 4) {
        uint32_t* c = cnt + sl * stride;
        uint32_t carry = 0;
        for (uint32_t c0 = 0; c0 < nb; c0 += 64) {
          const uint32_t i = c0 + lane;
          const uint32_t inc = wave_scan_incl(i < nb ? c[i] : 0u) + carry;
          if (i < nb) c[i] = inc;
          carry = __shfl(inc, 63);
        }
      }
      __syncthreads();
      // ---- apply, in ascending-pid order.  Every wave forms the same two masks from LDS, so the loop is uniform over
      // the block: the identities with an image before the batch's last true match (the others have p = 0 for every
      // state: no-ops), and the query's own identity, which gives the kept true matches before t instead.
      const uint64_t own_mask = __ballot(lane < ns && sb[lane] == oa);
      uint64_t todo = __ballot(lane < ns && cnt[lane * stride + nb - 1] != 0) & ~own_mask;
      if (own_mask) {
        const uint32_t* c = cnt + (__ffsll((unsigned long long)own_mask) - 1) * stride;
        for (uint32_t i = t; i < nb; i += CK_THREADS) before[i] = c[i];
      }
      while (todo) {
        const int sl = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t* c = cnt + sl * stride;
        const double n = (double)(sb[sl + 1] - sb[sl]);
        for (uint32_t i = t; i < nb; i += CK_THREADS) others[i] += c[i];
        for (uint32_t st = t; st < nstates; st += CK_THREADS) {
          const uint32_t tt = st / (uint32_t)R, k = st - tt * (uint32_t)R;
          const double p = (double)c[tt] / n;
          const double old = pmf[cur][st], prev = k ? pmf[cur][st - 1] : 0.0;
          pmf[cur ^ 1][st] = old * (1.0 - p) + prev * p;
        }
        __syncthreads();
        cur ^= 1;
      }
      __syncthreads();
    }
    // ---- the batch's curve: column sums over its true matches, then the running sum over ranks
    double* col = pmf[cur ^ 1];
    for (int k = t; k < R; k += CK_THREADS) {
      double s = 0.0;
      for (uint32_t tt = 0; tt < nb; ++tt) s += pmf[cur][tt * (uint32_t)R + k];
      col[k] = s;
    }
    __syncthreads();
    for (int k = t; k < R; k += CK_THREADS) {
      double s = 0.0;
      for (int i = 0; i <= k; ++i) s += col[i];
      cmc[k] += s;
    }
    __syncthreads();
    // ---- AP terms (rank.py:86-90): matches up to and including t over kept entries up to and including t
    double part = 0.0;
    for (uint32_t i = t; i < nb; i += CK_THREADS)
      part += (double)(before[i] + 1u) / (double)(others[i] + before[i] + 1u);
    block_tree_sum(part, col);
    ap_sum += col[0];
    nt_total += nb;
    __syncthreads();
  }
  if (nt_total > 0) {
    for (int k = t; k < R; k += CK_THREADS) cmc[k] = cmc[k] / (double)nt_total;
  }
  if (t == 0) ap_out[q] = nt_total > 0 ? ap_sum / (double)nt_total : -1.0;   // rank.py:62-64: skipped
}

// summary = [max_rank curve sums over the valid queries, number of valid queries, AP sum].  Workgroup k sums column k
// (workgroup max_rank the APs): a contiguous span of queries per thread, then a binary tree over the threads, the
// association rank_finalize_kernel uses -- the same on every launch, and for the APs the same as the Market evaluator's.
__global__ __launch_bounds__(CK_THREADS) void cuhk03_finalize_kernel(const double* __restrict__ cmc,
                                                                     const double* __restrict__ ap, int num_q, int max_rank,
                                                                     double* __restrict__ summary) {
  __shared__ double dsum[CK_THREADS];
  __shared__ uint32_t nsum[CK_THREADS];
  const int t = threadIdx.x, k = blockIdx.x;
  const int per = (num_q + CK_THREADS - 1) / CK_THREADS;
  double s = 0.0;
  uint32_t nv = 0;
  for (int64_t q = (int64_t)t * per; q < min((int64_t)num_q, (int64_t)(t + 1) * per); ++q) {
    const double a = ap[q];
    if (a >= 0.0) {
      ++nv;
      s += k < max_rank ? cmc[q * max_rank + k] : a;
    }
  }
  block_tree_sum(s, nv, dsum, nsum, [](uint32_t a, uint32_t b) { return a + b; });
  if (t == 0) {
    if (k < max_rank) {
      summary[k] = dsum[0];
    } else {
      summary[max_rank] = (double)nsum[0];
      summary[max_rank + 1] = dsum[0];
    }
  }
}

}  // namespace ieee

using namespace ieee;

extern "C" int64_t ieee_rank_cuhk03_workspace_bytes(int64_t num_g) {
  return (int64_t)sizeof(int32_t) * (4 * (num_g > 0 ? num_g : 0) + 2);   // sidx, spid, seg_start[num_g + 1], nseg, pos
}

extern "C" int ieee_rank_cuhk03(const float* distmat, int64_t ldd, int64_t num_q, int64_t num_g, const int32_t* q_pids,
                                const int32_t* g_pids, const int32_t* q_keys, const int32_t* g_keys, int64_t max_rank,
                                double* cmc, double* ap, double* summary, void* work, int64_t work_bytes, void* stream) {
  IEEE_REQUIRE(distmat && q_pids && g_pids && q_keys && g_keys && cmc && ap && summary && work, "rank_cuhk03: null pointer");
  IEEE_REQUIRE(num_q > 0 && num_g > 0, "rank_cuhk03: empty distmat");
  IEEE_REQUIRE(num_g < (1ll << 31) - 1024 && num_q < (1ll << 31), "rank_cuhk03: too large");
  IEEE_REQUIRE(ldd >= num_g, "rank_cuhk03: ldd %ld < num_g %ld", (long)ldd, (long)num_g);
  IEEE_REQUIRE(max_rank >= 1 && max_rank <= CK_MAX_RANK, "rank_cuhk03: max_rank %ld out of range [1,%d]", (long)max_rank,
               CK_MAX_RANK);
  IEEE_REQUIRE(work_bytes >= ieee_rank_cuhk03_workspace_bytes(num_g), "rank_cuhk03: workspace of %ld bytes, %ld needed",
               (long)work_bytes, (long)ieee_rank_cuhk03_workspace_bytes(num_g));
  IEEE_REQUIRE(((uintptr_t)work & 3) == 0, "rank_cuhk03: workspace not 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int32_t* sidx = (int32_t*)work;
  int32_t* spid = sidx + num_g;
  int32_t* seg_start = spid + num_g;
  int32_t* nseg = seg_start + num_g + 1;
  int32_t* pos = nseg + 1;
  // about a thousand workgroups for the quadratic count: the gallery in spans of whole 1024-entry tiles
  const int gx = cdiv(num_g, CK_THREADS);
  const int want = (1024 + gx - 1) / gx;
  const int64_t span = (int64_t)cdiv(cdiv(num_g, want), 1024) * 1024;
  const int gy = cdiv(num_g, span);
  IEEE_HIP(hipMemsetAsync(pos, 0, sizeof(int32_t) * num_g, st));
  cuhk03_order_kernel<<<dim3(gx, gy), CK_THREADS, 0, st>>>(g_pids, (int)num_g, (int)span, pos);
  cuhk03_scatter_kernel<<<gx, CK_THREADS, 0, st>>>(g_pids, (int)num_g, pos, sidx, spid);
  cuhk03_segments_kernel<<<1, CK_THREADS, 0, st>>>(spid, (int)num_g, seg_start, nseg);
  cuhk03_query_kernel<<<(int)num_q, CK_THREADS, 0, st>>>(distmat, ldd, (int)num_g, q_pids, q_keys, g_keys, sidx, spid,
                                                         seg_start, nseg, (int)max_rank, cmc, ap);
  cuhk03_finalize_kernel<<<(int)max_rank + 1, CK_THREADS, 0, st>>>(cmc, ap, (int)num_q, (int)max_rank, summary);
  return launch_status("rank_cuhk03");
}
