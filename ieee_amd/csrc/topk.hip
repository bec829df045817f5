// Ranked retrieval: the k nearest kept gallery entries of every query, on the device.
// Reference: torchreid/utils/reidtools.py:49 (np.argsort(distmat, axis=1)) and :110-112 (the same-identity,
// same-camera entries are skipped); the rule is rank.py:136-137's.  The result equals a stable argsort of the
// filtered row: order on (distance, gallery index), -0.0 == +0.0, NaN after +inf (rank_common.h's folded order).
#include "rank_common.h"

namespace ieee {

constexpr int TOPK_MAX = 1024;
constexpr int TOPK_THREADS = 256;
constexpr int TOPK_UNR = 2;                                // 16-byte loads per thread per chunk
constexpr int TOPK_CHUNK = TOPK_UNR * 4 * TOPK_THREADS;    // 2048 distances streamed between two buffer checks
constexpr int TOPK_STORE = 2 * TOPK_CHUNK;                 // LDS candidate keys (32 KB)
constexpr int TOPK_SELECT_AT = TOPK_STORE - TOPK_CHUNK;    // more candidates than this: select down to k first

// One workgroup per query.  The row streams past in chunks of TOPK_CHUNK, loaded two chunks ahead; an element enters
// the LDS candidate buffer only when its key is below the running k-th key.  When the buffer holds more than
// select_at keys, select() drops the same-identity same-camera entries among the new ones (the only identity and
// camera reads: about k·ln(G/k) per row, never in the stream, where a dependent load would drain the loads in flight),
// sorts the rest and keeps k, which tightens the threshold; the room left always takes a whole chunk.  Adversarial
// rows (descending, all equal, all filtered) select more often but stay exact.
//
// MERGE: distmat is a column slab, the distances to gallery entries g_base ... g_base + num_g - 1 (labels indexed by
// the local column), and out_idx / out_dist hold the list so far, ascending, -1 / +inf in the unused places.  The
// list's entries start out as keys[0, kept) (filtered when they entered) and the stream's keys carry global indices;
// everything between is the same code.  The keys fold -0.0 and NaN payloads, so the old distances wait in LDS; the
// entries that stay are a prefix of the old list in the old order (whatever beats one of them beats the later ones),
// so the p-th old entry of the new list is the old list's p-th.  The old list is read before anything is written.
template <bool MERGE>
__global__ __launch_bounds__(TOPK_THREADS) void rank_topk_kernel(const float* __restrict__ distmat, int64_t ldd, int num_g,
                                                                 const int32_t* __restrict__ q_pids,
                                                                 const int32_t* __restrict__ g_pids,
                                                                 const int32_t* __restrict__ q_camids,
                                                                 const int32_t* __restrict__ g_camids, int filter, int k,
                                                                 int32_t* __restrict__ out_idx, float* __restrict__ out_dist,
                                                                 int g_base) {
  constexpr int PAIRS = TOPK_STORE / (2 * TOPK_THREADS);   // compare-exchange pairs per thread and sort stage, at most
  __shared__ uint64_t keys[TOPK_STORE];
  __shared__ uint32_t s_cnt, s_bad;
  __shared__ uint64_t s_thr;
  __shared__ float old_dist[MERGE ? TOPK_MAX : 1];         // MERGE: the list's distances as they came in (4 KB)
  __shared__ uint32_t s_wsum[4];

  const int q = blockIdx.x, t = threadIdx.x;
  const float* row = distmat + (int64_t)q * ldd;
  const int32_t qpid = filter ? q_pids[q] : 0, qcam = filter ? q_camids[q] : 0;
  const uint32_t gb = MERGE ? (uint32_t)g_base : 0u;
  // select when the buffer is past this: small k selects early (the first chunk is sorted at 2048, not 4096)
  const uint32_t select_at = (uint32_t)min(TOPK_SELECT_AT, max(2 * k, 512));
  if (t == 0) { s_cnt = 0; s_bad = 0; s_thr = ~0ull; }
  __syncthreads();

  uint32_t kept = 0;   // keys[0, kept) survived the last select: filtered already
  if constexpr (MERGE) {
    uint32_t mine = 0;
    for (int i = t; i < k; i += TOPK_THREADS) {
      const int32_t j = out_idx[(int64_t)q * k + i];
      const float d = out_dist[(int64_t)q * k + i];
      old_dist[i] = d;
      if (j >= 0) { keys[i] = order_key(order_word_folded(d), (uint32_t)j); ++mine; }   // unused places are at the end
    }
    if (mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    kept = s_cnt;                              // k <= select_at: the first chunk still fits
    if (t == 0 && kept == (uint32_t)k) s_thr = keys[k - 1];
    __syncthreads();
  }
  // drop the filtered keys among keys[kept, n), sort keys[0, n) ascending (padded with ~0 to a power of two), keep
  // the first k, tighten the threshold
  auto select = [&]() {
    const uint32_t n = min(s_cnt, (uint32_t)TOPK_STORE);
    if (filter) {
      uint32_t bad = 0;
      for (uint32_t i = kept + t; i < n; i += TOPK_THREADS) {
        const uint32_t j = (uint32_t)keys[i] - gb;
        if (g_pids[j] == qpid && g_camids[j] == qcam) { keys[i] = ~0ull; ++bad; }
      }
      if (bad) atomicAdd(&s_bad, bad);
    }
    uint32_t np2 = 1;
    while (np2 < n) np2 <<= 1;
    for (uint32_t i = n + t; i < np2; i += TOPK_THREADS) keys[i] = ~0ull;
    __syncthreads();
    const uint32_t half = np2 >> 1;
    for (uint32_t kk = 2; kk <= np2; kk <<= 1) {
      for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
        uint64_t a[PAIRS], b[PAIRS];   // every pair's two loads in flight before the first compare
#pragma unroll
        for (int r = 0; r < PAIRS; ++r) {
          const uint32_t p = t + r * TOPK_THREADS, i = 2 * p - (p & (j - 1));
          if (p < half) { a[r] = keys[i]; b[r] = keys[i + j]; }
        }
#pragma unroll
        for (int r = 0; r < PAIRS; ++r) {
          const uint32_t p = t + r * TOPK_THREADS, i = 2 * p - (p & (j - 1));
          if (p < half && (a[r] > b[r]) == ((i & kk) == 0)) { keys[i] = b[r]; keys[i + j] = a[r]; }
        }
        __syncthreads();
      }
    }
    const uint32_t valid = n - s_bad;
    kept = min(valid, (uint32_t)k);
    const uint64_t kth = keys[k - 1];
    __syncthreads();
    if (t == 0) {
      s_cnt = kept;
      s_bad = 0;
      if (valid >= (uint32_t)k) s_thr = kth;
    }
    __syncthreads();
  };

  typedef float f32x4v __attribute__((ext_vector_type(4)));
  int last_pos = -1;   // this thread's highest buffer slot in the previous chunk
  auto visit = [&](int base, const f32x4v* cur) {
    // the thread that took the highest slot knows the buffer's fill: one barrier, a block-uniform decision
    if (__syncthreads_or(last_pos + 1 > (int)select_at)) select();
    last_pos = -1;
    const uint64_t thr = s_thr;
    const uint32_t thr_hi = (uint32_t)(thr >> 32);
#pragma unroll
    for (int u = 0; u < TOPK_UNR; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = base + u * 1024 + t * 4 + e;
        const uint32_t w = order_word_folded(cur[u][e]);
        if (j < num_g && w <= thr_hi) {
          const uint64_t key = order_key(w, gb + (uint32_t)j);
          if (key < thr) {
            const uint32_t pos = atomicAdd(&s_cnt, 1u);
            if (pos < (uint32_t)TOPK_STORE) keys[pos] = key;     // always true: a chunk fits in the room left
            last_pos = (int)pos;
          }
        }
      }
  };

  // whole chunks of a 16-byte aligned row: loaded two chunks ahead into three rotating buffers.  Every step issues its
  // loads, past the end re-reading the last whole chunk (unused), so the number of loads in flight is the same on every
  // path and the wait for the current chunk leaves the two ahead of it outstanding.
  const int nfull = ((uintptr_t)row & 15) == 0 ? num_g / TOPK_CHUNK * TOPK_CHUNK : 0;
  auto load = [&](int base, f32x4v* v) {
    const int b = base + TOPK_CHUNK <= nfull ? base : nfull - TOPK_CHUNK;
#pragma unroll
    for (int u = 0; u < TOPK_UNR; ++u) v[u] = __builtin_nontemporal_load((const f32x4v*)(row + b + u * 1024 + t * 4));
  };
  f32x4v b0[TOPK_UNR], b1[TOPK_UNR], b2[TOPK_UNR];
  if (nfull > 0) {
    load(0, b0);
    load(TOPK_CHUNK, b1);
  }
  for (int base = 0; base < nfull; base += 3 * TOPK_CHUNK) {   // block-uniform bounds throughout
    load(base + 2 * TOPK_CHUNK, b2);
    visit(base, b0);
    load(base + 3 * TOPK_CHUNK, b0);
    if (base + TOPK_CHUNK < nfull) visit(base + TOPK_CHUNK, b1);
    load(base + 4 * TOPK_CHUNK, b1);
    if (base + 2 * TOPK_CHUNK < nfull) visit(base + 2 * TOPK_CHUNK, b2);
  }
  // the rest (the tail, or a whole row that is not 16-byte aligned), element by element
  for (int base = nfull; base < num_g; base += TOPK_CHUNK) {
#pragma unroll
    for (int u = 0; u < TOPK_UNR; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = base + u * 1024 + t * 4 + e;
        b0[u][e] = j < num_g ? row[j] : 0.f;
      }
    visit(base, b0);
  }
  __syncthreads();
  select();
  if constexpr (MERGE) {
    // places 4t ... 4t + 3 of the new list: an entry below g_base was in the old list, at the place that is the count
    // of such entries before it (at most k of them, so old_dist is never read past its end)
    constexpr int PER = TOPK_MAX / TOPK_THREADS;
    uint32_t old_here = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const uint32_t i = t * PER + e;
      if (i < kept && (uint32_t)keys[i] < gb) ++old_here;
    }
    uint32_t old_all;
    uint32_t p = block_scan_excl(old_here, s_wsum, &old_all);
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const uint32_t i = t * PER + e;
      if (i >= (uint32_t)k) break;
      const int64_t o = (int64_t)q * k + i;
      if (i < kept) {
        const uint32_t j = (uint32_t)keys[i];
        out_idx[o] = (int32_t)j;
        out_dist[o] = j < gb ? old_dist[p++] : row[min(j - gb, (uint32_t)num_g - 1)];
      } else {
        out_idx[o] = -1;
        out_dist[o] = __uint_as_float(0x7F800000u);
      }
    }
    return;
  }
  for (int i = t; i < k; i += TOPK_THREADS) {
    const int64_t o = (int64_t)q * k + i;
    if ((uint32_t)i < kept) {
      const uint32_t j = (uint32_t)keys[i];
      out_idx[o] = (int32_t)j;
      out_dist[o] = row[j];            // the stored value itself (the key folds -0.0 and NaN payloads)
    } else {
      out_idx[o] = -1;                 // fewer than k kept entries
      out_dist[o] = __uint_as_float(0x7F800000u);
    }
  }
}

}  // namespace ieee

using namespace ieee;

extern "C" int ieee_rank_topk(const float* distmat, int64_t ldd, int64_t num_q, int64_t num_g, const int32_t* q_pids,
                              const int32_t* g_pids, const int32_t* q_camids, const int32_t* g_camids, int exclude_same_cam,
                              int64_t k, int32_t* out_idx, float* out_dist, void* stream) {
  IEEE_REQUIRE(k >= 1 && k <= TOPK_MAX, "rank_topk: k = %ld out of range [1, %d]", (long)k, TOPK_MAX);
  IEEE_REQUIRE(num_q >= 0 && num_g >= 0, "rank_topk: negative size");
  IEEE_REQUIRE(num_q < (1ll << 31) && num_g < (1ll << 31) - 3 * TOPK_CHUNK, "rank_topk: too large");
  IEEE_REQUIRE(ldd >= num_g, "rank_topk: ldd %ld < num_g %ld", (long)ldd, (long)num_g);
  if (num_q == 0) return IEEE_OK;
  IEEE_REQUIRE(out_idx && out_dist, "rank_topk: null output");
  IEEE_REQUIRE(distmat || num_g == 0, "rank_topk: null distmat");
  IEEE_REQUIRE(!exclude_same_cam || (q_pids && g_pids && q_camids && g_camids), "rank_topk: filter without labels");
  rank_topk_kernel<false><<<(int)num_q, TOPK_THREADS, 0, (hipStream_t)stream>>>(
      distmat, ldd, (int)num_g, q_pids, g_pids, q_camids, g_camids, exclude_same_cam ? 1 : 0, (int)k, out_idx, out_dist, 0);
  return launch_status("rank_topk");
}

extern "C" int ieee_rank_topk_merge(const float* slab, int64_t ldd, int64_t num_q, int64_t slab_g, int64_t g_base,
                                    const int32_t* q_pids, const int32_t* slab_g_pids, const int32_t* q_camids,
                                    const int32_t* slab_g_camids, int exclude_same_cam, int64_t k, int32_t* state_idx,
                                    float* state_dist, void* stream) {
  IEEE_REQUIRE(k >= 1 && k <= TOPK_MAX, "rank_topk_merge: k = %ld out of range [1, %d]", (long)k, TOPK_MAX);
  IEEE_REQUIRE(num_q >= 0 && slab_g >= 0 && g_base >= 0, "rank_topk_merge: negative size or base");
  IEEE_REQUIRE(num_q < (1ll << 31) && slab_g < (1ll << 31) && g_base < (1ll << 31) &&
                   g_base + slab_g < (1ll << 31) - 3 * TOPK_CHUNK,
               "rank_topk_merge: too large");
  IEEE_REQUIRE(ldd >= slab_g, "rank_topk_merge: ldd %ld < slab_g %ld", (long)ldd, (long)slab_g);
  IEEE_REQUIRE(num_q == 0 || (state_idx && state_dist), "rank_topk_merge: null state");
  IEEE_REQUIRE(!exclude_same_cam || (q_pids && slab_g_pids && q_camids && slab_g_camids),
               "rank_topk_merge: filter without labels");
  if (num_q == 0 || slab_g == 0) return IEEE_OK;
  IEEE_REQUIRE(slab, "rank_topk_merge: null slab");
  rank_topk_kernel<true><<<(int)num_q, TOPK_THREADS, 0, (hipStream_t)stream>>>(
      slab, ldd, (int)slab_g, q_pids, slab_g_pids, q_camids, slab_g_camids, exclude_same_cam ? 1 : 0, (int)k, state_idx,
      state_dist, (int)g_base);
  return launch_status("rank_topk_merge");
}
