"""CMC / mAP without the [Q, G] distance matrix: the Market1501 protocol of rank.py (eval_market1501, rank_counts) with
the gallery going by in column slabs, twice.  All four label arrays are on the host before anything starts, so the host
plans: per query the gallery indices of its true matches (same identity, other camera) and of its removed entries (same
identity, same camera).  Pass 1 visits only the gallery rows that occur in the plan and keeps their distances as
(distance, global index) keys; after seal() has sorted them, pass 2 visits every gallery column once, in any order, and
adds to a running count per match key how many entries of the slab sort at or before it -- rank_query_fast_kernel's
stream, per slab.  result() is rank_counts' for the whole matrix (include/ieee_amd.h, ieee_rank_stream_*: counts and
first positions equal, APs equal as bits up to 1024 matches and 1024 removed entries per query) while the device holds
one [Q, slab] buffer, 12 bytes per match key and 8 per removed key.  The reference has nothing of the kind (rank.py:103-171 argsorts the
whole matrix on the host)."""
import bisect

import numpy as np
import torch

from .. import _lib
from . import distance as _dist
from ._stream import (SlabDistances, check_device, check_metric, check_precision, check_query, check_slab, count_rows,
                      device_matrix, host_labels, on_device, walk)
from .rank import finish_counts

RANK_STREAM_INDEX_LIMIT = 1 << 31   # ieee_rank_stream_collect / _count refuse a slab that ends at or beyond this index
MAX_RANK_LIMIT = 1024               # rank_finalize_kernel's histogram


class RankPlan(object):
    """What the labels alone decide.  Two CSR lists over the queries, gallery indices in (camera, index) order inside
    a query (the kernels ask for no order): m_off int64 [Q + 1] / m_idx int32: the true matches; r_off / r_idx: the
    removed entries.  match_columns (int64, ascending) lists the gallery indices that occur in either; m_pos / r_pos
    (int32) are the places of m_idx / r_idx in it.  Vectorised: no Python loop over queries or gallery."""

    def __init__(self, q_pids, q_camids, g_pids, g_camids):
        num_q, num_g = q_pids.size, g_pids.size
        # one sortable word per (identity, camera): the gallery in (identity, camera, index) order
        word = lambda p, c: ((p.astype(np.int64) + (1 << 31)).astype(np.uint64) << np.uint64(32)) | \
            (c.astype(np.int64) + (1 << 31)).astype(np.uint64)
        gw, qw = word(g_pids, g_camids), word(q_pids, q_camids)
        order = np.argsort(gw, kind="stable")
        gw = gw[order]
        low, high = qw & ~np.uint64(0xffffffff), qw | np.uint64(0xffffffff)
        lo, hi = np.searchsorted(gw, low, "left"), np.searchsorted(gw, high, "right")      # the query's identity
        rlo, rhi = np.searchsorted(gw, qw, "left"), np.searchsorted(gw, qw, "right")       # ... on the query's camera
        self.r_off, self.r_idx = self._csr(order, rlo.reshape(-1, 1), (rhi - rlo).reshape(-1, 1))
        self.m_off, self.m_idx = self._csr(order, np.stack([lo, rhi], 1), np.stack([rlo - lo, hi - rhi], 1))
        # a gallery entry is in some query's lists exactly when its identity occurs among the queries
        self.match_columns = np.flatnonzero(np.isin(g_pids, np.unique(q_pids))).astype(np.int64)
        place = np.full(num_g, -1, dtype=np.int32)
        place[self.match_columns] = np.arange(self.match_columns.size, dtype=np.int32)
        self.m_pos, self.r_pos = place[self.m_idx], place[self.r_idx]
        self.num_q, self.num_g = num_q, num_g

    @staticmethod
    def _csr(order, starts, lens):
        """order[starts[q, j] : starts[q, j] + lens[q, j]] for every j, joined per query"""
        num_q = starts.shape[0]
        off = np.zeros(num_q + 1, dtype=np.int64)
        np.cumsum(lens.sum(1), out=off[1:])
        flat_len, flat_start = lens.reshape(-1).astype(np.int64), starts.reshape(-1).astype(np.int64)
        before = np.cumsum(flat_len) - flat_len                      # entries ahead of every run
        at = np.repeat(flat_start - before, flat_len) + np.arange(int(off[-1]), dtype=np.int64)
        return off, order[at].astype(np.int32)


class RankAccumulator(object):
    """The Market1501 evaluation of num_q queries against a gallery whose distances arrive in column slabs.

    collect() takes the distances to the gallery entries match_columns[num_collected : num_collected + n] (pass 1, in
    this order); seal() closes pass 1; count(slab, g_base) takes the distances to gallery entries g_base ... g_base +
    n - 1 (pass 2: every column once, in any order); result() is rank_counts' triple for the slabs side by side.  The
    device is first needed when a call has work for it."""

    def __init__(self, q_pids, q_camids, g_pids, g_camids, max_rank=20, device=None):
        who = "RankAccumulator"
        q_pids = host_labels(q_pids, "q_pids", None, who)
        q_camids = host_labels(q_camids, "q_camids", q_pids.size, who)
        g_pids = host_labels(g_pids, "g_pids", None, who)
        g_camids = host_labels(g_camids, "g_camids", g_pids.size, who)
        if isinstance(max_rank, bool) or int(max_rank) != max_rank or not 1 <= int(max_rank) <= MAX_RANK_LIMIT:
            raise ValueError("%s: max_rank must be an integer in [1, %d], got %r" % (who, MAX_RANK_LIMIT, max_rank))
        if g_pids.size >= RANK_STREAM_INDEX_LIMIT or q_pids.size >= RANK_STREAM_INDEX_LIMIT:
            raise ValueError("%s: more than %d entries" % (who, RANK_STREAM_INDEX_LIMIT - 1))
        self.device = check_device(device, who)
        self.num_q, self.num_g = int(q_pids.size), int(g_pids.size)
        self.max_rank = max(1, min(int(max_rank), self.num_g))      # rank.py:110-115
        self.plan = RankPlan(q_pids, q_camids, g_pids, g_camids)
        self.match_columns = self.plan.match_columns
        self.num_collected = self.num_counted = 0
        self.sealed = False
        self._counted = []              # disjoint [lo, hi) column ranges, ascending
        self._dev = None
        self._summary = None

    # ---- the device side, on first use
    def _state(self):
        if self._dev is None:
            lib, p, dev = _lib.require_gpu(), self.plan, self.device
            tm, tr = int(p.m_off[-1]), int(p.r_off[-1])
            nbytes = int(lib.ieee_rank_stream_workspace_bytes(self.num_q, tm, tr))
            self._dev = dict(lib=lib, tm=tm, tr=tr, state=torch.empty(nbytes, dtype=torch.uint8, device=dev),
                             **{name: on_device(getattr(p, name), dev)
                                for name in ("m_off", "m_pos", "m_idx", "r_off", "r_pos", "r_idx")},
                             ap=torch.empty(self.num_q, dtype=torch.float64, device=dev),
                             first=torch.empty(self.num_q, dtype=torch.int32, device=dev))
        return self._dev

    def _slab(self, dist_slab, who):
        """the slab's column count, its shape checked"""
        if getattr(dist_slab, "ndim", None) != 2 or dist_slab.shape[0] != self.num_q:
            raise ValueError("%s: the slab must be [%d, n], got shape %s"
                             % (who, self.num_q, tuple(getattr(dist_slab, "shape", ()))))
        return int(dist_slab.shape[1])

    # ---- pass 1
    def collect(self, dist_slab):
        who = "RankAccumulator.collect"
        n = self._slab(dist_slab, who)
        if self.sealed:
            raise ValueError("%s: called after seal()" % who)
        if self.num_collected + n > self.match_columns.size:
            raise ValueError("%s: %d + %d columns run past the %d match columns"
                             % (who, self.num_collected, n, self.match_columns.size))
        if self.num_q and n:
            self._collect(*device_matrix(dist_slab, self.device, n), n)
        else:
            self.num_collected += n

    def _collect(self, d, ldd, n):
        """d: fp32 on the device, unit column stride, row stride ldd >= n"""
        s = self._state()
        _lib.check(s["lib"].ieee_rank_stream_collect(_lib.ptr(d), ldd, self.num_q, n, self.num_collected,
                                                     _lib.ptr(s["m_off"]), _lib.ptr(s["m_pos"]), _lib.ptr(s["m_idx"]),
                                                     _lib.ptr(s["r_off"]), _lib.ptr(s["r_pos"]), _lib.ptr(s["r_idx"]),
                                                     s["tm"], s["tr"], _lib.ptr(s["state"]), s["state"].numel(),
                                                     _lib.stream()))
        self.num_collected += n

    def seal(self):
        who = "RankAccumulator.seal"
        if self.num_collected != self.match_columns.size:
            raise ValueError("%s: %d of the %d match columns were collected"
                             % (who, self.num_collected, self.match_columns.size))
        if not self.sealed and self.num_q and self.match_columns.size:
            s = self._state()
            _lib.check(s["lib"].ieee_rank_stream_seal(self.num_q, _lib.ptr(s["m_off"]), _lib.ptr(s["r_off"]), s["tm"],
                                                      s["tr"], _lib.ptr(s["state"]), s["state"].numel(), _lib.stream()))
        self.sealed = True

    # ---- pass 2
    def count(self, dist_slab, g_base):
        who = "RankAccumulator.count"
        n = self._slab(dist_slab, who)
        if not self.sealed:
            raise ValueError("%s: called before seal()" % who)
        if isinstance(g_base, bool) or int(g_base) != g_base or g_base < 0 or int(g_base) + n > self.num_g:
            raise ValueError("%s: columns %r ... + %d run past the gallery's %d" % (who, g_base, n, self.num_g))
        g_base = int(g_base)
        self._claim(g_base, n, who)
        if self.num_q and n and self.match_columns.size:
            self._count(*device_matrix(dist_slab, self.device, n), n, g_base)

    def _claim(self, g_base, n, who="RankAccumulator.count"):
        if n == 0:
            return
        at = bisect.bisect_left(self._counted, (g_base, g_base))
        if (at and self._counted[at - 1][1] > g_base) or (at < len(self._counted) and self._counted[at][0] < g_base + n):
            raise ValueError("%s: columns %d ... %d overlap a range counted before" % (who, g_base, g_base + n - 1))
        self._counted.insert(at, (g_base, g_base + n))
        self.num_counted += n
        self._summary = None

    def _count(self, d, ldd, n, g_base):
        """d: fp32 on the device, unit column stride, row stride ldd >= n; the range was claimed"""
        s = self._state()
        _lib.check(s["lib"].ieee_rank_stream_count(_lib.ptr(d), ldd, self.num_q, n, g_base, _lib.ptr(s["m_off"]),
                                                   _lib.ptr(s["r_off"]), s["tm"], s["tr"], _lib.ptr(s["state"]), s["state"].numel(),
                                                   _lib.stream()))

    # ---- finish
    def _finish(self):
        if self.num_counted != self.num_g:
            raise ValueError("RankAccumulator: %d of the %d gallery columns were counted" % (self.num_counted, self.num_g))
        if self._summary is None:
            s = self._state()
            summary = torch.empty(self.max_rank + 2, dtype=torch.int64, device=self.device)
            _lib.check(s["lib"].ieee_rank_stream_finish(self.num_q, _lib.ptr(s["m_off"]), _lib.ptr(s["r_off"]), s["tm"],
                                                        s["tr"], _lib.ptr(s["state"]), s["state"].numel(), self.max_rank,
                                                        _lib.ptr(s["ap"]), _lib.ptr(s["first"]), _lib.ptr(summary),
                                                        _lib.stream()))
            self._summary = summary.cpu().numpy()       # the single read-back (max_rank + 2 words)
        return self._summary

    def result(self):
        """-> (cmc_counts int64[max_rank], num_valid_q, ap_sum): rank_counts' triple, additive over disjoint query sets"""
        if self.num_q == 0:
            if self.num_counted != self.num_g:
                raise ValueError("RankAccumulator: %d of the %d gallery columns were counted"
                                 % (self.num_counted, self.num_g))
            return np.zeros(self.max_rank, dtype=np.int64), 0.0, 0.0
        s, r = self._finish(), self.max_rank
        return s[:r].copy(), float(s[r]), float(s[r + 1:r + 2].view(np.float64)[0])

    def per_query(self):
        """-> (ap float64[num_q], first int32[num_q]) on the device; -1 / -1 for a skipped query"""
        if self.num_q:
            self._finish()
        s = self._state()
        return s["ap"].clone(), s["first"].clone()


def _streamed(who, query, gallery, q_pids, g_pids, q_camids, g_camids, max_rank, metric, slab, precision, clamp=False):
    """both passes over the gallery's descriptors -> the RankAccumulator, every column counted.  clamp: max_rank is
    eval_market1501's, at most the gallery's size (rank.py:110-115)"""
    metric_id = check_metric(metric)
    check_precision(precision)
    Q, dim = check_query(query, who)
    pieces = (gallery,) if isinstance(gallery, torch.Tensor) else gallery
    if not isinstance(pieces, (list, tuple)):
        raise ValueError("%s: the gallery is walked twice, so it must be a [G, d] tensor or a list / tuple of [g, d] "
                         "tensors; a one-shot iterator (got %s) cannot be walked again" % (who, type(gallery).__name__))
    G = count_rows(pieces, dim, who)
    if clamp and G < max_rank:
        max_rank = G
        print('Note: number of gallery samples is quite small, got {}'.format(G))
        if max_rank < 1:
            raise ValueError("%s: the gallery is empty" % who)
    slab = check_slab(slab, Q, who)
    q_pids = host_labels(q_pids, "q_pids", Q, who)
    g_pids = host_labels(g_pids, "g_pids", G, who)
    acc = RankAccumulator(q_pids, q_camids, g_pids, g_camids, max_rank)
    if Q == 0 or G == 0 or acc.match_columns.size == 0:      # nothing to rank: every query is skipped
        acc.num_collected = acc.match_columns.size
        acc.seal()
        acc._claim(0, G)
        return acc
    precision, cdt = _dist._resolve(precision, query.dtype)
    distances = SlabDistances(_lib.require_gpu(), query, metric_id, cdt, precision, acc.device)
    # ---- pass 1: the rows of match_columns, piece by piece
    mc, base = acc.match_columns, 0
    for piece in pieces:
        g = int(piece.shape[0])
        local = mc[np.searchsorted(mc, base):np.searchsorted(mc, base + g)] - base
        for lo in range(0, local.size, slab):
            pick, rows = local[lo:lo + slab], None             # the previous slab's rows go before the next ones come
            if pick[-1] - pick[0] + 1 == pick.size:            # a run of neighbours (every row, on a gallery without
                rows = piece[int(pick[0]):int(pick[-1]) + 1]   # distractors): a view, nothing is gathered
            else:
                rows = piece.detach().index_select(0, torch.from_numpy(pick).to(piece.device))
            acc._collect(*distances.stage(rows))
        base += g
    acc.seal()
    # ---- pass 2: every gallery row, in slabs
    for base, rows in walk(pieces, slab, dim, who):
        acc._claim(base, rows.shape[0])
        acc._count(*distances.stage(rows), base)
    return acc


def rank_counts_streamed(query, gallery, q_pids, g_pids, q_camids, g_camids, max_rank=20, metric='euclidean', slab=None,
                         precision=None):
    """rank_counts(compute_distance_matrix(query, gallery, metric, precision), ...) without the matrix:
    (cmc_counts int64[max_rank], num_valid_q, AP sum), additive over disjoint query sets.  max_rank is the caller's
    (clamp it to the gallery's size first, as eval_market1501 does); arguments as evaluate_rank_streamed's."""
    acc = _streamed("rank_counts_streamed", query, gallery, q_pids, g_pids, q_camids, g_camids, max_rank, metric, slab,
                    precision)
    return acc.result()


def evaluate_rank_streamed(query, gallery, q_pids, g_pids, q_camids, g_camids, max_rank=20, metric='euclidean',
                           slab=None, precision=None):
    """evaluate_rank(compute_distance_matrix(query, gallery, metric, precision), q_pids, g_pids, q_camids, g_camids,
    max_rank) -- the Market1501 protocol -- without the [Q, G] matrix.  -> (cmc float32[max_rank], mAP float).

    query: [Q, d] tensor.  gallery: a [G, d] tensor, on the device or on the host, or a list / tuple of [g_i, d] tensors
    (device and host mixed, empty pieces allowed).  It is walked twice, so a one-shot iterator is a ValueError.  Pass 1
    gathers the rows whose identity occurs among the queries; pass 2 cuts every piece into slabs of at most `slab` rows
    (default_slab_rows(Q) by default); only one slab of a host piece is on the device at a time.  metric and precision
    are compute_distance_matrix's."""
    acc = _streamed("evaluate_rank_streamed", query, gallery, q_pids, g_pids, q_camids, g_camids, max_rank, metric, slab,
                    precision, clamp=True)
    return finish_counts(*acc.result())
