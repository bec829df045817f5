"""Gallery search without the [Q, G] distance matrix: the gallery goes by in column slabs, each slab's distances are
written into one reused [Q, slab] buffer by the distance-matrix GEMM and folded into a running top-k list by
ieee_rank_topk_merge.  The result is rank_topk's for the whole matrix -- indices equal, distances equal bit for bit --
while device memory holds one slab.  The reference has nothing of the kind (reidtools.py:49 argsorts the whole matrix on
the host)."""
import torch

from .. import _lib
from . import distance as _dist
from ._stream import (SLAB_BUDGET_BYTES, TOPK_CHUNK, SlabDistances, as_pieces, check_device, check_k,  # noqa: F401
                      check_labels_all_or_none, check_metric, check_precision, check_query, check_slab, count_rows,
                      default_slab_rows, device_matrix, host_labels, on_device, walk)

# ieee_rank_topk_merge refuses a slab that ends at or beyond this gallery index (ieee_amd/csrc/topk.hip)
TOPK_MERGE_INDEX_LIMIT = (1 << 31) - 3 * TOPK_CHUNK


class TopKAccumulator(object):
    """The k nearest kept gallery entries of num_q queries, over a gallery whose distances arrive in column slabs.

    add() merges one [num_q, g] slab; its columns are gallery entries num_seen ... num_seen + g - 1.  result() is what
    rank_topk returns for the slabs side by side: ascending (distance, gallery index), -0.0 equal to +0.0, NaN after
    +inf, the stored distances with their own bits, -1 / +inf where a row has fewer than k kept entries.  With q_pids
    and q_camids given, every add() needs the slab's g_pids and g_camids and an entry with the query's identity and
    camera is not kept; without them no add() may bring labels.  merge() is add() for a caller whose slab and labels
    are on the device in the kernel's form already; state() hands out the running lists themselves."""

    def __init__(self, num_q, k, q_pids=None, q_camids=None, device=None):
        who = "TopKAccumulator"
        if isinstance(num_q, bool) or int(num_q) != num_q or num_q < 0:
            raise ValueError("%s: num_q must be a non-negative integer, got %r" % (who, num_q))
        self.num_q, self.k = int(num_q), check_k(k, who)
        if (q_pids is None) != (q_camids is None):
            raise ValueError("%s: give both q_pids and q_camids, or neither" % who)
        self.filtered = q_pids is not None
        if self.filtered:
            q_pids = host_labels(q_pids, "q_pids", self.num_q, who)
            q_camids = host_labels(q_camids, "q_camids", self.num_q, who)
        self.device = check_device(device, who)
        self._lib = _lib.require_gpu()
        self._qp = on_device(q_pids, self.device) if self.filtered else None
        self._qc = on_device(q_camids, self.device) if self.filtered else None
        self._idx = torch.full((self.num_q, self.k), -1, dtype=torch.int32, device=self.device)
        self._dist = torch.full((self.num_q, self.k), float("inf"), dtype=torch.float32, device=self.device)
        self.num_seen = 0

    def add(self, dist_slab, g_pids=None, g_camids=None):
        who = "TopKAccumulator.add"
        if getattr(dist_slab, "ndim", None) != 2 or dist_slab.shape[0] != self.num_q:
            raise ValueError("%s: the slab must be [%d, g], got shape %s"
                             % (who, self.num_q, tuple(getattr(dist_slab, "shape", ()))))
        g = int(dist_slab.shape[1])
        if (g_pids is None) != (g_camids is None) or (g_pids is not None) != self.filtered:
            raise ValueError("%s: the accumulator was made %s query labels, so every slab comes %s g_pids and g_camids"
                             % ((who,) + (("with", "with") if self.filtered else ("without", "without"))))
        if self.filtered:
            g_pids = host_labels(g_pids, "g_pids", g, who)
            g_camids = host_labels(g_camids, "g_camids", g, who)
        if self.num_seen + g >= TOPK_MERGE_INDEX_LIMIT:
            raise ValueError("%s: %d + %d gallery entries are beyond the index range (%d)"
                             % (who, self.num_seen, g, TOPK_MERGE_INDEX_LIMIT))
        self.merge(*device_matrix(dist_slab, self.device, g), g, on_device(g_pids, self.device) if self.filtered else None,
                   on_device(g_camids, self.device) if self.filtered else None)

    def merge(self, buf, ldd, n, g_pids=None, g_camids=None):
        """buf: fp32 on the device, unit column stride, row stride ldd >= n, its first n columns the slab (None when
        there are no queries or n is 0); g_pids, g_camids: int32 [n] on the device, or None without query labels"""
        if self.num_q and n:
            _lib.check(self._lib.ieee_rank_topk_merge(_lib.ptr(buf), ldd, self.num_q, n, self.num_seen,
                                                      _lib.ptr(self._qp), _lib.ptr(g_pids), _lib.ptr(self._qc),
                                                      _lib.ptr(g_camids), 1 if self.filtered else 0, self.k,
                                                      _lib.ptr(self._idx), _lib.ptr(self._dist), _lib.stream()))
        self.num_seen += n

    def state(self):
        """-> (indices int32 [num_q, k], distances float32 [num_q, k]): the live lists, which a later merge changes"""
        return self._idx, self._dist

    def result(self):
        """-> (indices int64 [num_q, k], distances float32 [num_q, k]) on the device, copies of the state"""
        return self._idx.long(), self._dist.clone()


def search_topk(query, gallery, k, metric='euclidean', q_pids=None, g_pids=None, q_camids=None, g_camids=None,
                slab=None, precision=None):
    """The k nearest kept gallery descriptors of every query descriptor, without the [Q, G] matrix.
    -> (indices int64 [Q, k], distances float32 [Q, k]) on the device, as rank_topk(compute_distance_matrix(query,
    gallery, metric, precision), k, ...) lists them.

    query: [Q, d] tensor.  gallery: a [G, d] tensor, on the device or on the host, or any iterable of [g_i, d] tensors
    (device and host mixed, empty pieces allowed, a generator is consumed once).  Every piece is cut into slabs of at
    most `slab` rows (default_slab_rows(Q) by default); only one slab of a host piece is on the device at a time.
    metric and precision are compute_distance_matrix's.  g_pids / g_camids cover the whole gallery in order, all four
    label arrays or none; pieces that run past the labels, or stop short of them, are a ValueError."""
    who = "search_topk"
    k = check_k(k, who)
    metric_id = check_metric(metric)
    check_precision(precision)
    Q, dim = check_query(query, who)
    given = check_labels_all_or_none(q_pids, g_pids, q_camids, g_camids, who)
    slab = check_slab(slab, Q, who)
    pieces = as_pieces(gallery, who)
    known = None                                        # the gallery's length, where it can be had without consuming it
    if isinstance(pieces, (list, tuple)):
        known = count_rows(pieces, dim, who)
        if known >= TOPK_MERGE_INDEX_LIMIT:
            raise ValueError("%s: %d gallery entries are beyond the index range (%d)" % (who, known, TOPK_MERGE_INDEX_LIMIT))
    if given:
        g_pids = host_labels(g_pids, "g_pids", None, who)
        g_camids = host_labels(g_camids, "g_camids", g_pids.size, who)
        if known is not None and g_pids.size != known:
            raise ValueError("%s: %d gallery labels for %d gallery rows" % (who, g_pids.size, known))
    acc = TopKAccumulator(Q, k, q_pids, q_camids)      # the query labels' checks, then the device
    precision, cdt = _dist._resolve(precision, query.dtype)
    distances = SlabDistances(acc._lib, query, metric_id, cdt, precision, acc.device)
    if given:
        g_pids, g_camids = on_device(g_pids, acc.device), on_device(g_camids, acc.device)

    def arrived(base, piece):                           # a one-shot gallery's length shows only as its pieces arrive
        if given and base + piece.shape[0] > g_pids.numel():
            raise ValueError("%s: the gallery runs past its %d labels" % (who, g_pids.numel()))
        if base + piece.shape[0] >= TOPK_MERGE_INDEX_LIMIT:
            raise ValueError("%s: more than %d gallery entries" % (who, TOPK_MERGE_INDEX_LIMIT))

    for base, rows in walk(pieces, slab, dim, who, arrived):
        n = rows.shape[0]
        if Q == 0:
            acc.merge(None, 0, n)                       # counted, so that the labels' length is still checked
            continue
        acc.merge(*distances.stage(rows), *((g_pids[base:base + n], g_camids[base:base + n]) if given else ()))
    if given and acc.num_seen != g_pids.numel():
        raise ValueError("%s: %d gallery labels for %d gallery rows" % (who, g_pids.numel(), acc.num_seen))
    return acc.result()
