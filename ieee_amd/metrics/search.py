"""Gallery search without the [Q, G] distance matrix: the gallery goes by in column slabs, each slab's distances are
written into one reused [Q, slab] buffer by the distance-matrix GEMM and folded into a running top-k list by
ieee_rank_topk_merge.  The result is rank_topk's for the whole matrix -- indices equal, distances equal bit for bit --
while device memory holds one slab.  The reference has nothing of the kind (reidtools.py:49 argsorts the whole matrix on
the host)."""
import numpy as np
import torch

from .. import _lib
from . import distance as _dist
from .topk import TOPK_MAX

TOPK_CHUNK = 2048                  # ieee_amd/csrc/topk.hip: the kernel streams a row in chunks of this many distances
# The distance buffer of one slab.  The first value was 128 MiB, half of the Infinity Cache, so that what the GEMM
# wrote would still be cached when the merge reads it; measured, that is not what decides (LABNOTES.md R19.1, 10 000 x
# 100 000, d = 2304, fp32, k = 10, one MI355X, medians of 7 interleaved rounds): slab 2048 (that budget's) 43.9 ms,
# 8192 39.6 ms, 32768 37.9 ms, the whole gallery 37.5 ms = the two-step path.  Every slab costs a query-norm pass, four
# launches and a GEMM that starts and drains once more, so larger is faster; 1250 MiB is 32768 rows at 10 000 queries,
# within 1 % of no slabs at a third of the memory.
SLAB_BUDGET_BYTES = 1250 << 20
_INDEX_LIMIT = (1 << 31) - 3 * TOPK_CHUNK


def default_slab_rows(num_q):
    """Gallery rows per slab for num_q queries: the largest multiple of TOPK_CHUNK whose [num_q, rows] fp32 buffer
    fits SLAB_BUDGET_BYTES, and at least TOPK_CHUNK."""
    rows = SLAB_BUDGET_BYTES // (4 * max(int(num_q), 1)) // TOPK_CHUNK * TOPK_CHUNK
    return max(rows, TOPK_CHUNK)


def _check_k(k, who):
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= TOPK_MAX:
        raise ValueError("%s: k must be an integer in [1, %d], got %r" % (who, TOPK_MAX, k))
    return int(k)


def _host_labels(x, name, n, who):
    """-> a contiguous int32 numpy array, on the host: range and length checked before any device is needed"""
    a = np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x).reshape(-1)
    if a.size and (a.max() > np.iinfo(np.int32).max or a.min() < np.iinfo(np.int32).min):
        raise ValueError("%s: %s does not fit int32" % (who, name))
    if n is not None and a.size != n:
        raise ValueError("%s: %s has %d entries, expected %d" % (who, name, a.size, n))
    return np.ascontiguousarray(a.astype(np.int32))


def _on(x, device):
    return torch.from_numpy(x).to(device)


class TopKAccumulator(object):
    """The k nearest kept gallery entries of num_q queries, over a gallery whose distances arrive in column slabs.

    add() merges one [num_q, g] slab; its columns are gallery entries num_seen ... num_seen + g - 1.  result() is what
    rank_topk returns for the slabs side by side: ascending (distance, gallery index), -0.0 equal to +0.0, NaN after
    +inf, the stored distances with their own bits, -1 / +inf where a row has fewer than k kept entries.  With q_pids
    and q_camids given, every add() needs the slab's g_pids and g_camids and an entry with the query's identity and
    camera is not kept; without them no add() may bring labels."""

    def __init__(self, num_q, k, q_pids=None, q_camids=None, device=None):
        who = "TopKAccumulator"
        if isinstance(num_q, bool) or int(num_q) != num_q or num_q < 0:
            raise ValueError("%s: num_q must be a non-negative integer, got %r" % (who, num_q))
        self.num_q, self.k = int(num_q), _check_k(k, who)
        if (q_pids is None) != (q_camids is None):
            raise ValueError("%s: give both q_pids and q_camids, or neither" % who)
        self.filtered = q_pids is not None
        if self.filtered:
            q_pids = _host_labels(q_pids, "q_pids", self.num_q, who)
            q_camids = _host_labels(q_camids, "q_camids", self.num_q, who)
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise ValueError("%s: device must be a CUDA device, got %s" % (who, self.device))
        self._lib = _lib.require_gpu()
        self._qp = _on(q_pids, self.device) if self.filtered else None
        self._qc = _on(q_camids, self.device) if self.filtered else None
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
            g_pids = _host_labels(g_pids, "g_pids", g, who)
            g_camids = _host_labels(g_camids, "g_camids", g, who)
        if self.num_seen + g >= _INDEX_LIMIT:
            raise ValueError("%s: %d + %d gallery entries are beyond the index range (%d)"
                             % (who, self.num_seen, g, _INDEX_LIMIT))
        if isinstance(dist_slab, torch.Tensor):
            d = dist_slab.to(self.device)
        else:
            d = np.ascontiguousarray(dist_slab, dtype=np.float32)
            d = torch.from_numpy(d if d.flags.writeable else d.copy()).to(self.device)
        d = d.to(torch.float32)
        if g and (d.stride(-1) != 1 or d.stride(0) < g):
            d = d.contiguous()
        self._merge(d, max(d.stride(0), g), g, _on(g_pids, self.device) if self.filtered else None,
                    _on(g_camids, self.device) if self.filtered else None)

    def _merge(self, d, ldd, g, gp, gc):
        """d: fp32 on the device, unit column stride, row stride ldd >= g; gp, gc: int32 [g] on the device or None"""
        if self.num_q and g:
            _lib.check(self._lib.ieee_rank_topk_merge(_lib.ptr(d), ldd, self.num_q, g, self.num_seen, _lib.ptr(self._qp),
                                                      _lib.ptr(gp), _lib.ptr(self._qc), _lib.ptr(gc),
                                                      1 if self.filtered else 0, self.k, _lib.ptr(self._idx),
                                                      _lib.ptr(self._dist), _lib.stream()))
        self.num_seen += g

    def result(self):
        """-> (indices int64 [num_q, k], distances float32 [num_q, k]) on the device, copies of the state"""
        return self._idx.long(), self._dist.clone()


_METRIC_ID = {"euclidean": 0, "cosine": 1}


def _check_piece(piece, dim):
    if not isinstance(piece, torch.Tensor) or piece.dim() != 2 or piece.shape[1] != dim:
        raise ValueError("search_topk: the gallery and every piece of it must be a [g, %d] tensor, got %s"
                         % (dim, tuple(piece.shape) if isinstance(piece, torch.Tensor) else type(piece).__name__))


def _pieces(gallery):
    if isinstance(gallery, torch.Tensor):
        return (gallery,)
    if isinstance(gallery, (str, bytes)) or not hasattr(gallery, "__iter__"):
        raise ValueError("search_topk: gallery must be a [G, d] tensor or an iterable of [g, d] tensors, got %s"
                         % type(gallery).__name__)
    return gallery


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
    k = _check_k(k, who)
    if metric not in _METRIC_ID:
        raise ValueError('Unknown distance metric: {}. Please choose either "euclidean" or "cosine"'.format(metric))
    if precision is not None and precision not in _dist.PRECISIONS:
        raise ValueError("Unknown distmat precision: {}. Choose one of {}".format(precision, _dist.PRECISIONS))
    if not isinstance(query, torch.Tensor) or query.dim() != 2:
        raise ValueError("%s: query must be a [Q, d] tensor, got %s"
                         % (who, tuple(query.shape) if isinstance(query, torch.Tensor) else type(query).__name__))
    Q, dim = query.shape
    labels = (q_pids, g_pids, q_camids, g_camids)
    given = sum(x is not None for x in labels)
    if given not in (0, 4):
        raise ValueError("%s: give all four of q_pids, g_pids, q_camids, g_camids, or none (got %d)" % (who, given))
    if slab is None:
        slab = default_slab_rows(Q)
    if isinstance(slab, bool) or int(slab) != slab or slab < 1:
        raise ValueError("%s: slab must be a positive integer, got %r" % (who, slab))
    slab = int(slab)
    pieces = _pieces(gallery)
    known = None                                        # the gallery's length, where it can be had without consuming it
    if isinstance(pieces, (list, tuple)):
        for piece in pieces:
            _check_piece(piece, dim)
        known = sum(int(piece.shape[0]) for piece in pieces)
        if known >= _INDEX_LIMIT:
            raise ValueError("%s: %d gallery entries are beyond the index range (%d)" % (who, known, _INDEX_LIMIT))
    if given:
        g_pids = _host_labels(g_pids, "g_pids", None, who)
        g_camids = _host_labels(g_camids, "g_camids", g_pids.size, who)
        if known is not None and g_pids.size != known:
            raise ValueError("%s: %d gallery labels for %d gallery rows" % (who, g_pids.size, known))
    acc = TopKAccumulator(Q, k, q_pids, q_camids)      # the query labels' checks, then the device
    lib, dev = acc._lib, acc.device
    precision, cdt = _dist._resolve(precision, query.dtype)
    metric_id = _METRIC_ID[metric]
    q = _dist._pad8(query.detach().to(dev).to(cdt).contiguous())
    if given:
        g_pids, g_camids = _on(g_pids, dev), _on(g_camids, dev)
    buf = work = None
    for piece in pieces:
        _check_piece(piece, dim)
        if given and acc.num_seen + piece.shape[0] > g_pids.numel():
            raise ValueError("%s: the gallery runs past its %d labels" % (who, g_pids.numel()))
        if acc.num_seen + piece.shape[0] >= _INDEX_LIMIT:
            raise ValueError("%s: more than %d gallery entries" % (who, _INDEX_LIMIT))
        for lo in range(0, piece.shape[0], slab):
            rows = _dist._pad8(piece[lo:lo + slab].detach().to(dev).to(cdt).contiguous())
            n = rows.shape[0]
            if Q == 0:
                acc.num_seen += n
                continue
            if buf is None or buf.shape[1] < n:        # one buffer, as wide as the widest slab (rows stay 16-byte aligned)
                buf = None                             # the narrower one goes before its successor comes
                buf = torch.empty((Q, (n + 3) // 4 * 4), dtype=torch.float32, device=dev)
            need = _dist._workspace_bytes(lib, Q, n, q.shape[1], cdt, precision)
            if work is None or work.numel() < need:
                work = None
                work = torch.empty(need, dtype=torch.uint8, device=dev)
            _dist._launch(lib, q, rows, metric_id, cdt, precision, buf, buf.shape[1], work)
            at = acc.num_seen
            acc._merge(buf, buf.shape[1], n, g_pids[at:at + n] if given else None, g_camids[at:at + n] if given else None)
    if given and acc.num_seen != g_pids.numel():
        raise ValueError("%s: %d gallery labels for %d gallery rows" % (who, g_pids.numel(), acc.num_seen))
    return acc.result()

