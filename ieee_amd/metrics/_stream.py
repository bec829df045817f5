"""What the retrieval drivers share (search.py, rank_stream.py, rank.py, topk.py, ../rerank.py): the argument checks,
each once and each before a device is needed; device_matrix, the one way a distance matrix or slab reaches the device
as fp32; SlabDistances, the one slab-distance stage of the streamed paths; walk, a gallery cut into slabs."""
import numpy as np
import torch

from . import distance as _dist

TOPK_MAX = 1024                    # ieee_amd/csrc/topk.hip: the longest list a workgroup keeps
TOPK_CHUNK = 2048                  # ieee_amd/csrc/topk.hip: the kernel streams a row in chunks of this many distances
# The distance buffer of one slab.  The first value was 128 MiB, half of the Infinity Cache, so that what the GEMM
# wrote would still be cached when the merge reads it; measured, that is not what decides (LABNOTES.md R19.1, 10 000 x
# 100 000, d = 2304, fp32, k = 10, one MI355X, medians of 7 interleaved rounds): slab 2048 (that budget's) 43.9 ms,
# 8192 39.6 ms, 32768 37.9 ms, the whole gallery 37.5 ms = the two-step path.  Every slab costs a query-norm pass, four
# launches and a GEMM that starts and drains once more, so larger is faster; 1250 MiB is 32768 rows at 10 000 queries,
# within 1 % of no slabs at a third of the memory.
SLAB_BUDGET_BYTES = 1250 << 20
_METRIC_ID = {"euclidean": 0, "cosine": 1}


def default_slab_rows(num_q):
    """Gallery rows per slab for num_q queries: the largest multiple of TOPK_CHUNK whose [num_q, rows] fp32 buffer
    fits SLAB_BUDGET_BYTES, and at least TOPK_CHUNK."""
    rows = SLAB_BUDGET_BYTES // (4 * max(int(num_q), 1)) // TOPK_CHUNK * TOPK_CHUNK
    return max(rows, TOPK_CHUNK)


# ---- the checks: all on the host, none needs the library or a device ---------------------------------------------------
def check_k(k, who):
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= TOPK_MAX:
        raise ValueError("%s: k must be an integer in [1, %d], got %r" % (who, TOPK_MAX, k))
    return int(k)


def check_slab(slab, num_q, who, name="slab"):
    if slab is None:
        return default_slab_rows(num_q)
    if isinstance(slab, bool) or int(slab) != slab or slab < 1:
        raise ValueError("%s: %s must be a positive integer, got %r" % (who, name, slab))
    return int(slab)


def check_labels_all_or_none(q_pids, g_pids, q_camids, g_camids, who):
    """-> whether the four label arrays are given"""
    given = sum(x is not None for x in (q_pids, g_pids, q_camids, g_camids))
    if given not in (0, 4):
        raise ValueError("%s: give all four of q_pids, g_pids, q_camids, g_camids, or none (got %d)" % (who, given))
    return given == 4


def check_metric(metric):
    """-> the library's metric id"""
    if metric not in _METRIC_ID:
        raise ValueError('Unknown distance metric: {}. Please choose either "euclidean" or "cosine"'.format(metric))
    return _METRIC_ID[metric]


def check_precision(precision):
    if precision is not None and precision not in _dist.PRECISIONS:
        raise ValueError("Unknown distmat precision: {}. Choose one of {}".format(precision, _dist.PRECISIONS))


def check_query(query, who):
    """-> (Q, d)"""
    if not isinstance(query, torch.Tensor) or query.dim() != 2:
        raise ValueError("%s: query must be a [Q, d] tensor, got %s"
                         % (who, tuple(query.shape) if isinstance(query, torch.Tensor) else type(query).__name__))
    return query.shape


def check_piece(piece, dim, who):
    if not isinstance(piece, torch.Tensor) or piece.dim() != 2 or piece.shape[1] != dim:
        raise ValueError("%s: the gallery and every piece of it must be a [g, %d] tensor, got %s"
                         % (who, dim, tuple(piece.shape) if isinstance(piece, torch.Tensor) else type(piece).__name__))


def check_device(device, who):
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise ValueError("%s: device must be a CUDA device, got %s" % (who, device))
    return device


def host_labels(x, name, n, who):
    """-> a contiguous int32 numpy array, on the host: range and length (n, unless None) checked"""
    a = np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x).reshape(-1)
    who = who + ": " if who else ""
    if a.size and (a.max() > np.iinfo(np.int32).max or a.min() < np.iinfo(np.int32).min):
        raise ValueError("%s%s does not fit int32" % (who, name))
    if n is not None and a.size != n:
        raise ValueError("%s%s has %d entries, expected %d" % (who, name, a.size, n))
    return np.ascontiguousarray(a.astype(np.int32))


def on_device(x, device):
    return torch.from_numpy(x).to(device)


# ---- distances on their way to a kernel --------------------------------------------------------------------------------
def device_matrix(x, device=None, cols=None):
    """A [rows, cols] distance matrix or slab, tensor or numpy array -> (d, ldd): fp32 on the device with unit column
    stride and row stride ldd >= cols, copied only when it is not in that form already (a row-strided slice is read in
    place; a column-strided view, or one whose rows overlap, is not).  device None: where x is when that is a GPU,
    else the current GPU."""
    if device is None:
        device = x.device if isinstance(x, torch.Tensor) and x.is_cuda else "cuda"
    if isinstance(x, torch.Tensor):
        d = x.to(device)
    else:
        d = np.ascontiguousarray(x, dtype=np.float32)
        d = torch.from_numpy(d if d.flags.writeable else d.copy()).to(device)      # from_numpy wants a writable array
    d = d.to(torch.float32)
    if cols is None:
        cols = d.shape[-1]
    if d.stride(-1) != 1 or d.stride(0) < cols:
        d = d.contiguous()
    return d, max(d.stride(0), cols)


class SlabDistances(object):
    """The slab-distance stage of the streamed paths: the distances of query_rows [Q, d] to one slab of rows after
    another, each written by the distance-matrix GEMM into one reused [Q, slab] fp32 buffer.  metric_id,
    compute_dtype and precision are distance._launch's; both sides are prepared alike (on the device, compute_dtype,
    contiguous, the feature axis padded to 8), the query side once."""

    def __init__(self, lib, query_rows, metric_id, compute_dtype, precision, device):
        self.lib, self.metric_id, self.cdt, self.precision, self.device = lib, metric_id, compute_dtype, precision, device
        self.q = self._prepare(query_rows)
        self._buf = self._work = None

    def _prepare(self, rows):
        return _dist._pad8(rows.detach().to(self.device).to(self.cdt).contiguous())

    def set_query(self, query_rows):
        """Another query side of at most as many rows as the first: the distance buffer and the workspace stay, so a
        driver that walks its rows block by block (cluster.py) allocates them once, not once per block."""
        q = self._prepare(query_rows)
        if self._buf is not None and q.shape[0] > self._buf.shape[0]:
            self._buf = None
        self.q = q

    def stage(self, rows):
        """rows [n, d], on the host or on the device -> (buf, ldd, n): buf[:, :n] holds the distances, row stride ldd.
        The next call overwrites them."""
        rows = self._prepare(rows)
        Q, n = self.q.shape[0], rows.shape[0]
        # One buffer, as wide as the widest slab so far (rows stay 16-byte aligned), and one GEMM workspace.  Either
        # grows only when too small, and the old one is released BEFORE its successor is allocated: the peak-memory
        # bounds of the streamed paths are one buffer, not two.  For the same reason the buffer is returned with no
        # other name bound to it; a caller that keeps it across calls keeps a replaced buffer alive.
        if self._buf is None or self._buf.shape[1] < n:
            self._buf = None
            self._buf = torch.empty((Q, (n + 3) // 4 * 4), dtype=torch.float32, device=self.device)
        need = _dist._workspace_bytes(self.lib, Q, n, self.q.shape[1], self.cdt, self.precision)
        if self._work is None or self._work.numel() < need:
            self._work = None
            self._work = torch.empty(need, dtype=torch.uint8, device=self.device)
        _dist._launch(self.lib, self.q, rows, self.metric_id, self.cdt, self.precision, self._buf, self._buf.shape[1],
                      self._work)
        return self._buf, self._buf.shape[1], n


# ---- a gallery, piece by piece -----------------------------------------------------------------------------------------
def as_pieces(gallery, who):
    """a [G, d] tensor is one piece; anything else must be iterable (its pieces are checked when they are reached)"""
    if isinstance(gallery, torch.Tensor):
        return (gallery,)
    if isinstance(gallery, (str, bytes)) or not hasattr(gallery, "__iter__"):
        raise ValueError("%s: gallery must be a [G, d] tensor or an iterable of [g, d] tensors, got %s"
                         % (who, type(gallery).__name__))
    return gallery


def count_rows(pieces, dim, who):
    """the rows of a list or tuple of pieces, every piece checked"""
    for piece in pieces:
        check_piece(piece, dim, who)
    return sum(int(piece.shape[0]) for piece in pieces)


def walk(pieces, slab, dim, who, arrived=None):
    """Yields (base, rows): the gallery -- a [G, d] tensor, a list or tuple of [g, d] tensors or a one-shot iterable of
    them -- in order, every piece cut into slabs of at most `slab` rows; rows is a view of the piece, base the gallery
    index of its first row.  A piece is checked when it is reached, then arrived(base, piece) is called, if given."""
    base = 0
    for piece in as_pieces(pieces, who):
        check_piece(piece, dim, who)
        if arrived is not None:
            arrived(base, piece)
        for lo in range(0, piece.shape[0], slab):
            yield base + lo, piece[lo:lo + slab]
        base += piece.shape[0]
