"""Ranked retrieval on the device: the k nearest gallery entries of every query (ieee_rank_topk), the ranking
torchreid/utils/reidtools.py:49 gets from a host argsort of the whole distance matrix."""
import torch

from .. import _lib
from ._stream import TOPK_MAX, check_k, check_labels_all_or_none, device_matrix  # noqa: F401
from .rank import _i32


def rank_topk(distmat, k, q_pids=None, g_pids=None, q_camids=None, g_camids=None):
    """-> (indices int64 [num_q, k], distances float32 [num_q, k]) on the distance matrix's device.

    Each row lists the k smallest kept entries in ascending (distance, gallery index) order -- a stable argsort of the
    kept row, -0.0 equal to +0.0, NaN after +inf.  With all four label arrays given, an entry with the query's identity
    and camera is not kept (reidtools.py:110-112).  A row with fewer than k kept entries ends in index -1 / +inf.
    distmat: a CUDA tensor (a row-strided slice is read in place) or a numpy array (copied to the device once)."""
    given = check_labels_all_or_none(q_pids, g_pids, q_camids, g_camids, "rank_topk")
    k = check_k(k, "rank_topk")
    if getattr(distmat, "ndim", None) != 2:
        raise ValueError("rank_topk: distmat must be 2-D, got shape %s" % (tuple(getattr(distmat, "shape", ())),))
    lib = _lib.require_gpu()
    d, ldd = device_matrix(distmat)
    num_q, num_g = d.shape
    dev = d.device
    idx = torch.empty((num_q, k), dtype=torch.int32, device=dev)
    dist = torch.empty((num_q, k), dtype=torch.float32, device=dev)
    if given:
        qp, gp = _i32(q_pids, "q_pids", dev), _i32(g_pids, "g_pids", dev)
        qc, gc = _i32(q_camids, "q_camids", dev), _i32(g_camids, "g_camids", dev)
        if qp.numel() != num_q or qc.numel() != num_q or gp.numel() != num_g or gc.numel() != num_g:
            raise ValueError("rank_topk: label lengths (%d, %d, %d, %d) do not match distmat %s"
                             % (qp.numel(), gp.numel(), qc.numel(), gc.numel(), tuple(d.shape)))
    else:
        qp = gp = qc = gc = None
    if num_q:
        _lib.check(lib.ieee_rank_topk(_lib.ptr(d), ldd, num_q, num_g, _lib.ptr(qp), _lib.ptr(gp),
                                      _lib.ptr(qc), _lib.ptr(gc), 1 if given else 0, k, _lib.ptr(idx), _lib.ptr(dist),
                                      _lib.stream()))
    return idx.long(), dist
