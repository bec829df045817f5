"""k-reciprocal re-ranking on the device, same call as the reference's
torchreid/utils/rerank.py::re_ranking(q_g_dist, q_q_dist, g_g_dist, k1=20, k2=6, lambda_value=0.3); and GNN re-ranking,
the reference's torchreid/utils/GPU-Re-Ranking/gnn_reranking.py::gnn_reranking(X_q, X_g, k1, k2), plus the same result as a
distance matrix (gnn_distmat)."""
import os

import numpy as np
import torch

from . import _lib


def _dev(x):
    if isinstance(x, torch.Tensor):
        t = x if x.is_cuda else x.cuda()
    else:
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    return t.to(torch.float32).contiguous()


DENSE_LIMIT = 46000      # the dense formulation holds three (Q+G)^2 fp32 work matrices: Q+G below this only


def _inputs(q_g_dist, q_q_dist, g_g_dist):
    qg, qq, gg = _dev(q_g_dist), _dev(q_q_dist), _dev(g_g_dist)
    Q, G = qg.shape
    if qq.shape != (Q, Q) or gg.shape != (G, G):
        raise ValueError("re_ranking: expected q_q_dist %s and g_g_dist %s, got %s and %s"
                         % ((Q, Q), (G, G), tuple(qq.shape), tuple(gg.shape)))
    return qg, qq, gg, Q, G


def _sparse(lib, qg, qq, gg, Q, G, k1, k2, lambda_value):
    """ieee_rerank_sparse; returns (out, workspace) so that tests can read the intermediates (sparse_layout)"""
    nbytes = int(lib.ieee_rerank_sparse_workspace_bytes(Q, G, int(k1), int(k2)))
    if nbytes < 0:
        _lib.check(-1)
    out = torch.empty((Q, G), dtype=torch.float32, device=qg.device)
    work = torch.empty(nbytes, dtype=torch.uint8, device=qg.device)
    _lib.check(lib.ieee_rerank_sparse(_lib.ptr(qg), _lib.ptr(qq), _lib.ptr(gg), Q, G, int(k1), int(k2),
                                      float(lambda_value), _lib.ptr(out), _lib.ptr(work), nbytes, _lib.stream()))
    return out, work


def sparse_layout(Q, G, k1, k2):
    """where ieee_rerank_sparse keeps its intermediates in the workspace (include/ieee_amd.h)"""
    import ctypes
    fields = (ctypes.c_int64 * 11)()
    _lib.check(_lib.load().ieee_rerank_sparse_layout(Q, G, int(k1), int(k2), ctypes.cast(fields, ctypes.c_void_p)))
    names = ("K", "capV", "capVq", "rank", "V_n", "V_idx", "V_val", "Vq_n", "Vq_idx", "Vq_val", "colmax")
    return dict(zip(names, (int(f) for f in fields)))


def re_ranking(q_g_dist, q_q_dist, g_g_dist, k1=20, k2=6, lambda_value=0.3, formulation=None):
    """returns the re-ranked [Q, G] distance matrix: a CUDA tensor when q_g_dist is one, else a numpy array
    (the reference's type, rerank.py:112-113).  formulation: "dense" (ieee_rerank, three (Q+G)^2 work matrices),
    "sparse" (ieee_rerank_sparse: the same bits, no (Q+G)^2 workspace) or None: dense below Q+G = 46 000, else
    sparse.  The keyword is this package's; the reference has none."""
    if formulation not in (None, "dense", "sparse"):
        raise ValueError("re_ranking: formulation must be None, 'dense' or 'sparse', got %r" % (formulation,))
    lib = _lib.require_gpu()
    qg, qq, gg, Q, G = _inputs(q_g_dist, q_q_dist, g_g_dist)
    if formulation is None:
        formulation = "dense" if Q + G < DENSE_LIMIT else "sparse"
    if formulation == "sparse":
        out, _ = _sparse(lib, qg, qq, gg, Q, G, k1, k2, lambda_value)
    else:
        out = torch.empty((Q, G), dtype=torch.float32, device=qg.device)
        nbytes = int(lib.ieee_rerank_workspace_bytes(Q, G, int(k1)))
        work = torch.empty(nbytes, dtype=torch.uint8, device=qg.device)
        _lib.check(lib.ieee_rerank(_lib.ptr(qg), _lib.ptr(qq), _lib.ptr(gg), Q, G, int(k1), int(k2),
                                   float(lambda_value), _lib.ptr(out), _lib.ptr(work), nbytes, _lib.stream()))
    if isinstance(q_g_dist, torch.Tensor) and q_g_dist.is_cuda:
        return out
    return out.cpu().numpy()


# ---- GNN re-ranking (the reference's torchreid/utils/GPU-Re-Ranking/gnn_reranking.py) ----------------------------------
_GNN_PRECISION = {"fp32": 0, "bf16x3": 6, "bf16x2": 3, "f16x2": 2}     # 0, or IEEE_SPLIT_* in include/ieee_amd.h


def _gnn(x_q, x_g, k1, k2, precision=None):
    """ieee_gnn_rerank; returns (distmat, workspace) so that tests can read the intermediates (gnn_layout)"""
    lib = _lib.require_gpu()
    if precision is None:
        precision = os.environ.get("IEEE_DISTMAT_PRECISION", "fp32")
    if precision not in _GNN_PRECISION:
        raise ValueError("gnn re-ranking: precision must be one of %s, got %r" % (sorted(_GNN_PRECISION), precision))
    q, g = _dev(x_q), _dev(x_g)
    if q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1]:
        raise ValueError("gnn re-ranking: expected X_q [Q, d] and X_g [G, d], got %s and %s" % (tuple(q.shape), tuple(g.shape)))
    Q, G = q.shape[0], g.shape[0]
    d = (q.shape[1] + 7) // 8 * 8    # kernels move 16-byte chunks: zero columns change no inner product (metrics/distance.py)
    nbytes = int(lib.ieee_gnn_rerank_workspace_bytes(Q, G, d, int(k1), int(k2), _GNN_PRECISION[precision]))
    if nbytes < 0:
        _lib.check(-1)
    need = nbytes + (Q * G + (Q + G) * d) * 4
    free = torch.cuda.mem_get_info()[0]
    if need > free:
        raise RuntimeError("gnn re-ranking is dense: N = Q + G = %d rows need two N x N fp32 work matrices, %d bytes "
                           "with the features and the output, and the device has %d bytes free" % (Q + G, need, free))
    x = torch.zeros((Q + G, d), dtype=torch.float32, device=q.device)    # one array: the scores are then one GEMM
    x[:Q, :q.shape[1]] = q
    x[Q:, :g.shape[1]] = g
    out = torch.empty((Q, G), dtype=torch.float32, device=q.device)
    work = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    _lib.check(lib.ieee_gnn_rerank(_lib.ptr(x), _lib.ptr(x[Q:]), Q, G, d, int(k1), int(k2), _GNN_PRECISION[precision],
                                   _lib.ptr(out), _lib.ptr(work), nbytes, _lib.stream()))
    return out, work


def gnn_layout(Q, G, d, k1, k2, precision="fp32"):
    """where ieee_gnn_rerank keeps its intermediates in the workspace (include/ieee_amd.h); d as passed to the library,
    i.e. rounded up to a multiple of 8"""
    import ctypes
    fields = (ctypes.c_int64 * 7)()
    _lib.check(_lib.load().ieee_gnn_rerank_layout(Q, G, d, int(k1), int(k2), _GNN_PRECISION[precision],
                                                  ctypes.cast(fields, ctypes.c_void_p)))
    return dict(zip(("ld", "rank", "S", "sumsq", "M0", "M1", "rows"), (int(f) for f in fields)))


def gnn_distmat(X_q, X_g, k1=26, k2=7, precision=None):
    """GNN re-ranking as a [Q, G] fp32 distance matrix, 1 - similarity, so that evaluate_rank, rank_topk and
    visualize_ranked_results take it like any other: a CUDA tensor when X_q is one, else a numpy array.  The features
    are used as they are (plain inner products, as in the reference): hand in L2-normalised rows, as the reference's
    driver does (main.py) -- on rows that are not normalised the raw inner product is a poor first ranking.  Defaults
    are that driver's Market-1501 values.  Where the reference leaves the result open: ties are broken by the smaller
    index, and a row whose propagated vector is all zero (e.g. an all-zero feature row) has similarity 0 to everything,
    not the reference's NaN.  precision: as in metrics.distance (fp32, or a split scheme for the two GEMMs).  Dense:
    two (Q+G)^2 fp32 work matrices; raises RuntimeError when the device has not that much free."""
    out, _ = _gnn(X_q, X_g, k1, k2, precision)
    if isinstance(X_q, torch.Tensor) and X_q.is_cuda:
        return out
    return out.cpu().numpy()


def gnn_reranking(X_q, X_g, k1, k2):
    """the reference's gnn_reranking(X_q, X_g, k1, k2) (GPU-Re-Ranking/gnn_reranking.py:27-59): L, an integer numpy
    array [Q, G], row i the gallery indices of query i best first (a stable sort of gnn_distmat's rows: equal
    similarities in index order).  CPU or CUDA tensors, or numpy arrays.  See gnn_distmat for what is defined here
    that the reference leaves open (ties; zero rows give similarity 0, not NaN)."""
    out, _ = _gnn(X_q, X_g, k1, k2)
    return torch.sort(out, dim=1, stable=True)[1].cpu().numpy()
