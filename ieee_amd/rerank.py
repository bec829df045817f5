"""k-reciprocal re-ranking on the device, same call as the reference's
torchreid/utils/rerank.py::re_ranking(q_g_dist, q_q_dist, g_g_dist, k1=20, k2=6, lambda_value=0.3)."""
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
