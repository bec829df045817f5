"""k-reciprocal re-ranking on the device, same call as the reference's
torchreid/utils/rerank.py::re_ranking(q_g_dist, q_q_dist, g_g_dist, k1=20, k2=6, lambda_value=0.3); and GNN re-ranking,
the reference's torchreid/utils/GPU-Re-Ranking/gnn_reranking.py::gnn_reranking(X_q, X_g, k1, k2), plus the same result as a
distance matrix (gnn_distmat)."""
import os

import numpy as np
import torch

from . import _lib
from .metrics import _stream
from .metrics import distance as _dist
from .metrics._stream import (SlabDistances, check_k, check_labels_all_or_none, check_metric, check_slab, device_matrix,
                              host_labels, on_device)
from .metrics.search import TopKAccumulator


def _dev(x):
    """device_matrix with the rows back to back: the re-ranking kernels take no row stride"""
    return device_matrix(x)[0].contiguous()


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


# ---- k-reciprocal re-ranking from descriptors (ieee_amd/csrc/rerank_stream.hip): no Q x Q, G x G or (Q+G)^2 tensor ------
RERANK_MAX_K = 64        # rerank_sparse.h: k1 + 1 <= RS_MAXK


def stream_slab_rows(slab_rows, who="re_ranking_features"):
    """-> the rows on either side of one distance GEMM: slab_rows checked, or for None the largest multiple of 128
    whose square fp32 buffer stays within SLAB_BUDGET_BYTES"""
    if slab_rows is None:
        return int((_stream.SLAB_BUDGET_BYTES // 4) ** 0.5) // 128 * 128
    return check_slab(slab_rows, 0, who, "slab_rows")


def stream_pieces(n, slab_rows, cut=None):
    """[0, n) in pieces of at most slab_rows, none across `cut` (the first gallery row of [queries; gallery]): a list
    of (lo, hi)"""
    cuts = [0, n] if cut is None or not 0 < cut < n else [0, cut, n]
    return [(lo, min(lo + slab_rows, hi)) for b, hi in zip(cuts[:-1], cuts[1:]) for lo in range(b, hi, slab_rows)]


def stream_schedule(n, slab_rows, cut=None):
    """The blocks (a0, a1, i0, i1) of the n x n all-pairs matrix in the order the strip passes visit them: for every
    strip of owner columns [i0, i1), every slab of rows [a0, a1).  Every (row, column) pair lies in exactly one block,
    no block is longer than slab_rows on either side, and none crosses `cut`, so one block is one distance GEMM whose
    operands are those of the matrix path."""
    pieces = stream_pieces(n, slab_rows, cut)
    return [(a0, a1, i0, i1) for i0, i1 in pieces for a0, a1 in pieces]


def _stream_checks(X_q, X_g, k1, k2, metric, slab_rows, precision, who):
    """every argument check, on the host, before the library or a device is needed -> (metric_id, Q, G, k1, k2, slab)"""
    metric_id = check_metric(metric)
    if precision is None:
        precision = os.environ.get("IEEE_DISTMAT_PRECISION", "fp32")
    if precision != "fp32":
        raise ValueError("%s: precision must be None or 'fp32' (the bits of the fp32 matrix path are the contract), got %r"
                         % (who, precision))
    sq, sg = tuple(np.shape(X_q)), tuple(np.shape(X_g))
    if len(sq) != 2 or len(sg) != 2 or sq[1] != sg[1]:
        raise ValueError("%s: expected X_q [Q, d] and X_g [G, d], got %s and %s" % (who, sq, sg))
    Q, G = int(sq[0]), int(sg[0])
    for name, v in (("k1", k1), ("k2", k2)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("%s: %s must be an integer, got %r" % (who, name, v))
    k1, k2 = int(k1), int(k2)
    if Q < 1 or G < 1:
        raise ValueError("%s: empty query or gallery set (Q = %d, G = %d)" % (who, Q, G))
    if not (1 <= k1 and k1 + 1 <= RERANK_MAX_K and k1 + 1 <= Q + G < 2 ** 31):
        raise ValueError("%s: k1 = %d out of range (1 .. %d, and k1 + 1 <= Q + G = %d < 2^31)"
                         % (who, k1, RERANK_MAX_K - 1, Q + G))
    if not 1 <= k2 <= k1 + 1:
        raise ValueError("%s: k2 = %d out of range (1 .. k1 + 1 = %d)" % (who, k2, k1 + 1))
    return metric_id, Q, G, k1, k2, stream_slab_rows(slab_rows, who)


def stream_layout(Q, G, k1, k2, slab_rows=None):
    """where the ieee_rerank_stream_* calls keep their intermediates in the workspace (include/ieee_amd.h): sparse_layout's
    fields, then keys (the running lists), strip and range (the longest strip of columns and gallery range)"""
    import ctypes
    fields = (ctypes.c_int64 * 14)()
    _lib.check(_lib.load().ieee_rerank_stream_layout(Q, G, int(k1), int(k2), stream_slab_rows(slab_rows),
                                                     ctypes.cast(fields, ctypes.c_void_p)))
    names = ("K", "capV", "capVq", "rank", "V_n", "V_idx", "V_val", "Vq_n", "Vq_idx", "Vq_val", "colmax", "keys", "strip",
             "range")
    return dict(zip(names, (int(f) for f in fields)))


def _rerank_stream(X_q, X_g, k1, k2, metric, slab_rows, precision, who):
    """steps A - D -> dict(lib, Q, G, slab, x [Q + G, d] (fp32, d padded to 8), metric_id, args (what every
    ieee_rerank_stream_* call ends with), work).  Two sweeps of distance GEMMs over the blocks of stream_schedule, each
    into one reused buffer of at most slab x slab distances, then one gathered-operand GEMM for the members' distances."""
    metric_id, Q, G, k1, k2, slab = _stream_checks(X_q, X_g, k1, k2, metric, slab_rows, precision, who)
    lib = _lib.require_gpu()
    q, g = _dev(X_q), _dev(X_g)
    N, dev = Q + G, q.device
    x = _gnn_features(q, g, (q.shape[1] + 7) // 8 * 8)
    del q, g
    nbytes = int(lib.ieee_rerank_stream_workspace_bytes(Q, G, k1, k2, slab))
    if nbytes < 0:
        _lib.check(-1)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    args = (Q, G, k1, k2, slab, _lib.ptr(work), nbytes)
    _lib.check(lib.ieee_rerank_stream_begin(*args, _lib.stream()))
    pieces = stream_pieces(N, slab, Q)
    longest = max(hi - lo for lo, hi in pieces)
    buf = torch.empty(longest * ((longest + 3) // 4 * 4), dtype=torch.float32, device=dev)
    norms = torch.empty(2 * longest * 4, dtype=torch.uint8, device=dev)

    def block(step, a0, a1, i0, i1):
        # the Q x G block has the query as its row operand wherever it is used (cosine's epilogue is not symmetric):
        # as orig[a in G][i in Q] it is produced [i][a] and read transposed
        transposed = a0 >= Q and i1 <= Q
        rows, cols = ((i0, i1), (a0, a1)) if transposed else ((a0, a1), (i0, i1))
        ld = (cols[1] - cols[0] + 3) // 4 * 4
        _dist._launch(lib, x[rows[0]:rows[1]], x[cols[0]:cols[1]], metric_id, torch.float32, "fp32", buf, ld, norms)
        sa, si = (1, ld) if transposed else (ld, 1)
        _lib.check(lib.ieee_rerank_stream_block(step, _lib.ptr(buf), sa, si, a0, a1, i0, i1, *args, _lib.stream()))

    schedule = stream_schedule(N, slab, Q)
    for s in range(0, len(schedule), len(pieces)):      # one strip: A over all its slabs, then B -- a strip's maxima are
        for step in (0, 1):                             # complete before its keys are formed
            for blk in schedule[s:s + len(pieces)]:
                block(step, *blk)
    del buf
    _lib.check(lib.ieee_rerank_stream_sets(*args, _lib.stream()))
    # C2: the members' distances, each with the matrix's bits, from the gathered-operand GEMM -- no third sweep
    L = stream_layout(Q, G, k1, k2, slab)
    norms = torch.empty(N * 4, dtype=torch.uint8, device=dev)
    _lib.check(lib.ieee_distmat_member_pairs(_lib.ptr(x), N, x.shape[1], Q, _lib.ptr(work[L["V_n"]:]),
                                             _lib.ptr(work[L["V_idx"]:]), L["capV"], metric_id,
                                             _lib.ptr(work[L["V_val"]:]), _lib.ptr(norms), _lib.stream()))
    _lib.check(lib.ieee_rerank_stream_rows(*args, _lib.stream()))
    del norms
    return dict(lib=lib, Q=Q, G=G, slab=slab, x=x, metric_id=metric_id, args=args, work=work)


def _rerank_stream_ranges(st, lambda_value):
    """steps E and F, gallery range by gallery range: yields (g0, g1, fill), fill(out, ldo) writing the range's
    re-ranked distances into out (a tensor whose first element is column g0 of row 0, row stride ldo)"""
    lib, Q, G, x = st["lib"], st["Q"], st["G"], st["x"]
    distances = SlabDistances(lib, x[:Q], st["metric_id"], torch.float32, "fp32", x.device)
    width = min(st["slab"], G)
    for g0 in range(0, G, width):
        g1 = min(g0 + width, G)

        def fill(out, ldo, g0=g0, g1=g1):
            d, ldd, _ = distances.stage(x[Q + g0:Q + g1])
            _lib.check(lib.ieee_rerank_stream_range(_lib.ptr(d), ldd, g0, g1, float(lambda_value), _lib.ptr(out), ldo,
                                                    *st["args"], _lib.stream()))
        yield g0, g1, fill


def re_ranking_features(X_q, X_g, k1=20, k2=6, lambda_value=0.3, metric='euclidean', slab_rows=None, precision=None):
    """k-reciprocal re-ranking from the descriptors X_q [Q, d] and X_g [G, d] (tensors on the host or the device, or
    numpy arrays; converted to fp32): the [Q, G] fp32 matrix, on the device, that re_ranking(cd(X_q, X_g), cd(X_q, X_q),
    cd(X_g, X_g), k1, k2, lambda_value, formulation='sparse') returns for cd = compute_distance_matrix(., ., metric) in
    fp32, bit for bit -- with no [Q, Q], [G, G] or [Q+G, Q+G] tensor.  The distances are produced block by block by the
    distance GEMM, at most slab_rows rows on either side of one GEMM (None: one buffer within SLAB_BUDGET_BYTES), in
    two sweeps over the (Q+G)^2 pairs (column maxima, then the k1+1 nearest of every row), and the distances to the
    members of the k-reciprocal sets by a gathered-operand GEMM (ieee_distmat_member_pairs); the result has the same
    bits for every slab_rows.  Device memory: the
    descriptors, the sparse workspace, one distance buffer and the output.  precision: None or 'fp32' only."""
    st = _rerank_stream(X_q, X_g, k1, k2, metric, slab_rows, precision, "re_ranking_features")
    Q, G = st["Q"], st["G"]
    out = torch.empty((Q, G), dtype=torch.float32, device=st["x"].device)
    for g0, g1, fill in _rerank_stream_ranges(st, lambda_value):
        fill(out[:, g0:], G)
    return out


def rerank_search_topk(X_q, X_g, k, k1=20, k2=6, lambda_value=0.3, metric='euclidean', q_pids=None, g_pids=None,
                       q_camids=None, g_camids=None, slab_rows=None, precision=None):
    """The k nearest kept gallery entries of every query under k-reciprocal re-ranking, without the [Q, G] matrix:
    -> (indices int64 [Q, k], distances fp32 [Q, k]) on the device, what rank_topk(re_ranking_features(X_q, X_g, ...), k,
    ...) lists, bit for bit.  Each gallery range's finished rows go from one reused [Q, slab_rows] buffer through
    ieee_rank_topk_merge into the running lists.  Labels as in search_topk: all four or none."""
    who = "rerank_search_topk"
    k = check_k(k, who)
    given = check_labels_all_or_none(q_pids, g_pids, q_camids, g_camids, who)
    _stream_checks(X_q, X_g, k1, k2, metric, slab_rows, precision, who)
    if given:
        Q, G = int(np.shape(X_q)[0]), int(np.shape(X_g)[0])
        q_pids, q_camids = host_labels(q_pids, "q_pids", Q, who), host_labels(q_camids, "q_camids", Q, who)
        g_pids, g_camids = host_labels(g_pids, "g_pids", G, who), host_labels(g_camids, "g_camids", G, who)
    st = _rerank_stream(X_q, X_g, k1, k2, metric, slab_rows, precision, who)
    Q, G, dev = st["Q"], st["G"], st["x"].device
    acc = TopKAccumulator(Q, k, q_pids if given else None, q_camids if given else None, device=dev)
    if given:
        g_pids, g_camids = on_device(g_pids, dev), on_device(g_camids, dev)
    width = min(st["slab"], G)
    buf = torch.empty((Q, (width + 3) // 4 * 4), dtype=torch.float32, device=dev)
    for g0, g1, fill in _rerank_stream_ranges(st, lambda_value):
        fill(buf, buf.shape[1])
        acc.merge(buf, buf.shape[1], g1 - g0, *((g_pids[g0:g1], g_camids[g0:g1]) if given else ()))
    return acc.result()


# ---- GNN re-ranking (the reference's torchreid/utils/GPU-Re-Ranking/gnn_reranking.py) ----------------------------------
_GNN_PRECISION = {"fp32": 0, "bf16x3": 6, "bf16x2": 3, "f16x2": 2}     # 0, or IEEE_SPLIT_* in include/ieee_amd.h


_GNN_FORMULATIONS = (None, "dense", "sparse", "auto")


def _check_formulation(formulation):
    """before a device is needed"""
    if formulation not in _GNN_FORMULATIONS:
        raise ValueError("gnn re-ranking: formulation must be None, 'dense', 'sparse' or 'auto', got %r" % (formulation,))


def _gnn_inputs(x_q, x_g, precision):
    """-> (lib, precision, q, g, Q, G, d): the checks and the device copies both formulations start with"""
    lib = _lib.require_gpu()
    if precision is None:
        precision = os.environ.get("IEEE_DISTMAT_PRECISION", "fp32")
    if precision not in _GNN_PRECISION:
        raise ValueError("gnn re-ranking: precision must be one of %s, got %r" % (sorted(_GNN_PRECISION), precision))
    q, g = _dev(x_q), _dev(x_g)
    if q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1]:
        raise ValueError("gnn re-ranking: expected X_q [Q, d] and X_g [G, d], got %s and %s" % (tuple(q.shape), tuple(g.shape)))
    d = (q.shape[1] + 7) // 8 * 8    # kernels move 16-byte chunks: zero columns change no inner product (metrics/distance.py)
    return lib, precision, q, g, q.shape[0], g.shape[0], d


def _gnn_dense_bytes(lib, Q, G, d, k1, k2, precision):
    """-> (workspace bytes, bytes needed in all, bytes free): the dense formulation's memory check"""
    nbytes = int(lib.ieee_gnn_rerank_workspace_bytes(Q, G, d, int(k1), int(k2), _GNN_PRECISION[precision]))
    if nbytes < 0:
        _lib.check(-1)
    return nbytes, nbytes + (Q * G + (Q + G) * d) * 4, torch.cuda.mem_get_info()[0]


def _gnn_features(q, g, d):
    """one [Q + G, d] array: the scores are then one GEMM"""
    Q = q.shape[0]
    x = torch.zeros((Q + g.shape[0], d), dtype=torch.float32, device=q.device)
    x[:Q, :q.shape[1]] = q
    x[Q:, :g.shape[1]] = g
    return x


def _gnn(x_q, x_g, k1, k2, precision=None):
    """ieee_gnn_rerank; returns (distmat, workspace) so that tests can read the intermediates (gnn_layout)"""
    lib, precision, q, g, Q, G, d = _gnn_inputs(x_q, x_g, precision)
    nbytes, need, free = _gnn_dense_bytes(lib, Q, G, d, k1, k2, precision)
    if need > free:
        raise RuntimeError("gnn re-ranking is dense: N = Q + G = %d rows need two N x N fp32 work matrices, %d bytes "
                           "with the features and the output, and the device has %d bytes free" % (Q + G, need, free))
    x = _gnn_features(q, g, d)
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



# ---- the sparse formulation (ieee_amd/csrc/gnn_sparse.hip): CSR rows, no (Q+G)^2 and no Q x G allocation --------------
class _Csr(object):
    """rowptr int64 [N+1], col int32, val fp32, norm fp32 [N] or None, on the device; nnz as read back"""
    def __init__(self, rowptr, col, val, norm, nnz):
        self.rowptr, self.col, self.val, self.norm, self.nnz = rowptr, col, val, norm, nnz


def _room(n, dtype, dev):
    return torch.empty(max(int(n), 1), dtype=dtype, device=dev)     # never a null pointer


def _gs_transpose(lib, a, N, r0, r1, scaled, cursor, tptr, trow, tval):
    _lib.check(lib.ieee_gnn_sparse_transpose(_lib.ptr(a.rowptr), _lib.ptr(a.col), _lib.ptr(a.val),
                                             _lib.ptr(a.norm if scaled else None), N, r0, r1, _lib.ptr(cursor),
                                             _lib.ptr(tptr), _lib.ptr(trow), _lib.ptr(tval), trow.numel(), _lib.stream()))


def _gs_symmetrise(lib, a, N, scratch, scaled=False, transposed=True):
    """a / n + (a / n)^T (n = 1 unless scaled); transposed=False: a alone, its rows sorted.  One read-back."""
    dev = a.col.device
    tptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    trow, tval = _room(a.nnz if transposed else 0, torch.int32, dev), _room(a.nnz if transposed else 0, torch.float32, dev)
    if transposed:
        _gs_transpose(lib, a, N, 0, N, scaled, torch.empty(N, dtype=torch.int32, device=dev), tptr, trow, tval)
    rowptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
    sb = scratch.numel()
    _lib.check(lib.ieee_gnn_sparse_symmetrise_count(_lib.ptr(a.rowptr), _lib.ptr(a.col), _lib.ptr(tptr), _lib.ptr(trow), N,
                                                    _lib.ptr(scratch), sb, _lib.ptr(rowptr), _lib.stream()))
    nnz = int(rowptr[N])
    col, val = _room(nnz, torch.int32, dev), _room(nnz, torch.float32, dev)
    norm = torch.empty(N, dtype=torch.float32, device=dev)
    _lib.check(lib.ieee_gnn_sparse_symmetrise_fill(_lib.ptr(a.rowptr), _lib.ptr(a.col), _lib.ptr(a.val),
                                                   _lib.ptr(a.norm if scaled else None), _lib.ptr(tptr), _lib.ptr(trow),
                                                   _lib.ptr(tval), N, _lib.ptr(scratch), sb, _lib.ptr(rowptr),
                                                   _lib.ptr(col), _lib.ptr(val), _lib.ptr(norm), nnz, _lib.stream()))
    return _Csr(rowptr, col, val, norm, nnz)


def _gs_propagate(lib, a, rank, S, N, k1, k2, scratch):
    """sum_{j<k2} S[i][j]^2 a[rank[i][j]] with its row norms.  One read-back."""
    dev = a.col.device
    rowptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
    sb = scratch.numel()
    _lib.check(lib.ieee_gnn_sparse_propagate_count(_lib.ptr(a.rowptr), _lib.ptr(a.col), _lib.ptr(rank), N, k1, k2,
                                                   _lib.ptr(scratch), sb, _lib.ptr(rowptr), _lib.stream()))
    nnz = int(rowptr[N])
    col, val = _room(nnz, torch.int32, dev), _room(nnz, torch.float32, dev)
    norm = torch.empty(N, dtype=torch.float32, device=dev)
    _lib.check(lib.ieee_gnn_sparse_propagate_fill(_lib.ptr(a.rowptr), _lib.ptr(a.col), _lib.ptr(a.val), _lib.ptr(rank),
                                                  _lib.ptr(S), N, k1, k2, _lib.ptr(scratch), sb, _lib.ptr(rowptr),
                                                  _lib.ptr(col), _lib.ptr(val), _lib.ptr(norm), nnz, _lib.stream()))
    return _Csr(rowptr, col, val, norm, nnz)


def _gnn_sparse(x_q, x_g, k1, k2, precision=None, slab_rows=None):
    """steps 1-5 of the sparse formulation -> dict(lib, Q, G, N, slab, rank int32 [N, k1], S fp32 [N, k1] (the negated
    scores, as the dense workspace keeps them), the final rows rowptr / col / val / norm, and entries: the stored
    entries of every stage in order).  Four small read-backs, one per sized stage (one when k2 = 1), and one more in
    _gnn_sparse_ranges."""
    lib, precision, q, g, Q, G, d = _gnn_inputs(x_q, x_g, precision)
    k1, k2 = int(k1), int(k2)
    N = Q + G
    sbytes = int(lib.ieee_gnn_sparse_scratch_bytes(Q, G, k1, k2))
    if sbytes < 0:
        _lib.check(-1)
    slab = check_slab(slab_rows, N, "gnn re-ranking", "slab_rows")
    dev = q.device
    x = _gnn_features(q, g, d)
    # 1: the k1 best of every row of -X X^T (metric id 2), the columns going by in slabs; the first slab is the widest
    acc = TopKAccumulator(N, k1, device=dev)
    scores = SlabDistances(lib, x, 2, torch.float32, precision, dev)
    for lo in range(0, N, slab):
        acc.merge(*scores.stage(x[lo:lo + slab]))
    del scores, x                                   # the slab buffer, its workspace and the features go before steps 2-5
    rank, S = acc.state()
    # 2-5
    scratch = torch.zeros(sbytes, dtype=torch.uint8, device=dev)
    B = _Csr(torch.arange(N + 1, dtype=torch.int64, device=dev) * k1, rank.view(-1),
             torch.ones(N * k1, dtype=torch.float32, device=dev), None, N * k1)
    entries = []
    if k2 == 1:
        R = _gs_symmetrise(lib, B, N, scratch, transposed=False)
        entries.append(R.nnz)
    else:
        R = _gs_symmetrise(lib, B, N, scratch)
        entries.append(R.nnz)
        for last in (False, True):
            R = _gs_propagate(lib, R, rank, S, N, k1, k2, scratch)
            entries.append(R.nnz)
            if not last:
                R = _gs_symmetrise(lib, R, N, scratch, scaled=True)
                entries.append(R.nnz)
    return dict(lib=lib, Q=Q, G=G, N=N, slab=slab, rank=rank, S=S, rowptr=R.rowptr, col=R.col, val=R.val, norm=R.norm,
                entries=entries)


def _gnn_sparse_ranges(st, width):
    """step 6, range by range: yields (g0, g1, fill), fill(out, ldo) writing 1 - cosine of the range into out (a tensor
    whose first element is column g0 of row 0, row stride ldo).  The per-range transposes share one set of buffers."""
    lib, Q, G, N = st["lib"], st["Q"], st["G"], st["N"]
    R = _Csr(st["rowptr"], st["col"], st["val"], None, None)
    dev = R.col.device
    cuts = list(range(0, G, width)) + [G]
    at = st["rowptr"][torch.tensor([Q + c for c in cuts], dtype=torch.int64, device=dev)].cpu()      # one read-back
    cap = int((at[1:] - at[:-1]).max())
    cursor, tptr = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N + 1, dtype=torch.int64, device=dev)
    trow, tval = _room(cap, torch.int32, dev), _room(cap, torch.float32, dev)
    for g0, g1 in zip(cuts[:-1], cuts[1:]):
        def fill(out, ldo, g0=g0, g1=g1):
            _gs_transpose(lib, R, N, Q + g0, Q + g1, False, cursor, tptr, trow, tval)
            _lib.check(lib.ieee_gnn_sparse_cosine(_lib.ptr(R.rowptr), _lib.ptr(R.col), _lib.ptr(R.val), _lib.ptr(st["norm"]),
                                                  _lib.ptr(tptr), _lib.ptr(trow), _lib.ptr(tval), Q, G, g0, g1,
                                                  _lib.ptr(out), ldo, _lib.stream()))
        yield g0, g1, fill


def _gnn_sparse_distmat(x_q, x_g, k1, k2, precision=None, slab_rows=None):
    st = _gnn_sparse(x_q, x_g, k1, k2, precision, slab_rows)
    Q, G = st["Q"], st["G"]
    out = torch.empty((Q, G), dtype=torch.float32, device=st["col"].device)
    for g0, g1, fill in _gnn_sparse_ranges(st, st["slab"]):
        fill(out[:, g0:], G)
    return out


def _gnn_distmat(X_q, X_g, k1, k2, precision, formulation, slab_rows):
    _check_formulation(formulation)
    if formulation == "auto":
        lib, prec, q, g, Q, G, d = _gnn_inputs(X_q, X_g, precision)
        _, need, free = _gnn_dense_bytes(lib, Q, G, d, k1, k2, prec)
        formulation = "dense" if need <= free else "sparse"
        X_q, X_g = q, g
    if formulation == "sparse":
        return _gnn_sparse_distmat(X_q, X_g, k1, k2, precision, slab_rows)
    return _gnn(X_q, X_g, k1, k2, precision)[0]


def gnn_distmat(X_q, X_g, k1=26, k2=7, precision=None, formulation=None, slab_rows=None):
    """GNN re-ranking as a [Q, G] fp32 distance matrix, 1 - similarity, so that evaluate_rank, rank_topk and
    visualize_ranked_results take it like any other: a CUDA tensor when X_q is one, else a numpy array.  The features
    are used as they are (plain inner products, as in the reference): hand in L2-normalised rows, as the reference's
    driver does (main.py) -- on rows that are not normalised the raw inner product is a poor first ranking.  Defaults
    are that driver's Market-1501 values.  Where the reference leaves the result open: ties are broken by the smaller
    index, and a row whose propagated vector is all zero (e.g. an all-zero feature row) has similarity 0 to everything,
    not the reference's NaN.  precision: as in metrics.distance (fp32, or a split scheme for the GEMMs).
    formulation: None or 'dense' -- two (Q+G)^2 fp32 work matrices, RuntimeError when the device has not that much
    free; 'sparse' -- the same algorithm on CSR rows (ieee_gnn_sparse_*), no (Q+G)^2 allocation, the same result within
    rounding (its sums skip the dense form's zero terms and its final product runs in another order); 'auto' -- dense
    when that memory check passes, else sparse.  slab_rows (sparse only): the columns of the score slab [Q+G, slab_rows]
    of the first ranking and the width of the final product's gallery ranges, metrics.search.default_slab_rows(Q+G) by
    default; the result does not depend on it."""
    out = _gnn_distmat(X_q, X_g, k1, k2, precision, formulation, slab_rows)
    if isinstance(X_q, torch.Tensor) and X_q.is_cuda:
        return out
    return out.cpu().numpy()


def gnn_reranking(X_q, X_g, k1, k2, formulation=None):
    """the reference's gnn_reranking(X_q, X_g, k1, k2) (GPU-Re-Ranking/gnn_reranking.py:27-59): L, an integer numpy
    array [Q, G], row i the gallery indices of query i best first (a stable sort of gnn_distmat's rows: equal
    similarities in index order).  CPU or CUDA tensors, or numpy arrays.  See gnn_distmat for what is defined here
    that the reference leaves open (ties; zero rows give similarity 0, not NaN) and for formulation."""
    out = _gnn_distmat(X_q, X_g, k1, k2, None, formulation, None)
    return torch.sort(out, dim=1, stable=True)[1].cpu().numpy()


def gnn_search_topk(X_q, X_g, k, k1=26, k2=7, q_pids=None, g_pids=None, q_camids=None, g_camids=None, precision=None,
                    slab_rows=None):
    """The k nearest kept gallery entries of every query under GNN re-ranking, without the [Q, G] matrix:
    -> (indices int64 [Q, k], distances fp32 [Q, k]) on the device, what rank_topk(gnn_distmat(X_q, X_g, k1, k2,
    formulation='sparse'), k, ...) lists, bit for bit.  The sparse rows are built once; the final product goes gallery
    range by gallery range (slab_rows wide) into one reused [Q, slab_rows] buffer that ieee_rank_topk_merge folds into
    the running lists.  Labels as in search_topk: all four of q_pids, g_pids, q_camids, g_camids (an entry with the
    query's identity and camera is not kept) or none; -1 / +inf where a row has fewer than k kept entries."""
    who = "gnn_search_topk"
    k = check_k(k, who)
    given = check_labels_all_or_none(q_pids, g_pids, q_camids, g_camids, who)
    if given:
        Q, G = int(np.shape(X_q)[0]), int(np.shape(X_g)[0])
        q_pids, q_camids = host_labels(q_pids, "q_pids", Q, who), host_labels(q_camids, "q_camids", Q, who)
        g_pids, g_camids = host_labels(g_pids, "g_pids", G, who), host_labels(g_camids, "g_camids", G, who)
    st = _gnn_sparse(X_q, X_g, k1, k2, precision, slab_rows)
    Q, G, dev = st["Q"], st["G"], st["col"].device
    acc = TopKAccumulator(Q, k, q_pids if given else None, q_camids if given else None, device=dev)
    if given:
        g_pids, g_camids = on_device(g_pids, dev), on_device(g_camids, dev)
    width = min(st["slab"], G)
    buf = torch.empty((Q, (width + 3) // 4 * 4), dtype=torch.float32, device=dev)
    for g0, g1, fill in _gnn_sparse_ranges(st, width):
        fill(buf, buf.shape[1])
        acc.merge(buf, buf.shape[1], g1 - g0, *((g_pids[g0:g1], g_camids[g0:g1]) if given else ()))
    return acc.result()
