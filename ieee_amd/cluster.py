"""DBSCAN on the device (not in the reference): descriptors, or a distance matrix, are grouped into clusters without a
matrix of size N x N being allocated here.

The distances are compute_distance_matrix's, produced block of rows by slab of columns (SlabDistances) and thresholded
where they are written (ieee_cluster_eps_count / _fill); the neighbour graph is closed symmetrically
(ieee_cluster_mirror_*), and the connected components of the core points are found by hook-and-shortcut rounds
(ieee_cluster_cc_round).  The definition the kernels are held to is in DESIGN.md, section 8i; it equals
sklearn.cluster.DBSCAN(eps, min_samples, metric='precomputed') on every symmetric matrix, and its result is unique:
the same labels on every call and for every block / slab."""
import math

import numpy as np
import torch

from . import _lib
from .metrics import distance as _dist
from .metrics._stream import SlabDistances, check_metric, check_precision, check_slab, device_matrix, walk

BLOCK_ROWS = 2048                  # rows thresholded together by default: one [block, slab] distance buffer
INDEX_LIMIT = (1 << 31) - 1        # points are int32 columns
METRICS = ('euclidean', 'cosine', 'precomputed')
EDGE_BYTES = 8                     # per directed neighbour pair: its int32 column, and at most one mirrored int32 column


# ---- the checks: all on the host, none needs the library or a device ---------------------------------------------------
def _check_int(v, name, lo, who):
    try:
        ok = not isinstance(v, bool) and int(v) == v and int(v) >= lo
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("%s: %s must be an integer >= %d, got %r" % (who, name, lo, v))
    return int(v)


def _check_eps(eps, who):
    try:
        e = float(eps)
    except (TypeError, ValueError):
        e = float("nan")
    if isinstance(eps, bool) or not math.isfinite(e) or e < 0:
        raise ValueError("%s: eps must be a finite number >= 0, got %r" % (who, eps))
    return e


def _check_metric(metric, who):
    if metric not in METRICS:
        raise ValueError("%s: metric must be 'euclidean', 'cosine' or 'precomputed', got %r" % (who, metric))
    return metric


def _check_points(N, who):
    if N >= INDEX_LIMIT:
        raise ValueError("%s: %d points are beyond the index range (%d)" % (who, N, INDEX_LIMIT))
    return N


def _check_input(X, metric, who):
    """-> N"""
    if metric == 'precomputed':
        shape = tuple(X.shape) if isinstance(X, (torch.Tensor, np.ndarray)) else None
        if shape is None or len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError("%s: metric='precomputed' takes an [N, N] distance matrix (tensor or numpy array), got %s"
                             % (who, shape if shape is not None else type(X).__name__))
        return _check_points(shape[0], who)
    if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.shape[1] < 1:
        raise ValueError("%s: X must be an [N, d] tensor with d >= 1, got %s"
                         % (who, tuple(X.shape) if isinstance(X, torch.Tensor) else type(X).__name__))
    return _check_points(X.shape[0], who)


def _blocking(N, block, slab, who):
    """-> (block, slab) in rows, expand_descriptors' conventions: `block` rows are thresholded together against slabs of
    `slab` columns; by default one [block, slab] fp32 buffer stays within SLAB_BUDGET_BYTES"""
    block = min(check_slab(BLOCK_ROWS if block is None else block, 0, who, "block"), max(N, 1))
    return block, check_slab(slab, block, who)


def _r512(nbytes):
    return (int(nbytes) + 511) // 512 * 512    # the caching allocator hands out multiples of 512 bytes


def dbscan_layout(N, d, edges, block=None, slab=None, metric='euclidean'):
    """The device memory dbscan(...) allocates for N fp32 points of d columns whose neighbour graph has `edges` directed
    pairs (info['edges'] of a run; N times the mean degree), in bytes, by purpose, and their sum as 'total' (each rounded
    up to the allocator's 512 bytes).  Only 'lists' and 'mirror' depend on eps: 4 bytes per pair, and at most 4 more for
    a pair that has to be mirrored (none where the distances are bitwise symmetric) -- EDGE_BYTES = 8 per pair, and
    max_edges defaults to the free device memory // (2 * EDGE_BYTES), which leaves half of it free.  'rows' is the copy
    of X (on the device, compute dtype, d rounded up to 8; not made where X is in that form already).  'precomputed': d
    is ignored, the matrix is read in place and 'matrix' is what a matrix arriving from the host takes.  The total holds
    for precision 'fp32' only ('gemm_work' is the fp32 GEMM's workspace, the two norm vectors): the split precisions
    and 'bf16' add the GEMM's own pieces or bf16 copies of one block and one slab, which are not counted here."""
    who = "dbscan_layout"
    _check_metric(metric, who)
    N, edges = _check_int(N, "N", 0, who), _check_int(edges, "edges", 0, who)
    _check_points(N, who)
    block, slab = _blocking(N, block, slab, who)
    slab = min(slab, max(N, 1))
    out = {
        "rowptr": 2 * _r512(8 * (N + 1)),                    # of the lists and of the mirrored lists
        "cursor": _r512(4 * N),
        "scan_work": _r512(8 * (N + 1)),                     # the exclusive sums' own scratch
        "lists": _r512(4 * edges), "mirror": _r512(4 * edges),
        "core": _r512(N), "parents": 2 * _r512(4 * N) + 512,  # two rounds' arrays and the flag
        "numbers": _r512(8 * (N + 1)), "labels": _r512(8 * N),
    }
    if metric == 'precomputed':
        out["matrix"] = _r512(4 * N * N)
    else:
        d = _check_int(d, "d", 1, who)
        d8 = (d + 7) // 8 * 8
        out["rows"] = _r512(4 * N * d8)
        out["distances"] = _r512(4 * block * ((slab + 3) // 4 * 4))
        out["gemm_work"] = _r512(4 * (block + slab))
    out["total"] = sum(out.values())
    return out


# ---- the sweeps: every [rows, cols] distance buffer of the problem, rows ascending, columns ascending within a row ------
def _sweep_descriptors(lib, Xp, metric_id, cdt, precision, block, slab, visit):
    N, d8 = Xp.shape
    stage = SlabDistances(lib, Xp[:block], metric_id, cdt, precision, Xp.device)
    for lo in range(0, N, block):
        stage.set_query(Xp[lo:lo + block])                   # one buffer and one workspace for all blocks
        for base, cand in walk((Xp,), slab, d8, "dbscan"):
            buf, ldd, n = stage.stage(cand)
            visit(buf, ldd, min(block, N - lo), n, lo, base)
            del buf


def _sweep_matrix(D, ldd, block, visit):
    N = D.shape[0]
    for lo in range(0, N, block):
        visit(D[lo:lo + block], ldd, min(block, N - lo), N, lo, 0)


def _exclusive_sum_in_place(ptr):
    """ptr [N + 1] int64 with ptr[0] = 0 and the counts in ptr[1:] -> the row pointers; returns the total (one read)"""
    ptr[1:].cumsum_(0)
    return int(ptr[-1].item())


def dbscan(X, eps, min_samples=4, metric='euclidean', block=None, slab=None, precision=None, max_edges=None,
           return_info=False):
    """DBSCAN.  -> labels, int64 [N] on the device: clusters 0, 1, ... numbered by ascending smallest core index, -1 for
    noise; with return_info=True also a dict: 'core' (bool [N] on the device), 'clusters', 'edges' (directed neighbour
    pairs found by the threshold), 'mirrored_edges' (pairs added by the symmetric closure) and 'rounds' (launches of the
    component search), python ints.

    metric 'euclidean' | 'cosine': X is an [N, d] tensor, on the device or on the host, and the distances are
    compute_distance_matrix(X, X, metric, precision)'s -- SQUARED Euclidean for 'euclidean', as everywhere in this
    project: scikit-learn's eps corresponds to eps ** 2 here.  They are produced `block` rows by `slab` columns at a time
    (expand_descriptors' conventions) and never kept; neither changes the result.  metric 'precomputed': X is an [N, N]
    distance matrix, tensor or numpy array (a Jaccard matrix from re_ranking, say), read `block` rows at a time.

    j is a neighbour of i iff i == j or D[i, j] <= float32(eps) or D[j, i] <= float32(eps) (a NaN is never a neighbour);
    i is core iff it has at least min_samples neighbours, itself included; clusters are the connected components of the
    core points; a non-core point with a core neighbour takes the smallest cluster number among its core neighbours.
    The memory grows with the number of neighbour pairs: above max_edges (default: what half of the free device memory
    holds, see dbscan_layout) a ValueError says so before anything is filled."""
    who = "dbscan"
    eps = _check_eps(eps, who)
    min_samples = _check_int(min_samples, "min_samples", 1, who)
    _check_metric(metric, who)
    check_precision(precision)
    N = _check_input(X, metric, who)
    block, slab = _blocking(N, block, slab, who)
    if max_edges is not None:
        max_edges = _check_int(max_edges, "max_edges", 0, who)
    lib = _lib.require_gpu()
    device = X.device if isinstance(X, torch.Tensor) and X.is_cuda else torch.device("cuda")
    if N == 0:
        labels = torch.empty(0, dtype=torch.int64, device=device)
        info = dict(core=torch.empty(0, dtype=torch.bool, device=device), clusters=0, edges=0, mirrored_edges=0, rounds=0)
        return (labels, info) if return_info else labels
    st = _lib.stream
    if metric == 'precomputed':
        D, ldd = device_matrix(X, device)

        def sweep(visit):
            _sweep_matrix(D, ldd, block, visit)
    else:
        metric_id = check_metric(metric)
        precision, cdt = _dist._resolve(precision, X.dtype)
        Xp = _dist._pad8(X.detach().to(device).to(cdt).contiguous())

        def sweep(visit):
            _sweep_descriptors(lib, Xp, metric_id, cdt, precision, block, slab, visit)

    # A: count, exclusive sum, fill
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=device)
    sweep(lambda buf, ld, rows, cols, row0, col0: _lib.check(lib.ieee_cluster_eps_count(
        _lib.ptr(buf), ld, rows, cols, row0, col0, N, eps, _lib.ptr(rowptr[1:]), st())))
    edges = _exclusive_sum_in_place(rowptr)
    if max_edges is None:
        max_edges = torch.cuda.mem_get_info(device)[0] // (2 * EDGE_BYTES)
    if edges > max_edges:
        raise ValueError("%s: eps = %g gives %d neighbour pairs over %d points, a mean degree of %.1f, above max_edges = %d: "
                         "eps is too large for this memory (dbscan_layout shows the arithmetic)"
                         % (who, eps, edges, N, edges / float(N), max_edges))
    col = torch.empty(edges, dtype=torch.int32, device=device)
    cursor = torch.zeros(N, dtype=torch.int32, device=device)
    sweep(lambda buf, ld, rows, cols, row0, col0: _lib.check(lib.ieee_cluster_eps_fill(
        _lib.ptr(buf), ld, rows, cols, row0, col0, N, eps, _lib.ptr(rowptr), _lib.ptr(cursor), _lib.ptr(col), edges, st())))
    # X: the OR closure
    xptr = torch.zeros(N + 1, dtype=torch.int64, device=device)
    _lib.check(lib.ieee_cluster_mirror_count(_lib.ptr(rowptr), _lib.ptr(col), N, _lib.ptr(xptr[1:]), st()))
    mirrored = _exclusive_sum_in_place(xptr)
    xcol = torch.empty(mirrored, dtype=torch.int32, device=device)
    if mirrored:
        cursor.zero_()
        _lib.check(lib.ieee_cluster_mirror_fill(_lib.ptr(rowptr), _lib.ptr(col), N, _lib.ptr(xptr), _lib.ptr(cursor),
                                                _lib.ptr(xcol), mirrored, st()))
    del cursor
    # core points, then the components
    core = torch.empty(N, dtype=torch.uint8, device=device)
    f, fnext = (torch.empty(N, dtype=torch.int32, device=device) for _ in range(2))
    changed = torch.empty(1, dtype=torch.int32, device=device)
    _lib.check(lib.ieee_cluster_core(_lib.ptr(rowptr), _lib.ptr(xptr), N, min_samples, _lib.ptr(core), _lib.ptr(f), st()))
    for rounds in range(1, N + 1):
        _lib.check(lib.ieee_cluster_cc_round(_lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(xptr), _lib.ptr(xcol), _lib.ptr(core),
                                             N, _lib.ptr(f), _lib.ptr(fnext), _lib.ptr(changed), st()))
        f, fnext = fnext, f
        if not int(changed.item()):
            break
    else:
        raise _lib.IeeeAmdError("%s: the components did not settle in %d rounds" % (who, N))
    del fnext
    # labels
    number = torch.zeros(N + 1, dtype=torch.int64, device=device)
    _lib.check(lib.ieee_cluster_roots(_lib.ptr(core), _lib.ptr(f), N, _lib.ptr(number[1:]), st()))
    clusters = _exclusive_sum_in_place(number)
    labels = torch.empty(N, dtype=torch.int64, device=device)
    _lib.check(lib.ieee_cluster_labels(_lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(xptr), _lib.ptr(xcol), _lib.ptr(core),
                                       _lib.ptr(f), _lib.ptr(number), N, _lib.ptr(labels), st()))
    if not return_info:
        return labels
    return labels, dict(core=core.view(torch.bool), clusters=clusters, edges=edges, mirrored_edges=mirrored, rounds=rounds)
