"""Query expansion and database-side augmentation on the device (not in the reference): a descriptor is replaced by the
weighted sum of its k nearest neighbours' L2-normalised rows, itself normalised.

    alpha = 0            average query expansion, AQE (Chum et al. 2007)
    alpha > 0            weights similarity^alpha, alpha-QE (Radenovic et al. 2018)
    mode = 'both'        query and gallery rows alike, each over all Q + G rows, itself included: database-side
                         augmentation (Arandjelovic & Zisserman 2012) together with the query side
    mode = 'query'       the queries alone, over the gallery rows, the query itself with weight 1

The neighbour lists are search_topk's (metric 'cosine'): the slab-distance GEMM and ieee_rank_topk_merge, block of
rows by block of rows, so nothing of size N x N is ever allocated.  The weights (ieee_expand_weights) and the gather-
and-sum (ieee_neighbour_sum) are this module's kernels.  The result replaces the descriptors, so every path that takes
descriptors takes it: compute_distance_matrix, search_topk, evaluate_rank_streamed, the re-ranking drivers.  Labels are
never used.  The definition, row by row, is in DESIGN.md ("Query expansion")."""
import torch

from . import _lib
from .metrics import distance as _dist
from .metrics._stream import (SlabDistances, as_pieces, check_k, check_piece, check_precision, check_query, check_slab,
                              count_rows, walk)
from .metrics.search import TOPK_MERGE_INDEX_LIMIT, TopKAccumulator

ALPHA_MAX = 64                     # ieee_amd/csrc/expand.hip: the longest weight chain
BLOCK_ROWS = 2048                  # rows whose lists are formed together by default: one [block, slab] distance buffer
MODES = ('both', 'query')


# ---- the checks: all on the host, none needs the library or a device ---------------------------------------------------
def _check_int(v, name, lo, hi, who):
    try:
        ok = not isinstance(v, bool) and int(v) == v and lo <= int(v) and (hi is None or int(v) <= hi)
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("%s: %s must be an integer %s, got %r"
                         % (who, name, "in [%d, %d]" % (lo, hi) if hi is not None else ">= %d" % lo, v))
    return int(v)


def _check_mode(mode, who):
    if mode not in MODES:
        raise ValueError("%s: mode must be 'both' or 'query', got %r" % (who, mode))
    return mode


def check_expansion_args(k, alpha, times, mode, who):
    """-> (k, alpha, times, mode), checked: what expand_descriptors and the engine's query_expansion share"""
    return (check_k(k, who), _check_int(alpha, "alpha", 0, ALPHA_MAX, who), _check_int(times, "times", 1, None, who),
            _check_mode(mode, who))


def _pad8_cols(d):
    return (d + 7) // 8 * 8


def _blocking(n_rows, slab, block, who):
    """-> (block, slab) in rows: `block` rows form their lists together, the candidates go by `slab` rows at a time;
    by default one [block, slab] fp32 buffer stays within SLAB_BUDGET_BYTES"""
    block = min(check_slab(BLOCK_ROWS if block is None else block, 0, who, "block"), max(n_rows, 1))
    return block, check_slab(slab, block, who)


def _r512(nbytes):
    return (int(nbytes) + 511) // 512 * 512    # the caching allocator hands out multiples of 512 bytes


def expansion_layout(Q, G, d, k, slab=None, block=None, mode='both'):
    """The device memory expand_descriptors(...) allocates for fp32 inputs at the default precision, in bytes, by
    purpose, and their sum as 'total' (each rounded up to the allocator's 512 bytes).  'both': the rows and the output
    are [Q + G, d8] buffers, d8 = d rounded up to 8.  'query': the rows of a host gallery never arrive wholesale --
    'table' holds the at most min(Q k, G) distinct neighbour rows and 'staged' one slab of a host piece (twice that when
    d is no multiple of 8).  'neighbours' is allocated with return_neighbours=True only.  Other precisions add the
    GEMM's own split or bf16 copies of one block and one slab."""
    who = "expansion_layout"
    k = check_k(k, who)
    _check_mode(mode, who)
    Q, G, d = (_check_int(v, n, lo, None, who) for v, n, lo in ((Q, "Q", 0), (G, "G", 0), (d, "d", 1)))
    d8 = _pad8_cols(d)
    n_rows, n_cand = (Q + G, Q + G) if mode == 'both' else (Q, G)
    block, slab = _blocking(n_rows, slab, block, who)
    slab = min(slab, max(n_cand, 1))
    out = {
        "rows": _r512(4 * n_rows * d8), "out": _r512(4 * n_rows * d8), "rinv": _r512(4 * n_rows),
        "distances": _r512(4 * block * ((slab + 3) // 4 * 4)), "gemm_work": _r512(4 * (block + slab)),
        # a block's lists and weights live until the next block's are formed: two blocks' worth
        "lists": 4 * _r512(4 * block * k), "weights": 2 * _r512(4 * block * k),
        "neighbours": _r512(8 * n_rows * k) + _r512(4 * n_rows * k),
    }
    if mode == 'query':
        table = min(Q * k, G)
        out["lists"] = 2 * _r512(4 * Q * k) + 2 * _r512(4 * block * k)
        out["weights"] = _r512(4 * Q * k)
        out["table"] = _r512(4 * table * d8) + _r512(4 * table) + 4 * _r512(8 * Q * k)
        out["staged"] = _r512(4 * slab * d8) * (1 if d == d8 else 2)
    out["total"] = sum(out.values())
    return out


# ---- the kernels' shims ------------------------------------------------------------------------------------------------
def _row_stride(t, cols, name, who):
    """a 2-D fp32 device tensor the kernels can read in place: unit column stride, rows that do not overlap"""
    if t.stride(1) != 1 and t.shape[1] > 1 or (t.shape[0] > 1 and t.stride(0) < cols):
        raise ValueError("%s: %s must have unit column stride and a row stride of at least %d" % (who, name, cols))
    return max(t.stride(0), cols)


def row_rinv(x):
    """1 / max(|row|, 1e-12) of the rows of x [n, d] (fp32, on the device), with the bits the cosine distance's norm pass
    gives (ieee_row_rinv: the same kernel); zero columns are appended where d is no multiple of 8, which changes nothing"""
    lib = _lib.require_gpu()
    x = _dist._pad8(x.contiguous())
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    _lib.check(lib.ieee_row_rinv(_lib.ptr(x), x.shape[0], x.shape[1], _lib.ptr(out), _lib.stream()))
    return out


def expand_weights(idx, dist, alpha):
    """(idx int32, dist fp32) [n, k] on the device, as TopKAccumulator.state() holds them -> w fp32 [n, k]:
    max(1 - dist, 0)^alpha by alpha - 1 fp32 multiplications, 1 for alpha = 0, 0 at a padded place (idx < 0)"""
    alpha = _check_int(alpha, "alpha", 0, ALPHA_MAX, "expand_weights")
    lib = _lib.require_gpu()
    idx, dist = idx.to(torch.int32).contiguous(), dist.to(torch.float32).contiguous()
    w = torch.empty_like(dist)
    _lib.check(lib.ieee_expand_weights(_lib.ptr(idx), _lib.ptr(dist), idx.numel(), alpha, _lib.ptr(w), _lib.stream()))
    return w


def _check_neighbour_sum(src, idx, weights, rinv, self_rows, self_rinv, who):
    for t, name in ((src, "src"), (idx, "idx"), (weights, "weights")):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError("%s: %s must be a 2-D tensor" % (who, name))
    (n_src, d), (n, k) = src.shape, idx.shape
    if d < 1:
        raise ValueError("%s: src must have at least one column" % who)
    check_k(k, who)
    if idx.dtype.is_floating_point or idx.dtype == torch.bool:
        raise ValueError("%s: idx must be an integer tensor, got %s" % (who, idx.dtype))
    if tuple(weights.shape) != (n, k):
        raise ValueError("%s: weights %s do not match idx %s" % (who, tuple(weights.shape), (n, k)))
    if rinv is not None and (not isinstance(rinv, torch.Tensor) or tuple(rinv.shape) != (n_src,)):
        raise ValueError("%s: rinv must be a [%d] tensor" % (who, n_src))
    if self_rinv is not None and self_rows is None:
        raise ValueError("%s: self_rinv without self_rows" % who)
    if self_rows is not None and (not isinstance(self_rows, torch.Tensor) or tuple(self_rows.shape) != (n, d)):
        raise ValueError("%s: self_rows must be a [%d, %d] tensor" % (who, n, d))
    if self_rinv is not None and (not isinstance(self_rinv, torch.Tensor) or tuple(self_rinv.shape) != (n,)):
        raise ValueError("%s: self_rinv must be a [%d] tensor" % (who, n))
    return n_src, d, n, k


def _in_place_fp32(t):
    """fp32 with unit column stride and rows that do not overlap: as it is when it is that already (a row-strided
    view is read in place), else a contiguous copy"""
    t = t.to(torch.float32)
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def neighbour_sum(src, idx, weights, rinv=None, self_rows=None, self_rinv=None, normalize=True, out=None):
    """out[i] = [self_rinv[i] * self_rows[i] +] sum_j (weights[i, j] * rinv[idx[i, j]]) * src[idx[i, j]], normalised to
    unit length with normalize (a zero sum stays zero): ieee_neighbour_sum.  src [n_src, d], idx / weights [n, k] with
    k <= 1024, on the device; an index outside [0, n_src) -- -1 pads a list -- adds nothing.  Without rinv the
    coefficient is the weight alone; without self_rinv the self row enters unscaled.  Row-strided views are read in
    place.  -> fp32 [n, d] on the device (out, when given: fp32, unit column stride, disjoint from src and self_rows)."""
    who = "neighbour_sum"
    n_src, d, n, k = _check_neighbour_sum(src, idx, weights, rinv, self_rows, self_rinv, who)
    lib = _lib.require_gpu()
    src = _in_place_fp32(src)
    if idx.dtype != torch.int32:       # an int64 index beyond int32 is outside [0, n_src) either way
        idx = idx.clamp(-1, (1 << 31) - 1).to(torch.int32)
    if idx.stride(1) != 1 and k > 1 or n > 1 and idx.stride(0) < k or tuple(weights.stride()) != tuple(idx.stride()) \
            or weights.dtype != torch.float32:
        idx, weights = idx.contiguous(), weights.to(torch.float32).contiguous()
    if self_rows is not None:
        self_rows = _in_place_fp32(self_rows)
    rinv = None if rinv is None else rinv.to(torch.float32).contiguous()
    self_rinv = None if self_rinv is None else self_rinv.to(torch.float32).contiguous()
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=src.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n, d):
        raise ValueError("%s: out must be a float32 [%d, %d] tensor" % (who, n, d))
    _lib.check(lib.ieee_neighbour_sum(
        _lib.ptr(src), _row_stride(src, d, "src", who), n_src, _lib.ptr(rinv), _lib.ptr(idx), _lib.ptr(weights),
        max(idx.stride(0), k), n, k, _lib.ptr(self_rows),
        _lib.ptr(self_rinv), _row_stride(self_rows, d, "self_rows", who) if self_rows is not None else 0, d,
        1 if normalize else 0, _lib.ptr(out), _row_stride(out, d, "out", who), _lib.stream()))
    return out


# ---- the driver ----------------------------------------------------------------------------------------------------
def _device_of(query):
    """where the work happens: the query's GPU, else the current one"""
    return query.device if query.is_cuda else torch.device("cuda")


def _lists(lib, rows, pieces, k, slab, dim, cdt, precision, who):
    """the k nearest candidates (cosine) of every row of rows [n, d8]: TopKAccumulator's live (idx int32, dist fp32)"""
    acc = TopKAccumulator(rows.shape[0], k, device=rows.device)
    distances = SlabDistances(lib, rows, 1, cdt, precision, rows.device)
    for _, cand in walk(pieces, slab, dim, who):
        acc.merge(*distances.stage(cand))
    return acc.state()


def _round_both(lib, X, Y, k, alpha, slab, block, cdt, precision, keep, who):
    """one round over X [N, d8] into Y; keep: None or the (idx int64, dist fp32) [N, k] tensors the lists are copied into"""
    N, d8 = X.shape
    rinv = row_rinv(X)
    for lo in range(0, N, block):
        idx, dist = _lists(lib, X[lo:lo + block], (X,), k, slab, d8, cdt, precision, who)
        if keep is not None:
            keep[0][lo:lo + block].copy_(idx)
            keep[1][lo:lo + block].copy_(dist)
        neighbour_sum(X, idx, expand_weights(idx, dist, alpha), rinv=rinv, out=Y[lo:lo + block])


def _neighbour_table(idx, pieces, d8, device):
    """The distinct gallery rows the lists name, as a compact fp32 [U, d8] table on the device, and the lists remapped
    to it.  Rows are picked piece by piece where the piece is, by sorted unique indices, and copied once."""
    valid = idx >= 0
    uniq, inverse = torch.unique(idx[valid], sorted=True, return_inverse=True)
    remapped = torch.full_like(idx, -1)
    remapped[valid] = inverse.to(torch.int32)
    table = torch.zeros((uniq.numel(), d8), dtype=torch.float32, device=device)
    uniq_host = uniq.cpu().long()
    base = 0
    for piece in pieces:
        lo, hi = (int(v) for v in torch.searchsorted(uniq_host, torch.tensor([base, base + piece.shape[0]])))
        if hi > lo:
            local = uniq_host[lo:hi] - base
            table[lo:hi, :piece.shape[1]].copy_(piece.detach().index_select(0, local.to(piece.device)))
        base += piece.shape[0]
    return table, remapped


def _round_query(lib, Xq, Y, pieces, k, alpha, slab, block, dim, cdt, precision, keep, who):
    """one round of the queries Xq [Q, d8] against the gallery's pieces into Y"""
    Q, d8 = Xq.shape
    idx = torch.empty((Q, k), dtype=torch.int32, device=Xq.device)
    dist = torch.empty((Q, k), dtype=torch.float32, device=Xq.device)
    for lo in range(0, Q, block):
        i, s = _lists(lib, Xq[lo:lo + block], pieces, k, slab, dim, cdt, precision, who)
        idx[lo:lo + block].copy_(i)
        dist[lo:lo + block].copy_(s)
    if keep is not None:
        keep[0].copy_(idx)
        keep[1].copy_(dist)
    table, remapped = _neighbour_table(idx, pieces, d8, Xq.device)
    neighbour_sum(table, remapped, expand_weights(idx, dist, alpha), rinv=row_rinv(table), self_rows=Xq,
                  self_rinv=row_rinv(Xq), out=Y)


def expand_descriptors(query, gallery, k=5, alpha=3, times=1, mode='both', slab=None, block=None, precision=None,
                       return_neighbours=False):
    """Query expansion (mode 'query') or query expansion with database-side augmentation (mode 'both'), `times` rounds.
    -> (query', gallery') fp32 on the device, unit rows; with return_neighbours also (idx int64, dist fp32) [rows, k],
    the last round's lists as search_topk returns them (over the Q + G rows in 'both', over the Q queries in 'query').

    One round: every row's k nearest candidates by cosine distance (search_topk's lists: ascending (distance, index),
    -1 / +inf where k exceeds the candidates); w = max(1 - dist, 0)^alpha (1 for alpha = 0, 0 at a padded place);
    y = sum_j (w_j / max(|x_j|, 1e-12)) x_j over the list in order; the row becomes y / max(|y|, 1e-12).  'both': the
    candidates of a row are all Q + G rows, itself included, and every row of a round reads the round's input.  'query':
    the candidates are the gallery rows, the query itself enters first with weight 1, and the gallery is returned as
    the object that was passed in; every round runs against it.  The returned queries have unit length and that gallery
    is as it was: rank them with metric='cosine' unless the gallery is normalised too.

    query: [Q, d] tensor.  gallery: 'both': a [G, d] tensor; 'query': a [G, d] tensor or a list / tuple / other
    re-iterable of [g_i, d] tensors, on the host or on the device (not a one-shot generator: the gallery is walked once
    for the lists and once for the rows they name).  Rows are handled `block` at a time against slabs of `slab`
    candidates; neither changes a bit of the result.  precision is compute_distance_matrix's, for the lists' distances.
    expansion_layout(...) says what is allocated; nothing grows like (Q + G)^2 or Q x G."""
    who = "expand_descriptors"
    k, alpha, times, mode = check_expansion_args(k, alpha, times, mode, who)
    check_precision(precision)
    Q, dim = check_query(query, who)
    if dim < 1:
        raise ValueError("%s: the descriptors need at least one column" % who)
    if mode == 'both':
        check_piece(gallery, dim, who)
        pieces, G = (gallery,), int(gallery.shape[0])
        n_rows = n_cand = Q + G
    else:
        pieces = as_pieces(gallery, who)
        if iter(pieces) is pieces:
            raise ValueError("%s: mode='query' walks the gallery twice (the lists, then the rows they name): a one-shot "
                             "iterator cannot be walked again; pass a tensor or a list of pieces" % who)
        if not isinstance(pieces, (list, tuple)):
            pieces = tuple(pieces)
        G = count_rows(pieces, dim, who)
        n_rows, n_cand = Q, G
    if n_cand >= TOPK_MERGE_INDEX_LIMIT:
        raise ValueError("%s: %d candidate rows are beyond the index range (%d)" % (who, n_cand, TOPK_MERGE_INDEX_LIMIT))
    block, slab = _blocking(n_rows, slab, block, who)
    lib = _lib.require_gpu()
    device = _device_of(query)
    precision, cdt = _dist._resolve(precision, torch.float32)
    d8 = _pad8_cols(dim)
    X = torch.empty((n_rows, d8), dtype=torch.float32, device=device) if d8 == dim else \
        torch.zeros((n_rows, d8), dtype=torch.float32, device=device)
    X[:Q, :dim].copy_(query.detach())
    if mode == 'both':
        X[Q:, :dim].copy_(gallery.detach())
    Y = torch.empty_like(X)
    keep = None
    if return_neighbours:
        keep = (torch.empty((n_rows, k), dtype=torch.int64, device=device),
                torch.empty((n_rows, k), dtype=torch.float32, device=device))
    for _ in range(times):
        if n_rows:
            if mode == 'both':
                _round_both(lib, X, Y, k, alpha, slab, block, cdt, precision, keep, who)
            else:
                _round_query(lib, X, Y, pieces, k, alpha, slab, block, dim, cdt, precision, keep, who)
        X, Y = Y, X
    result = (X[:Q, :dim], X[Q:, :dim] if mode == 'both' else gallery)
    return result + (keep,) if return_neighbours else result
