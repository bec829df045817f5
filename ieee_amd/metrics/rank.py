"""CMC / mAP on MI355X.  Mirrors torchreid/metrics/rank.py:246-287 (evaluate_rank ->
evaluate_py -> eval_market1501 :103-171); the per-query ranking runs in
ieee_rank_market1501 (no sort: the true matches are sorted in LDS and each one's
rank is a prefix sum of a histogram filled while the distance row streams past).
eval_cuhk03 (:24-100, the single-gallery-shot protocol with the time-id filter) runs
in ieee_rank_cuhk03 as the closed form of what the reference samples; eval_regdb
(:175-230) is the Market kernel with constant cameras."""
import numpy as np
import torch

from .. import _lib
from ._stream import device_matrix, host_labels, on_device


def _i32(x, name, device):
    """labels as a flat int32 array on the device, their range checked"""
    return on_device(host_labels(x, name, None, None), device)


def rank_counts(distmat, q_pids, g_pids, q_camids, g_camids, max_rank):
    """the device part of eval_market1501: returns (cmc_counts int64[max_rank], num_valid_q, AP sum) of the given
    queries -- additive over disjoint query sets, which is what a query-sharded evaluation all-reduces"""
    lib = _lib.require_gpu()
    d, ldd = device_matrix(distmat)
    num_q, num_g = d.shape
    dev = d.device
    qp, gp = _i32(q_pids, "q_pids", dev), _i32(g_pids, "g_pids", dev)
    qc, gc = _i32(q_camids, "q_camids", dev), _i32(g_camids, "g_camids", dev)
    assert qp.numel() == num_q and qc.numel() == num_q and gp.numel() == num_g and gc.numel() == num_g
    if num_q == 0:
        return np.zeros(max_rank, dtype=np.int64), 0.0, 0.0
    ap = torch.empty(num_q, dtype=torch.float64, device=dev)
    first = torch.empty(num_q, dtype=torch.int32, device=dev)
    summary = torch.empty(max_rank + 2, dtype=torch.int64, device=dev)
    work = torch.empty(lib.ieee_rank_workspace_bytes(num_g), dtype=torch.uint8, device=dev)
    _lib.check(lib.ieee_rank_market1501_ws(_lib.ptr(d), ldd, num_q, num_g, _lib.ptr(qp), _lib.ptr(gp),
                                           _lib.ptr(qc), _lib.ptr(gc), max_rank, _lib.ptr(ap), _lib.ptr(first),
                                           _lib.ptr(summary), _lib.ptr(work), work.numel(), _lib.stream()))
    s = summary.cpu().numpy()          # the evaluator's single read-back (22 words)
    return s[:max_rank].copy(), float(s[max_rank]), float(s[max_rank + 1:max_rank + 2].view(np.float64)[0])


def finish_counts(cmc_counts, num_valid_q, ap_sum):
    """rank.py:166-169: CMC curve and mAP from the summed per-query results"""
    assert num_valid_q > 0, 'Error: all query identities do not appear in gallery'
    all_cmc = np.asarray(cmc_counts).astype(np.float32) / np.float32(num_valid_q)
    return all_cmc, float(ap_sum / num_valid_q)


def eval_market1501(distmat, q_pids, g_pids, q_camids, g_camids, max_rank):
    """rank.py:103-171.  distmat: numpy array (as the reference's caller passes, engine.py:400) or a
    CUDA tensor (on-device hand-off)."""
    num_g = distmat.shape[1]
    if num_g < max_rank:
        max_rank = num_g
        print('Note: number of gallery samples is quite small, got {}'.format(num_g))
    return finish_counts(*rank_counts(distmat, q_pids, g_pids, q_camids, g_camids, max_rank))


def fold_keys(q_camids, g_camids, q_timeids=None, g_timeids=None):
    """(camera, time id) pairs as dense int32 keys, numbered jointly over query and gallery so that equal pairs get
    equal keys on both sides.  None for both time-id arrays means "all equal": upstream Torchreid's cuhk03 protocol,
    which filters on identity and camera only."""
    if (q_timeids is None) != (g_timeids is None):
        raise ValueError("q_timeids and g_timeids are given together or not at all")
    as_np = lambda x: np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x).reshape(-1)
    qc, gc = as_np(q_camids), as_np(g_camids)
    qt = np.zeros(len(qc), dtype=np.int64) if q_timeids is None else as_np(q_timeids)
    gt = np.zeros(len(gc), dtype=np.int64) if g_timeids is None else as_np(g_timeids)
    assert len(qt) == len(qc) and len(gt) == len(gc)
    pairs = np.stack([np.concatenate([qc, gc]), np.concatenate([qt, gt])], 1)
    _, keys = np.unique(pairs, axis=0, return_inverse=True)
    keys = keys.reshape(-1).astype(np.int32)
    return keys[:len(qc)], keys[len(qc):]


def cuhk03_sums(distmat, q_pids, g_pids, q_camids, g_camids, q_timeids, g_timeids, max_rank):
    """the device part of eval_cuhk03 (ieee_rank_cuhk03): returns (cmc_sums float64[max_rank], num_valid_q, AP sum,
    cmc, ap) -- the first three additive over disjoint query sets like rank_counts', then the per-query expected
    curves float64[num_q][max_rank] (zeros for a skipped query) and APs float64[num_q] (-1 when skipped) as device
    tensors, for tests and tools."""
    lib = _lib.require_gpu()
    d, ldd = device_matrix(distmat)
    num_q, num_g = d.shape
    dev = d.device
    qk, gk = fold_keys(q_camids, g_camids, q_timeids, g_timeids)
    qp, gp = _i32(q_pids, "q_pids", dev), _i32(g_pids, "g_pids", dev)
    qk, gk = _i32(qk, "q_keys", dev), _i32(gk, "g_keys", dev)
    assert qp.numel() == num_q and qk.numel() == num_q and gp.numel() == num_g and gk.numel() == num_g
    cmc = torch.empty(num_q, max_rank, dtype=torch.float64, device=dev)
    ap = torch.empty(num_q, dtype=torch.float64, device=dev)
    if num_q == 0:
        return np.zeros(max_rank, dtype=np.float64), 0.0, 0.0, cmc, ap
    summary = torch.empty(max_rank + 2, dtype=torch.float64, device=dev)
    work = torch.empty(lib.ieee_rank_cuhk03_workspace_bytes(num_g), dtype=torch.uint8, device=dev)
    _lib.check(lib.ieee_rank_cuhk03(_lib.ptr(d), ldd, num_q, num_g, _lib.ptr(qp), _lib.ptr(gp), _lib.ptr(qk),
                                    _lib.ptr(gk), max_rank, _lib.ptr(cmc), _lib.ptr(ap), _lib.ptr(summary),
                                    _lib.ptr(work), work.numel(), _lib.stream()))
    s = summary.cpu().numpy()          # the single read-back
    return s[:max_rank].copy(), float(s[max_rank]), float(s[max_rank + 1]), cmc, ap


def eval_cuhk03(distmat, q_pids, g_pids, q_camids, g_camids, q_timeids, g_timeids, max_rank):
    """rank.py:24-100, as the EXPECTED value of what the reference samples.  The reference draws one gallery image per
    identity with np.random.choice, ten times per query, and averages the curves: a Monte-Carlo estimate that differs
    from run to run.  This returns the closed form it scatters around (a Poisson-binomial distribution function per
    true match, include/ieee_amd.h), deterministic and bitwise repeatable; the mAP is the reference's.  A query that
    sees fewer than max_rank gallery identities gets 1.0 in the tail of its curve -- the reference builds a ragged
    list there and fails.  q_timeids = g_timeids = None filters on identity and camera only (upstream Torchreid).
    distmat: numpy array or CUDA tensor.  Returns (float32[max_rank], float)."""
    num_g = distmat.shape[1]
    if num_g < max_rank:
        max_rank = num_g
        print('Note: number of gallery samples is quite small, got {}'.format(num_g))
    sums, num_valid_q, ap_sum, _, _ = cuhk03_sums(distmat, q_pids, g_pids, q_camids, g_camids, q_timeids, g_timeids,
                                                  max_rank)
    assert num_valid_q > 0, 'Error: all query identities do not appear in gallery'
    return (sums / num_valid_q).astype(np.float32), float(ap_sum / num_valid_q)


def eval_regdb(distmat, q_pids, g_pids, q_timeids, g_timeids, max_rank=20):
    """rank.py:175-230: the Market protocol with the cameras overwritten by 1 for every query and 2 for every gallery
    entry, so nothing is removed (the time ids are accepted and unused, as there; its debug prints are not kept)."""
    num_q, num_g = distmat.shape
    return eval_market1501(distmat, q_pids, g_pids, np.ones(num_q, dtype=np.int32), 2 * np.ones(num_g, dtype=np.int32),
                           max_rank)


def evaluate_py(distmat, q_pids, g_pids, q_camids, g_camids, max_rank, use_metric_cuhk03, q_timeids=None,
                g_timeids=None):
    """rank.py:233-243; its cuhk03 branch passes 6 of eval_cuhk03's 8 arguments and cannot run -- here the time ids
    come as two trailing arguments (None: filter on identity and camera only)."""
    if use_metric_cuhk03:
        return eval_cuhk03(distmat, q_pids, g_pids, q_camids, g_camids, q_timeids, g_timeids, max_rank)
    return eval_market1501(distmat, q_pids, g_pids, q_camids, g_camids, max_rank)


def evaluate_rank(distmat, q_pids, g_pids, q_camids, g_camids, max_rank=20, use_metric_cuhk03=False,
                  use_cython=True, q_timeids=None, g_timeids=None):
    """rank.py:246-287.  `use_cython` is accepted and ignored, as in the reference (:278-287).  q_timeids / g_timeids
    are read by the cuhk03 protocol only."""
    return evaluate_py(distmat, q_pids, g_pids, q_camids, g_camids, max_rank, use_metric_cuhk03, q_timeids, g_timeids)
