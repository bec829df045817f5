"""float64 NumPy restatement of what ieee_rank_cuhk03 computes: the expected CMC curve of the CUHK03 single-gallery-shot
protocol (torchreid/metrics/rank.py:24-100 with the time-id filter) and the mAP of the kept list.

Per query: the gallery in a stable sort on distance (ties to the lower gallery index); entries with the query's
identity AND camera AND time id dropped; skipped when no kept entry has the query's identity.  The protocol draws one
kept image per identity uniformly and reads the CMC off the drawn list, so the rank of the drawn true match t is a sum
over the other identities j of independent Bernoulli(c_j(t) / n_j), c_j(t) = images of j before t, and

    cmc[r] = (1 / n_t) * sum_t P(sum_j B_j(t) <= r)

by the recurrence pmf'[k] = pmf[k] (1 - p) + pmf[k - 1] p over the identities in ascending-pid order, truncated at
max_rank terms (the terms below max_rank do not depend on where it is cut, so a curve for a smaller max_rank is a
prefix of one for a larger).  AP as rank.py:86-90.

`variant` selects a deliberately WRONG restatement (tests/test_cuhk03_cpu.py shows that each leaves the brute-force
bound): 'camera_only' filters on identity and camera alone, 'ties_le' counts c_j with <= on equal distances,
'all_true' averages over every true match, removed ones included."""
import itertools

import numpy as np


def _labels(q_camids, g_camids, q_timeids, g_timeids):
    qc, gc = np.asarray(q_camids).reshape(-1), np.asarray(g_camids).reshape(-1)
    qt = np.zeros(len(qc), dtype=np.int64) if q_timeids is None else np.asarray(q_timeids).reshape(-1)
    gt = np.zeros(len(gc), dtype=np.int64) if g_timeids is None else np.asarray(g_timeids).reshape(-1)
    return qc, gc, qt, gt


def cuhk03_reference(distmat, q_pids, g_pids, q_camids, g_camids, q_timeids, g_timeids, max_rank, variant=None):
    """returns dict(cmc float64[num_q][max_rank] (zeros when skipped), ap float64[num_q] (-1 when skipped),
    valid bool[num_q], n_true int[num_q], all_cmc float32[max_rank], mAP float, cmc_sum, ap_sum, num_valid)"""
    assert variant in (None, 'camera_only', 'ties_le', 'all_true')
    d = np.asarray(distmat)
    q_pids, g_pids = np.asarray(q_pids).reshape(-1), np.asarray(g_pids).reshape(-1)
    qc, gc, qt, gt = _labels(q_camids, g_camids, q_timeids, g_timeids)
    num_q, num_g = d.shape
    R = int(max_rank)
    ids = np.unique(g_pids)                                       # ascending
    members = [np.flatnonzero(g_pids == j) for j in ids]
    cmc = np.zeros((num_q, R), dtype=np.float64)
    ap = -np.ones(num_q, dtype=np.float64)
    n_true = np.zeros(num_q, dtype=np.int64)
    for q in range(num_q):
        row = d[q]
        order = np.argsort(row, kind='stable')
        pos = np.empty(num_g, dtype=np.int64)
        pos[order] = np.arange(num_g)
        same = g_pids == q_pids[q]
        remove = same & (gc == qc[q])
        if variant != 'camera_only':
            remove &= gt == qt[q]
        keep = ~remove
        true_kept = np.flatnonzero(same & keep)
        if len(true_kept) == 0:
            continue
        trues = np.flatnonzero(same) if variant == 'all_true' else true_kept
        curve = np.zeros(R, dtype=np.float64)
        for t in trues[np.argsort(pos[trues])]:
            pmf = np.zeros(R, dtype=np.float64)
            pmf[0] = 1.0
            for j, m in zip(ids, members):
                if j == q_pids[q]:
                    continue
                c = int(np.sum(row[m] <= row[t])) if variant == 'ties_le' else int(np.sum(pos[m] < pos[t]))
                if c == 0:
                    continue
                p = c / float(len(m))
                new = pmf * (1.0 - p)
                new[1:] += pmf[:-1] * p
                pmf = new
            curve += np.cumsum(pmf)
        cmc[q] = curve / len(trues)
        n_true[q] = len(true_kept)
        raw = same[order][keep[order]].astype(np.int64)           # rank.py:60-61
        tmp = raw.cumsum() / (np.arange(len(raw)) + 1.0)          # :87-88
        ap[q] = (tmp * raw).sum() / raw.sum()                     # :89-90
    valid = ap >= 0
    nv = int(valid.sum())
    out = dict(cmc=cmc, ap=ap, valid=valid, n_true=n_true, num_valid=nv, cmc_sum=cmc[valid].sum(0),
               ap_sum=float(ap[valid].sum()))
    if nv:
        out['all_cmc'] = (out['cmc_sum'] / nv).astype(np.float32)
        out['mAP'] = float(np.mean(ap[valid]))
    return out


def brute_force(distmat, q_pids, g_pids, q_camids, g_camids, q_timeids, g_timeids, max_rank):
    """the protocol itself, every joint draw enumerated: per valid query the exact mean of the CMC vectors of all
    prod_j n_j drawn lists (one kept image per identity), padded with ones past the list's end.  Returns
    (cmc float64[num_q][max_rank], valid bool[num_q]); keep the product of the counts small."""
    d = np.asarray(distmat)
    q_pids, g_pids = np.asarray(q_pids).reshape(-1), np.asarray(g_pids).reshape(-1)
    qc, gc, qt, gt = _labels(q_camids, g_camids, q_timeids, g_timeids)
    num_q, num_g = d.shape
    R = int(max_rank)
    cmc = np.zeros((num_q, R), dtype=np.float64)
    valid = np.zeros(num_q, dtype=bool)
    for q in range(num_q):
        order = np.argsort(d[q], kind='stable')
        keep = ~((g_pids[order] == q_pids[q]) & (gc[order] == qc[q]) & (gt[order] == qt[q]))
        kept_pids = g_pids[order][keep]
        raw = (kept_pids == q_pids[q]).astype(np.int64)
        if not raw.any():
            continue
        valid[q] = True
        groups = [np.flatnonzero(kept_pids == j) for j in np.unique(kept_pids)]
        hits = np.zeros(R, dtype=np.int64)
        draws = 0
        for pick in itertools.product(*groups):
            drawn = raw[np.sort(np.asarray(pick))]
            c = np.minimum(drawn.cumsum(), 1)
            full = np.ones(R, dtype=np.int64)
            full[:min(R, len(c))] = c[:R]
            hits += full
            draws += 1
        cmc[q] = hits / float(draws)
    return cmc, valid


def error_bound(num_ids, max_rank, n_true):
    """absolute bound on a per-query curve value or AP computed in float64: every value is at most 1, each step of the
    recurrence costs at most 3 roundings (num_ids steps), the sums over max_rank and over the true matches one each"""
    return (3.0 * num_ids + max_rank + n_true) * 2.0 ** -52
