"""Test-side restatement of the reference's k-reciprocal re-ranking (torchreid/utils/rerank.py:31-113, oracle/rerank.py)
in sparse form: no N x N matrix, N = Q + G.  The rank lists come from the caller (a stable argsort of the normalised
rows: on the host for small cases, a chunked torch.sort(stable=True) on the device for large ones), the D values
from a gather function; the set logic, weights, query expansion and Jaccard sums follow oracle/rerank.py's numpy
operations, so on the same rank lists the result is that of oracle.re_ranking bit for bit."""
import numpy as np


def host_provider(qg, qq, gg):
    """(rank_fn(K), dgather(rows, cols), dq, colmax) from host matrices, with the oracle's float32 operations"""
    qg, qq, gg = (np.asarray(a, dtype=np.float32) for a in (qg, qq, gg))
    orig = np.concatenate([np.concatenate([qq, qg], axis=1), np.concatenate([qg.T, gg], axis=1)], axis=0)
    sq = np.power(orig, 2).astype(np.float32)
    colmax = np.max(sq, axis=0)
    D = np.transpose(1. * sq / colmax)
    Q = qg.shape[0]

    def rank_fn(K):
        return np.argsort(D, kind="stable")[:, :K].astype(np.int64)

    def dgather(rows, cols):
        return D[rows, cols]
    return rank_fn, dgather, D[:Q, Q:], colmax


def krecip_sets(rank, k1, chunk=4096):
    """per row the sorted unique expanded k-reciprocal set (rerank.py:56-79), vectorised over rows"""
    N = rank.shape[0]
    K, Kh = k1 + 1, int(np.around(k1 / 2.)) + 1
    fwd, hf = rank[:, :K], rank[:, :Kh]
    recip = np.zeros((N, K), dtype=bool)
    hrecip = np.zeros((N, Kh), dtype=bool)
    for r0 in range(0, N, chunk):
        ids = np.arange(r0, min(N, r0 + chunk))[:, None, None]
        recip[r0:r0 + chunk] = (rank[fwd[r0:r0 + chunk]][:, :, :K] == ids).any(-1)
        hrecip[r0:r0 + chunk] = (rank[hf[r0:r0 + chunk]][:, :, :Kh] == ids).any(-1)
    rset = np.where(recip, fwd, -1)                                   # R(i), -1 for the non-members
    take = np.zeros((N, K), dtype=bool)
    for r0 in range(0, N, chunk):
        m = fwd[r0:r0 + chunk]                                        # candidate members
        cand, cmask = hf[m], hrecip[m]                                # their half-size lists [n][K][Kh]
        inside = (cand[..., None] == rset[r0:r0 + chunk, None, None, :]).any(-1) & cmask
        take[r0:r0 + chunk] = recip[r0:r0 + chunk] & (inside.sum(-1) > 2. / 3 * cmask.sum(-1))
    sets = []
    for i in range(N):
        parts = [fwd[i][recip[i]]] + [hf[c][hrecip[c]] for c in fwd[i][take[i]]]
        sets.append(np.unique(np.concatenate(parts)))
    return sets


def re_ranking_sparse(rank, dgather, dq, k1=20, k2=6, lambda_value=0.3):
    """rank [N][>=k1+1] ints; dgather(rows, cols) -> float32 D[rows, cols]; dq [Q][G] = D[i][Q+g] float32.
    Returns (final [Q][G] float32, V, Vq): V and Vq as lists of (ascending columns, float32 values); Vq is V for k2 = 1."""
    rank = np.asarray(rank)
    N = rank.shape[0]
    Q, G = dq.shape
    sets = krecip_sets(rank, k1)
    lens = np.array([len(s) for s in sets])
    rows = np.repeat(np.arange(N), lens)
    dv = np.asarray(dgather(rows, np.concatenate(sets)), dtype=np.float32)
    V, at = [], 0
    for i in range(N):
        weight = np.exp(-dv[at:at + lens[i]])
        at += lens[i]
        V.append((sets[i], (1. * weight / np.sum(weight)).astype(np.float32)))
    Vq = V
    if k2 != 1:
        Vq = []
        for i in range(N):
            cols = np.concatenate([V[j][0] for j in rank[i, :k2]])
            vals = np.concatenate([V[j][1] for j in rank[i, :k2]])
            u, inv = np.unique(cols, return_inverse=True)
            acc = np.zeros(len(u), dtype=np.float32)
            np.add.at(acc, inv, vals)                                 # rows added in rank order, as np.mean does
            Vq.append((u, np.true_divide(acc, k2).astype(np.float32)))
    gal = [(Vq[j][0], np.full(len(Vq[j][0]), j - Q), Vq[j][1]) for j in range(Q, N)]
    c_all = np.concatenate([g[0] for g in gal])
    j_all = np.concatenate([g[1] for g in gal])
    v_all = np.concatenate([g[2] for g in gal])
    order = np.argsort(c_all, kind="stable")
    c_all, j_all, v_all = c_all[order], j_all[order], v_all[order]
    starts = np.searchsorted(c_all, np.arange(N + 1))
    jaccard = np.zeros((Q, G), dtype=np.float32)
    for i in range(Q):
        temp_min = np.zeros(G, dtype=np.float32)
        for c, a in zip(*Vq[i]):                                      # c ascending, the reference's order
            s, e = starts[c], starts[c + 1]
            temp_min[j_all[s:e]] = temp_min[j_all[s:e]] + np.minimum(a, v_all[s:e])
        jaccard[i] = 1 - temp_min / (2. - temp_min)
    final = jaccard * (1 - lambda_value) + dq * lambda_value
    return final, V, Vq
