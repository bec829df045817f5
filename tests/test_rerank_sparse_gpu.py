"""Sparse k-reciprocal re-ranking on the device (ieee_rerank_sparse):
- bit for bit the dense ieee_rerank wherever that runs (goldens, device distance matrices, index ties, k2 = 1, k1 = 63,
  and a case near the dense limit);
- beyond the dense limit, the rank lists, the supports of V and Vq and the output of the sparse restatement
  (tests/util_rerank_sparse.py) fed with ranks from torch on the same device matrices;
- Engine.test(rerank=True) at a size the dense form refuses."""
import os

import numpy as np
import pytest
import torch

from tests import util_rerank_sparse as urs

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "rerank_golden.npz"))


def _both(qg, qq, gg, k1, k2, lam):
    from ieee_amd.rerank import re_ranking
    dense = re_ranking(qg, qq, gg, k1=k1, k2=k2, lambda_value=lam, formulation="dense")
    sparse = re_ranking(qg, qq, gg, k1=k1, k2=k2, lambda_value=lam, formulation="sparse")
    return dense, sparse


def _features(seed, Q, G, D, ids):
    g = torch.Generator().manual_seed(seed)
    centers = torch.randn(ids, D, generator=g) * 2.0
    qf = centers[torch.randint(0, ids, (Q,), generator=g)] + torch.randn(Q, D, generator=g)
    gf = centers[torch.randint(0, ids, (G,), generator=g)] + torch.randn(G, D, generator=g)
    return qf.cuda(), gf.cuda()


def _distmats(qf, gf):
    from ieee_amd.metrics.distance import compute_distance_matrix
    return compute_distance_matrix(qf, gf), compute_distance_matrix(qf, qf), compute_distance_matrix(gf, gf)


def test_sparse_equals_dense_on_goldens():
    for c in range(int(GOLD["cases"])):
        k1, k2, lam = GOLD["params%d" % c]
        args = [torch.from_numpy(GOLD[k + "%d" % c]).cuda() for k in ("qg", "qq", "gg")]
        dense, sparse = _both(*args, int(k1), int(k2), float(lam))
        assert torch.equal(dense, sparse), c
        np.testing.assert_allclose(sparse.cpu().numpy(), GOLD["final%d" % c], rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("Q,G,k1,k2", [(150, 700, 20, 6), (64, 64, 8, 1), (333, 1201, 20, 6), (97, 410, 63, 6),
                                       (40, 300, 63, 64), (50, 13, 62, 1),
                                       (60, 240, 9, 3), (120, 500, 21, 6)])   # odd k1, k1/2 = x.5: Kh rounds half to even
def test_sparse_equals_dense_on_device_distmats(Q, G, k1, k2):
    qg, qq, gg = _distmats(*_features(Q + G, Q, G, 24, 9))
    dense, sparse = _both(qg, qq, gg, k1, k2, 0.3)
    assert torch.equal(dense, sparse)


@pytest.mark.parametrize("Q,G,levels,k1,k2", [(80, 400, 3, 20, 6), (31, 250, 2, 10, 1), (64, 700, 5, 63, 20)])
def test_sparse_equals_dense_on_integer_ties(Q, G, levels, k1, k2):
    """few distinct distances: the index tie-break decides most rank positions, and D ties across distinct squares"""
    g = torch.Generator().manual_seed(Q * G + levels)
    qg, qq, gg = (torch.randint(0, levels, s, generator=g).float().cuda() for s in ((Q, G), (Q, Q), (G, G)))
    dense, sparse = _both(qg, qq, gg, k1, k2, 0.3)
    assert torch.equal(dense, sparse)


def test_sparse_equals_dense_near_the_dense_limit():
    qg, qq, gg = _distmats(*_features(7, 2000, 18000, 64, 400))
    dense, sparse = _both(qg, qq, gg, 20, 6, 0.3)
    assert torch.equal(dense, sparse)


def _orig_cols(qg, qq, gg, c0, c1):
    """orig[:, c0:c1] of the all-pairs matrix [[qq, qg], [qg^T, gg]], on the device"""
    Q = qq.shape[0]
    parts = []
    if c0 < Q:
        b = min(c1, Q)
        parts.append(torch.cat([qq[:, c0:b], qg[c0:b, :].T], 0))
    if c1 > Q:
        a = max(c0, Q)
        parts.append(torch.cat([qg[:, a - Q:c1 - Q], gg[:, a - Q:c1 - Q]], 0))
    return torch.cat(parts, 1)


def _torch_provider(qg, qq, gg, K, chunk=1024):
    """rank lists of the normalised rows by a chunked stable torch.sort, and a gather of D, on the same matrices"""
    N = qq.shape[0] + gg.shape[0]
    ranks, colmax = [], []
    for c0 in range(0, N, chunk):
        sq = _orig_cols(qg, qq, gg, c0, min(N, c0 + chunk))
        sq = sq * sq
        cm = sq.max(0).values
        D = (sq / cm).T.contiguous()
        ranks.append(torch.sort(D, dim=1, stable=True).indices[:, :K].cpu())
        colmax.append(cm)
    rank = torch.cat(ranks).numpy()
    colmax = torch.cat(colmax)
    Q = qq.shape[0]

    def dgather(rows, cols):
        r = torch.from_numpy(np.asarray(rows)).cuda()
        c = torch.from_numpy(np.asarray(cols)).cuda()
        v = torch.empty(r.shape, device="cuda")
        for rq in (False, True):
            for cq in (False, True):
                m = ((r < Q) == rq) & ((c < Q) == cq)       # D[r][c] = orig[c][r]^2 / colmax[r]
                rr, cc = r[m], c[m]
                if rq and cq:
                    x = qq[cc, rr]
                elif rq:
                    x = qg[rr, cc - Q]
                elif cq:
                    x = qg[cc, rr - Q]
                else:
                    x = gg[cc - Q, rr - Q]
                v[m] = x * x / colmax[rr]
        return v.cpu().numpy()
    dq = ((qg * qg) / colmax[:Q, None]).cpu().numpy()
    return rank, dgather, dq, colmax


def _sparse_state(qg, qq, gg, k1, k2, lam):
    from ieee_amd import _lib
    from ieee_amd.rerank import _sparse, sparse_layout
    Q, G = qg.shape
    out, work = _sparse(_lib.require_gpu(), qg, qq, gg, Q, G, k1, k2, lam)
    torch.cuda.synchronize()
    L = sparse_layout(Q, G, k1, k2)
    N, K = Q + G, L["K"]

    def view(off, n, dtype):
        return work[off:off + n * 4].view(dtype)
    rank = view(L["rank"], N * K, torch.int32).view(N, K).cpu().numpy()

    def rows(pre, cap):
        n = view(L[pre + "_n"], N, torch.int32).cpu().numpy()
        idx = view(L[pre + "_idx"], N * cap, torch.int32).view(N, cap).cpu().numpy()
        val = view(L[pre + "_val"], N * cap, torch.float32).view(N, cap).cpu().numpy()
        return [(idx[r, :n[r]], val[r, :n[r]]) for r in range(N)]
    V = rows("V", L["capV"])
    Vq = rows("Vq", L["capVq"]) if k2 != 1 else V
    return out, rank, V, Vq


@pytest.mark.parametrize("k2", [6, 1])
def test_sparse_beyond_the_dense_limit_matches_the_restatement(k2):
    from ieee_amd.rerank import re_ranking
    Q, G, k1 = 500, 47000, 20
    qg, qq, gg = _distmats(*_features(3, Q, G, 32, 1500))
    out, rank, V, Vq = _sparse_state(qg, qq, gg, k1, k2, 0.3)
    if k2 == 6:     # the default formulation switches to sparse here, and returns the same bits
        assert torch.equal(re_ranking(qg, qq, gg), out)
    trank, dgather, dq, colmax = _torch_provider(qg, qq, gg, k1 + 1)
    assert np.array_equal(rank, trank)
    want, tV, tVq = urs.re_ranking_sparse(trank, dgather, dq, k1, k2, 0.3)
    for r in range(Q + G):
        assert np.array_equal(V[r][0], tV[r][0]), r
        assert np.array_equal(Vq[r][0], tVq[r][0]), r
    np.testing.assert_allclose(V[Q][1], tV[Q][1], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=5e-5, atol=5e-6)
    del qg, qq, gg
    torch.cuda.empty_cache()


def test_engine_test_rerank_beyond_the_dense_limit(capsys):
    from ieee_amd.engine import MultiModalImageSoftmaxEngine
    from ieee_amd.models import build_model
    from ieee_amd.optim import build_optimizer
    Q, G = 400, 46000
    qf, gf = _features(11, Q, G, 32, 1200)
    rng = np.random.RandomState(0)
    labels = {"query": (qf, rng.randint(0, 1200, Q), np.zeros(Q, dtype=np.int64)),
              "gallery": (gf, rng.randint(0, 1200, G), np.ones(G, dtype=np.int64))}

    class DM(object):
        num_train_pids = 10
        train_loader = []
        test_loader = {"synthetic": {"query": "query", "gallery": "gallery"}}
        sources = ["synthetic"]
    m = build_model("ieee3modalPart", num_classes=10, loss="softmax", pretrained=False, compute_dtype=torch.float32)
    eng = MultiModalImageSoftmaxEngine(DM(), m, build_optimizer(m, optim="sgd", lr=1e-3), use_gpu=True)
    eng._descriptors = lambda loader, clock: labels[loader]
    mAP = eng.test(rerank=True, ranks=[1, 5])
    out = capsys.readouterr().out
    assert "Applying person re-ranking ..." in out and "mAP:" in out and "Rank-1" in out
    assert 0.0 <= mAP <= 1.0
