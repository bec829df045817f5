"""k-reciprocal re-ranking from descriptors on the device (re_ranking_features, rerank_search_topk, ieee_rerank_stream_*):
bit for bit the matrix path -- re_ranking(cd(q, g), cd(q, q), cd(g, g), formulation='sparse') -- for every slab_rows,
on real-valued descriptors, on integer descriptors full of ties, for both metrics; the same intermediates; the top-k
without the matrix; the memory bound; and the Engine keyword."""
import re

import numpy as np
import pytest
import torch

from tests.test_rerank_sparse_gpu import _features, _sparse_state

pytestmark = pytest.mark.gpu


def _matrix_path(qf, gf, k1, k2, lam=0.3, metric="euclidean"):
    from ieee_amd.metrics.distance import compute_distance_matrix as cd
    from ieee_amd.rerank import re_ranking
    return re_ranking(cd(qf, gf, metric), cd(qf, qf, metric), cd(gf, gf, metric), k1=k1, k2=k2, lambda_value=lam,
                      formulation="sparse")


_CASES = [(150, 700, 20, 6), (64, 64, 8, 1), (97, 410, 63, 6), (50, 13, 62, 1), (60, 240, 9, 3), (40, 300, 63, 64)]


@pytest.mark.parametrize("Q,G,k1,k2", _CASES)
def test_same_bits_as_the_matrix_path(Q, G, k1, k2):
    from ieee_amd.rerank import re_ranking_features
    qf, gf = _features(Q + G, Q, G, 24, 9)
    want = _matrix_path(qf, gf, k1, k2)
    for slab_rows in (64, 100, None):
        got = re_ranking_features(qf, gf, k1=k1, k2=k2, slab_rows=slab_rows)
        assert got.dtype == torch.float32 and got.is_cuda and got.shape == (Q, G)
        assert torch.equal(got, want), slab_rows


def test_same_bits_with_a_padded_feature_axis_and_host_inputs():
    from ieee_amd.rerank import re_ranking_features
    Q, G, k1, k2 = 150, 700, 20, 6
    qf, gf = _features(Q + G, Q, G, 23, 9)                   # d = 23: padded to 24
    want = _matrix_path(qf, gf, k1, k2)
    for slab_rows in (64, 100, None):
        assert torch.equal(re_ranking_features(qf, gf, k1=k1, k2=k2, slab_rows=slab_rows), want), slab_rows
    # values that are no multiple of 4, exactly Q + G, and beyond it
    for slab_rows in (37, 850, 5000):
        assert torch.equal(re_ranking_features(qf, gf, k1=k1, k2=k2, slab_rows=slab_rows), want), slab_rows
    got = re_ranking_features(qf.cpu().numpy(), gf.cpu().double(), k1=k1, k2=k2, lambda_value=0.3, slab_rows=100)
    assert got.is_cuda and torch.equal(got, want)


@pytest.mark.parametrize("Q,G,k1,k2,slabs", [(80, 400, 20, 6, (64, 100)), (31, 250, 10, 1, (37, None))])
def test_same_bits_on_integer_ties(Q, G, k1, k2, slabs):
    """descriptors in {0, 1, 2}, d = 8: exact arithmetic, duplicate rows, zero distances, a handful of distinct squares,
    so the index decides most rank positions and distinct squares round to equal D"""
    from ieee_amd.rerank import re_ranking_features
    g = torch.Generator().manual_seed(Q * G)
    qf = torch.randint(0, 3, (Q, 8), generator=g).float().cuda()
    gf = torch.randint(0, 3, (G, 8), generator=g).float().cuda()
    gf[5] = qf[3]
    gf[G - 1] = gf[0]
    want = _matrix_path(qf, gf, k1, k2)
    for slab_rows in slabs:
        assert torch.equal(re_ranking_features(qf, gf, k1=k1, k2=k2, slab_rows=slab_rows), want), slab_rows


def test_same_bits_for_cosine():
    """the cosine epilogue is not symmetric in its operands: every block is produced with the matrix path's"""
    from ieee_amd.rerank import re_ranking_features
    Q, G, k1, k2 = 150, 700, 20, 6
    qf, gf = _features(Q + G, Q, G, 24, 9)
    want = _matrix_path(qf, gf, k1, k2, metric="cosine")
    assert torch.equal(re_ranking_features(qf, gf, k1=k1, k2=k2, metric="cosine", slab_rows=100), want)


@pytest.mark.parametrize("d", [24, 2304, 23])
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_pair_distances_have_the_matrix_bits(d, metric):
    """10 000 random pairs; asymmetric operands (m != n, another scale on each side) so that a swapped pair shows"""
    from ieee_amd.metrics import compute_distance_matrix, pair_distances
    m, n, pairs = 333, 517, 10000
    g = torch.Generator().manual_seed(d)
    a = (torch.randn(m, d, generator=g) * 1.5).cuda()
    b = (torch.randn(n, d, generator=g) + 0.25).cuda()
    i1, i2 = torch.randint(0, m, (pairs,), generator=g), torch.randint(0, n, (pairs,), generator=g)
    want = compute_distance_matrix(a, b, metric)[i1.cuda(), i2.cuda()]
    got = pair_distances(a, b, i1, i2, metric)
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == (pairs,)
    assert torch.equal(got, want)
    assert torch.equal(pair_distances(a, b, i1.cuda(), i2.numpy(), metric), want)
    some = pair_distances(a.cpu(), b.cpu(), i1[:37], i2[:37], metric)        # a partial tile; host inputs come back on the host
    assert not some.is_cuda and torch.equal(some, want[:37].cpu())
    assert pair_distances(a, b, i1[:0], i2[:0], metric).shape == (0,)


def test_search_topk_equals_rank_topk_of_the_matrix():
    from ieee_amd.metrics import rank_topk
    from ieee_amd.rerank import rerank_search_topk
    Q, G, k1, k2 = 60, 240, 9, 3
    qf, gf = _features(Q + G, Q, G, 24, 9)
    rng = np.random.RandomState(1)
    labels = dict(q_pids=rng.randint(0, 9, Q), g_pids=rng.randint(0, 9, G), q_camids=np.arange(Q) % 3,
                  g_camids=np.arange(G) % 3)
    full = _matrix_path(qf, gf, k1, k2)
    for k in (1, 10, 300):                                   # 300 > G: every row ends in -1 / +inf
        for kw in ({}, labels):
            want_i, want_d = rank_topk(full, k, **kw)
            if k == 300:
                assert bool((want_i == -1).any(dim=1).all())
            for slab_rows in (64, 100):
                got_i, got_d = rerank_search_topk(qf, gf, k, k1=k1, k2=k2, slab_rows=slab_rows, **kw)
                assert got_i.dtype == torch.int64 and got_d.dtype == torch.float32 and got_i.is_cuda
                assert torch.equal(got_i, want_i), (k, slab_rows)
                assert torch.equal(got_d.view(torch.int32), want_d.view(torch.int32)), (k, slab_rows)


def _stream_state(qf, gf, k1, k2, slab_rows):
    from ieee_amd.rerank import _rerank_stream, stream_layout
    st = _rerank_stream(qf, gf, k1, k2, "euclidean", slab_rows, None, "test")
    torch.cuda.synchronize()
    work, N = st["work"], st["Q"] + st["G"]
    L = stream_layout(st["Q"], st["G"], k1, k2, slab_rows)

    def view(off, n, dtype):
        return work[off:off + n * 4].view(dtype)
    rank = view(L["rank"], N * L["K"], torch.int32).view(N, L["K"]).cpu().numpy()

    def rows(pre, cap):
        n = view(L[pre + "_n"], N, torch.int32).cpu().numpy()
        idx = view(L[pre + "_idx"], N * cap, torch.int32).view(N, cap).cpu().numpy()
        val = view(L[pre + "_val"], N * cap, torch.float32).view(N, cap).cpu().numpy()
        return [(idx[r, :n[r]], val[r, :n[r]]) for r in range(N)]
    colmax = view(L["colmax"], N, torch.int32).cpu().numpy()
    return rank, rows("V", L["capV"]), rows("Vq", L["capVq"]), colmax


def test_intermediates_through_the_layout():
    from ieee_amd.metrics.distance import compute_distance_matrix as cd
    from ieee_amd.rerank import sparse_layout
    Q, G, k1, k2 = 150, 700, 20, 6
    qf, gf = _features(Q + G, Q, G, 24, 9)
    _, want_rank, want_V, want_Vq = _sparse_state(cd(qf, gf), cd(qf, qf), cd(gf, gf), k1, k2, 0.3)
    rank, V, Vq, colmax = _stream_state(qf, gf, k1, k2, 100)
    assert np.array_equal(rank, want_rank)
    assert colmax.min() > 0
    for r in range(Q + G):
        assert np.array_equal(V[r][0], want_V[r][0]), r
        assert np.array_equal(Vq[r][0], want_Vq[r][0]), r
        assert np.array_equal(V[r][1].view(np.int32), want_V[r][1].view(np.int32)), r     # and the values' bits
        assert np.array_equal(Vq[r][1].view(np.int32), want_Vq[r][1].view(np.int32)), r
    assert sparse_layout(Q, G, k1, k2)["capV"] == 21 * 12


def test_memory_stays_far_below_the_gallery_matrix():
    """Q = 200, G = 40 000: g_g_dist alone is 6.4 GB.  From descriptors the call stays below an eighth of that: the
    sparse workspace (about 271 MB), the output (32 MB), the descriptors and one 2048 x 2048 buffer."""
    from ieee_amd.rerank import re_ranking_features
    Q, G, d, k1, k2 = 200, 40000, 16, 10, 3
    qf, gf = _features(17, Q, G, d, 1500)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = re_ranking_features(qf, gf, k1=k1, k2=k2, slab_rows=2048)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak %.1f MB; the G x G matrix is %.1f MB" % (peak / 1e6, G * G * 4 / 1e6))
    assert peak < G * G * 4 // 8
    want = _matrix_path(qf, gf, k1, k2)
    assert torch.equal(got, want)
    del want
    torch.cuda.empty_cache()


def test_engine_rerank_from_descriptors(capsys):
    from ieee_amd.engine import MultiModalImageSoftmaxEngine
    from ieee_amd.models import build_model
    from ieee_amd.optim import build_optimizer
    Q, G = 100, 3000
    qf, gf = _features(11, Q, G, 32, 120)
    rng = np.random.RandomState(0)
    labels = {"query": (qf, rng.randint(0, 120, Q), np.zeros(Q, dtype=np.int64)),
              "gallery": (gf, rng.randint(0, 120, G), np.ones(G, dtype=np.int64))}

    class DM(object):
        num_train_pids = 10
        train_loader = []
        test_loader = {"synthetic": {"query": "query", "gallery": "gallery"}}
        sources = ["synthetic"]
    m = build_model("ieee3modalPart", num_classes=10, loss="softmax", pretrained=False, compute_dtype=torch.float32)
    eng = MultiModalImageSoftmaxEngine(DM(), m, build_optimizer(m, optim="sgd", lr=1e-3), use_gpu=True)
    eng._descriptors = lambda loader, clock: labels[loader]
    seen = {}
    for source in ("matrices", "descriptors"):
        mAP = eng.test(rerank=True, rerank_from=source, ranks=[1, 5])
        out = capsys.readouterr().out
        assert "Applying person re-ranking ..." in out and "(gnn)" not in out
        seen[source] = (mAP, re.search(r"Rank-1\s*: (\S+)", out).group(1), re.search(r"mAP: (\S+)", out).group(1))
    assert seen["descriptors"] == seen["matrices"]
    assert 0.0 < seen["descriptors"][0] <= 1.0
    # the keyword belongs to rerank=True alone
    plain = eng.test(ranks=[1], rerank_from="descriptors")
    assert "Applying person re-ranking" not in capsys.readouterr().out and plain == eng.test(ranks=[1])
