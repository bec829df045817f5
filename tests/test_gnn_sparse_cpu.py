"""CPU side of the sparse GNN re-ranking: the keyword checks that need no device, the signatures, the C ABI's
argument checks (nothing is launched), and the reference-side conditions tests/test_gnn_sparse_gpu.py relies on."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import util_gnn_rerank as ug

normalize = torch.nn.functional.normalize


def test_unknown_formulation_is_a_value_error_before_a_device_is_needed():
    from ieee_amd.engine import MultiModalImageSoftmaxEngine
    from ieee_amd.rerank import gnn_distmat, gnn_reranking
    x = np.zeros((4, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="formulation.*'bogus'"):
        gnn_distmat(x, x, formulation='bogus')
    with pytest.raises(ValueError, match="formulation.*'bogus'"):
        gnn_reranking(x, x, 3, 2, formulation='bogus')
    eng = MultiModalImageSoftmaxEngine.__new__(MultiModalImageSoftmaxEngine)     # test() checks before it touches self
    for kw in (dict(rerank='gnn'), dict()):
        with pytest.raises(ValueError, match="formulation.*'bogus'"):
            eng.test(rerank_formulation='bogus', **kw)
    with pytest.raises(ValueError, match="formulation.*'bogus'"):
        eng.run(test_only=True, rerank='gnn', rerank_formulation='bogus')
    with pytest.raises(ValueError, match="stream_eval=True cannot be combined with rerank"):
        eng.test(rerank='gnn', rerank_formulation='sparse', stream_eval=True)


def test_signatures():
    from ieee_amd.engine import Engine
    from ieee_amd.rerank import gnn_distmat, gnn_reranking, gnn_search_topk

    def defaults(fn):
        return [(n, p.default) for n, p in inspect.signature(fn).parameters.items() if n != "self"]
    E = inspect.Parameter.empty
    assert defaults(gnn_distmat) == [("X_q", E), ("X_g", E), ("k1", 26), ("k2", 7), ("precision", None),
                                     ("formulation", None), ("slab_rows", None)]
    assert defaults(gnn_reranking) == [("X_q", E), ("X_g", E), ("k1", E), ("k2", E), ("formulation", None)]
    assert defaults(gnn_search_topk) == [("X_q", E), ("X_g", E), ("k", E), ("k1", 26), ("k2", 7), ("q_pids", None),
                                         ("g_pids", None), ("q_camids", None), ("g_camids", None), ("precision", None),
                                         ("slab_rows", None)]
    for fn in (Engine.run, Engine.test, Engine._evaluate):
        assert dict(defaults(fn))["rerank_formulation"] is None


def test_search_checks_fire_before_a_device_is_needed():
    from ieee_amd.rerank import gnn_search_topk
    xq, xg = np.zeros((4, 8), dtype=np.float32), np.zeros((9, 8), dtype=np.float32)
    for k in (0, 1025, 2.5, True):
        with pytest.raises(ValueError, match="k must be an integer"):
            gnn_search_topk(xq, xg, k)
    with pytest.raises(ValueError, match="all four"):
        gnn_search_topk(xq, xg, 3, q_pids=np.zeros(4), g_pids=np.zeros(9))
    ok = dict(q_pids=np.zeros(4), g_pids=np.zeros(9), q_camids=np.zeros(4), g_camids=np.zeros(9))
    for name, wrong in (("q_pids", np.zeros(5)), ("g_camids", np.zeros(8)), ("g_pids", np.full(9, 2 ** 40))):
        with pytest.raises(ValueError, match=name):
            gnn_search_topk(xq, xg, 3, **dict(ok, **{name: wrong}))


def test_c_abi_argument_checks():
    from ieee_amd import _lib
    lib = _lib.load()
    for args, msg in (((10, 20, 4, 5), b"k2 out of range"), ((10, 20, 4, 0), b"k2 out of range"),
                      ((10, 20, 31, 3), b"k1 out of range"), ((10, 20, 1025, 3), b"k1 out of range"),
                      ((0, 20, 4, 2), b"empty"), ((10, 1 << 30, 4, 2), b"2^31")):
        assert lib.ieee_gnn_sparse_scratch_bytes(*args) == -1
        assert b"gnn_sparse" in lib.ieee_last_error() and msg in lib.ieee_last_error()
    # 512 work rows of N floats and N bits, rows padded to 256 bytes
    assert lib.ieee_gnn_sparse_scratch_bytes(10, 20, 4, 2) == 30 * 64 * 4
    assert lib.ieee_gnn_sparse_scratch_bytes(1000, 11000, 26, 7) == 512 * 12416 * 4
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)      # never dereferenced: the checks come before any launch
    assert lib.ieee_gnn_sparse_propagate_count(one, one, one, 30, 4, 5, one, 1 << 20, one, null) == -1
    assert b"gnn_sparse_propagate_count: k2" in lib.ieee_last_error()
    assert lib.ieee_gnn_sparse_propagate_count(one, one, one, 30, 31, 2, one, 1 << 20, one, null) == -1
    assert b"gnn_sparse_propagate_count: k1" in lib.ieee_last_error()
    assert lib.ieee_gnn_sparse_propagate_count(one, one, null, 30, 4, 2, one, 1 << 20, one, null) == -1
    assert b"null pointer" in lib.ieee_last_error()
    assert lib.ieee_gnn_sparse_symmetrise_count(one, one, one, one, 30, one, 100, one, null) == -1
    assert b"scratch too small" in lib.ieee_last_error()
    assert lib.ieee_gnn_sparse_cosine(one, one, one, one, one, one, one, 10, 20, 5, 5, one, 20, null) == -1
    assert b"gnn_sparse_cosine: range" in lib.ieee_last_error()
    assert lib.ieee_gnn_sparse_transpose(one, one, one, null, 1 << 31, 0, 1, one, one, one, one, 1, null) == -1
    assert b"gnn_sparse_transpose: N" in lib.ieee_last_error()


@pytest.mark.parametrize("case", ug.golden_cases()[:4], ids=lambda c: c[0])
def test_enough_clear_positions_in_the_goldens(case):
    name, xq, xg, k1, k2, _ = case
    assert k2 != 1
    r64, r32 = ug.restate(xq, xg, k1, k2, torch.float64), ug.restate(xq, xg, k1, k2, torch.float32)
    _, T = ug.tolerance(r32["sim"], r64["sim"])
    share = ug.clear_positions(r64["sim"], 2 * T).mean()
    print("%s: clear share %.3f" % (name, share))
    assert share >= 0.2
    N = len(xq) + len(xg)
    indegree = int((r64["rows"] != 0).sum(1).max())
    print("%s: longest final row %d of %d" % (name, indegree, N))
    assert indegree >= 0.8 * N           # rows as long as N are the normal case of these fixtures


@pytest.mark.parametrize("k1,k2,lo,hi", [(26, 7, 0.05, 0.5), (10, 3, 0.5, 0.99)])
def test_exact_zero_shares_are_not_trivial(k1, k2, lo, hi):
    """the shape of test_real_valued_descriptors whose pairs without a shared column test the exact 1.0"""
    Q, G = 333, 2001
    xq, xg, _, _ = ug.clustered_features(Q + G, Q, G, 64, 80)
    xq, xg = normalize(xq, p=2, dim=1), normalize(xg, p=2, dim=1)
    share = float((ug.restate(xq, xg, k1, k2, torch.float64)["sim"] == 0).double().mean())
    print("(%d, %d): exact zeros %.3f" % (k1, k2, share))
    assert lo < share < hi


def test_stored_entries_of_the_memory_fixture():
    """N = 12 000, dense in float32 on the host: the entries of the four stages together stay below N * ld / 8, so one
    dense matrix's memory holds them twice over with their indices (8 bytes an entry)"""
    Q, G, k1, k2 = 1000, 11000, 26, 7
    xq, xg, _, _ = ug.clustered_features(12, Q, G, 64, 500)
    X = torch.cat([normalize(xq, p=2, dim=1), normalize(xg, p=2, dim=1)])
    N = Q + G
    S, rank = torch.topk(X @ X.t(), k1, dim=1)
    A = torch.zeros((N, N))
    A.scatter_(1, rank, 1.0)
    W = S * S
    stored = []
    for _ in range(2):
        A += A.t().clone()
        stored.append(int(torch.count_nonzero(A)))
        P = torch.zeros_like(A)
        for j in range(k2):
            P.addcmul_(A[rank[:, j]], W[:, j:j + 1])
        stored.append(int(torch.count_nonzero(P)))
        A = P.div_(P.norm(p=2, dim=1, keepdim=True).clamp_min(1e-12))
        del P
    print("stored entries per stage %s, dense %d" % (stored, N * N))
    assert sum(stored) < N * N // 8
    assert stored[0] < stored[1] < stored[2] < stored[3]
