"""GNN re-ranking without a device: the package's dense restatement (tests/util_gnn_rerank.py) against the reference's
own ranking lists (tests/golden/gnn_rerank_golden.npz), the argument checks and the workspace formula of the C ABI
(ieee_gnn_rerank, ieee_gnn_rerank_workspace_bytes), and the engine's check of its rerank keyword."""
import ctypes

import numpy as np
import pytest
import torch

from tests import util_gnn_rerank as ug

CASES = ug.golden_cases()


@pytest.mark.parametrize("case", [c for c in CASES if c[4] != 1], ids=lambda c: c[0])
def test_restatement_reproduces_the_reference_lists(case):
    """float64, every clear position: the similarity there differs from both sorted neighbours by more than 2 T"""
    _, xq, xg, k1, k2, L = case
    r64, r32 = ug.restate(xq, xg, k1, k2, torch.float64), ug.restate(xq, xg, k1, k2, torch.float32)
    err32, T = ug.tolerance(r32["sim"], r64["sim"])
    clear = ug.clear_positions(r64["sim"], 2 * T)
    print("%s: err32 %.3g T %.3g clear share %.3f" % (case[0], err32, T, clear.mean()))
    assert clear.mean() >= 0.2
    mine = ug.ranking(r64["sim"])
    assert np.array_equal(mine[clear], L[clear])


@pytest.mark.parametrize("case", [c for c in CASES if c[4] == 1], ids=lambda c: c[0])
def test_restatement_counts_shared_neighbours_when_k2_is_1(case):
    _, xq, xg, k1, k2, L = case
    r = ug.restate(xq, xg, k1, k2, torch.float64)
    B = np.zeros((len(xq) + len(xg),) * 2, dtype=np.int64)
    np.put_along_axis(B, r["rank"].numpy(), 1, axis=1)
    counts = B[:len(xq)] @ B[len(xq):].T
    assert np.array_equal(r["sim"].numpy(), counts.astype(np.float64))
    clear = ug.clear_positions(r["sim"], 0.5)          # integers: the count differs from both neighbours'
    assert clear.any()
    assert np.array_equal(ug.ranking(r["sim"])[clear], L[clear])


def _lib():
    from ieee_amd import _lib
    return _lib.load()


def test_workspace_formula_and_bad_arguments():
    lib = _lib()
    ws = lib.ieee_gnn_rerank_workspace_bytes
    for Q, G, d, k1, k2 in [(60, 400, 32, 26, 7), (333, 2001, 2304, 26, 7), (3368, 19732, 2304, 26, 7), (5, 6, 8, 1, 1),
                            (100, 1000, 64, 1024, 1024)]:
        N = Q + G
        ld = (N + 7) // 8 * 8
        got = ws(Q, G, d, k1, k2, 0)
        assert 2 * N * ld * 4 <= got < 2 * N * ld * 4 + 64 * N * k1 + 4096, (Q, G, got)
        for scheme in (6, 3, 2):     # IEEE_SPLIT_*: what the two GEMMs' split operands ask for, on top
            extra = max(lib.ieee_sqeuclid_distmat_split_workspace_bytes(N, N, d, scheme),
                        lib.ieee_sqeuclid_distmat_split_workspace_bytes(Q, G, ld, scheme))
            assert got - 8 * N < ws(Q, G, d, k1, k2, scheme) <= got + extra + 256
    for bad in [(0, 10, 8, 5, 1, 0), (10, 0, 8, 5, 1, 0), (10, 10, 12, 5, 1, 0), (10, 10, 0, 5, 1, 0), (10, 10, 8, 0, 1, 0),
                (600, 600, 8, 1025, 1, 0), (3, 3, 8, 7, 1, 0), (10, 10, 8, 5, 0, 0), (10, 10, 8, 5, 6, 0),
                (10, 10, 8, 5, 2, 1), (1 << 30, 1 << 30, 8, 5, 2, 0)]:
        assert ws(*bad) == -1, bad
        assert b"gnn_rerank" in lib.ieee_last_error()


def test_abi_rejects_bad_arguments_before_any_launch():
    lib = _lib()
    from ieee_amd import _lib as binding
    p = ctypes.c_void_p(16)                    # never dereferenced: every call below fails its argument check
    nul = ctypes.c_void_p(0)

    def call(xq=p, xg=p, Q=10, G=20, d=16, k1=5, k2=2, precision=0, out=p, work=p, nbytes=1 << 40):
        return lib.ieee_gnn_rerank(xq, xg, Q, G, d, k1, k2, precision, out, work, nbytes, nul)
    for kw, msg in [(dict(xq=nul), b"null pointer"), (dict(xg=nul), b"null pointer"), (dict(out=nul), b"null pointer"),
                    (dict(work=nul), b"null pointer"), (dict(Q=0), b"empty"), (dict(G=-1), b"empty"),
                    (dict(d=12), b"multiple of 8"), (dict(k1=0), b"k1"), (dict(Q=600, G=600, k1=1025), b"k1"),
                    (dict(Q=2, G=3, k1=6), b"k1"), (dict(k2=0), b"k2"), (dict(k2=6), b"k2"),
                    (dict(precision=5), b"precision"), (dict(nbytes=1024), b"workspace too small")]:
        assert call(**kw) == -1, kw            # IEEE_ERR_BAD_ARG
        assert msg in lib.ieee_last_error(), (kw, lib.ieee_last_error())
    with pytest.raises(binding.IeeeAmdError):
        binding.check(call(k2=0))
    fields = (ctypes.c_int64 * 7)()
    assert lib.ieee_gnn_rerank_layout(10, 20, 16, 5, 2, 0, ctypes.cast(fields, ctypes.c_void_p)) == 0
    ld, rank, S, sumsq, m0, m1, rows = fields
    assert ld == 32 and rows == m1 and m1 - m0 >= 30 * 32 * 4 and S - rank >= 30 * 5 * 4
    assert lib.ieee_gnn_rerank_layout(10, 20, 16, 5, 1, 0, ctypes.cast(fields, ctypes.c_void_p)) == 0
    assert fields[6] == fields[4]              # k2 = 1: the binary stage-1 rows feed the final product
    assert lib.ieee_gnn_rerank_layout(10, 20, 16, 5, 6, 0, ctypes.cast(fields, ctypes.c_void_p)) != 0


def test_engine_rejects_an_unknown_rerank_string_before_extracting():
    from ieee_amd.engine import Engine

    class DM(object):
        num_train_pids = 3
        sources = ["synthetic"]
        train_loader = []
        test_loader = {"synthetic": {"query": "query", "gallery": "gallery"}}
    eng = Engine(DM(), use_gpu=False)
    seen = []
    eng._descriptors = lambda loader, clock: seen.append(loader)
    with pytest.raises(ValueError, match="rerank"):
        eng.test(rerank='bogus')
    with pytest.raises(ValueError, match="rerank"):
        eng.run(test_only=True, rerank='k-reciprocal')
    assert seen == []
