"""The sparse restatement of k-reciprocal re-ranking (tests/util_rerank_sparse.py) against the oracle, bit for bit, and
the argument checks of the sparse C ABI (ieee_rerank_sparse and its workspace query) that run without a device."""
import ctypes
import os

import numpy as np
import pytest

from oracle import rerank as orr
from tests import util_rerank_sparse as urs

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "rerank_golden.npz"))


def _sparse_on_host(qg, qq, gg, k1, k2, lam):
    rank_fn, dgather, dq, _ = urs.host_provider(qg, qq, gg)
    return urs.re_ranking_sparse(rank_fn(k1 + 1), dgather, dq, k1, k2, lam)


def test_restatement_equals_reference_goldens():
    for c in range(int(GOLD["cases"])):
        k1, k2, lam = GOLD["params%d" % c]
        got, _, _ = _sparse_on_host(GOLD["qg%d" % c], GOLD["qq%d" % c], GOLD["gg%d" % c], int(k1), int(k2), float(lam))
        assert got.dtype == np.float32 and np.array_equal(got, GOLD["final%d" % c])


def _sq(a, b):
    return np.maximum(((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)), 0).astype(np.float32)


def _clustered(seed, Q, G, D=16, ids=8):
    rng = np.random.RandomState(seed)
    centers = rng.randn(ids, D) * 2.0
    qf = centers[rng.randint(0, ids, Q)] + rng.randn(Q, D)
    gf = centers[rng.randint(0, ids, G)] + rng.randn(G, D)
    qq, gg = _sq(qf, qf), _sq(gf, gf)
    np.fill_diagonal(qq, 0)
    np.fill_diagonal(gg, 0)
    return _sq(qf, gf), qq, gg


def _grid(seed, Q, G, levels=4):
    """integer distances from a handful of levels: most ranks are decided by the index tie-break"""
    rng = np.random.RandomState(seed)
    qg = rng.randint(0, levels, (Q, G)).astype(np.float32)
    qq = rng.randint(0, levels, (Q, Q)).astype(np.float32)
    gg = rng.randint(0, levels, (G, G)).astype(np.float32)
    return qg, qq, gg


@pytest.mark.parametrize("case,Q,G,k1,k2,lam", [
    ("clustered", 30, 90, 20, 6, 0.3),
    ("clustered", 17, 60, 8, 1, 0.5),          # k2 = 1: V itself feeds the Jaccard sum
    ("clustered", 40, 110, 63, 64, 0.3),       # k1 = 63, k2 = k1 + 1
    ("clustered", 10, 54, 63, 6, 0.2),         # k1 + 1 = N
    ("grid", 25, 75, 20, 6, 0.3),
    ("grid", 12, 40, 10, 3, 0.3),
    ("grid", 6, 18, 5, 1, 0.7),
])
def test_restatement_equals_oracle(case, Q, G, k1, k2, lam):
    qg, qq, gg = (_clustered if case == "clustered" else _grid)(Q * 1000 + G, Q, G)
    want = orr.re_ranking(qg, qq, gg, k1, k2, lam)
    got, V, Vq = _sparse_on_host(qg, qq, gg, k1, k2, lam)
    assert np.array_equal(got, want)
    assert len(V) == Q + G and all(np.all(np.diff(v[0]) > 0) for v in Vq)


def _load_lib():
    from ieee_amd import _lib
    return _lib.load()


def test_workspace_query_contract():
    lib = _load_lib()
    ws = lib.ieee_rerank_sparse_workspace_bytes
    # the project's evaluation size fits the stated 4 GB
    big = ws(10000, 100000, 20, 6)
    assert 0 < big <= 4 * 1024 ** 3
    # data-independent and monotone in the sizes; k2 = 1 needs no Vq rows
    assert ws(500, 47000, 20, 6) == ws(500, 47000, 20, 6)
    assert ws(500, 47000, 20, 1) < ws(500, 47000, 20, 6) <= ws(600, 47000, 20, 6)
    for bad in [(0, 10, 5, 1), (10, 0, 5, 1), (10, 10, 0, 1), (10, 10, 64, 1), (3, 3, 6, 1), (10, 10, 5, 0),
                (10, 10, 5, 7), (1 << 30, 1 << 30, 20, 6)]:
        assert ws(*bad) == -1, bad
        assert b"rerank_sparse" in lib.ieee_last_error()


def test_abi_rejects_bad_arguments_before_any_launch():
    lib = _load_lib()
    from ieee_amd import _lib
    p = ctypes.c_void_p(16)                    # never dereferenced: every call below fails its argument check
    nul = ctypes.c_void_p(0)
    big = 1 << 40

    def call(qg=p, Q=10, G=20, k1=5, k2=2, out=p, work=p, nbytes=big):
        return lib.ieee_rerank_sparse(qg, p, p, Q, G, k1, k2, 0.3, out, work, nbytes, nul)
    for kw, msg in [(dict(qg=nul), b"null pointer"), (dict(out=nul), b"null pointer"), (dict(work=nul), b"null pointer"),
                    (dict(Q=0), b"empty"), (dict(G=-1), b"empty"), (dict(k1=0), b"k1"), (dict(k1=64), b"k1"),
                    (dict(Q=2, G=3, k1=5), b"k1"), (dict(k2=0), b"k2"), (dict(k2=7), b"k2"),
                    (dict(Q=1 << 30, G=1 << 30), b"2^31"), (dict(nbytes=1024), b"workspace too small")]:
        assert call(**kw) != 0, kw
        assert msg in lib.ieee_last_error(), (kw, lib.ieee_last_error())
    with pytest.raises(_lib.IeeeAmdError):
        _lib.check(call(k2=0))
    fields = (ctypes.c_int64 * 11)()
    assert lib.ieee_rerank_sparse_layout(10, 20, 5, 2, ctypes.cast(fields, ctypes.c_void_p)) == 0
    K, capV, capVq = fields[0], fields[1], fields[2]
    assert (K, capV, capVq) == (6, 6 * (1 + 3), 30)       # Kh = round_half_even(2.5) + 1 = 3
    assert lib.ieee_rerank_sparse_layout(10, 20, 0, 2, ctypes.cast(fields, ctypes.c_void_p)) != 0


def test_re_ranking_rejects_an_unknown_formulation():
    from ieee_amd.rerank import re_ranking
    with pytest.raises(ValueError, match="formulation"):
        re_ranking(np.zeros((2, 3)), np.zeros((2, 2)), np.zeros((3, 3)), k1=2, k2=1, formulation="csr")
