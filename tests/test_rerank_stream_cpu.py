"""k-reciprocal re-ranking from descriptors (ieee_amd.rerank.re_ranking_features, rerank_search_topk; the
ieee_rerank_stream_* calls): what needs no device -- every argument check, the Engine keyword, the signatures, the
block schedule of the strip passes and the argument checks of the C ABI."""
import ctypes
import inspect

import numpy as np
import pytest


def _x(Q=4, G=9, d=8):
    return np.zeros((Q, d), dtype=np.float32), np.zeros((G, d), dtype=np.float32)


def test_value_errors_before_a_device_is_needed(monkeypatch):
    from ieee_amd.rerank import re_ranking_features, rerank_search_topk
    monkeypatch.delenv("IEEE_DISTMAT_PRECISION", raising=False)
    xq, xg = _x()
    calls = (lambda **kw: re_ranking_features(xq, xg, **kw), lambda **kw: rerank_search_topk(xq, xg, 3, **kw))
    for call in calls:
        with pytest.raises(ValueError, match="metric"):
            call(k1=5, k2=2, metric="manhattan")
        for precision in ("bf16x3", "f16x2", "bf16", "fp64"):
            with pytest.raises(ValueError, match="precision"):
                call(k1=5, k2=2, precision=precision)
        for slab in (0, -4, 2.5, True):
            with pytest.raises(ValueError, match="slab_rows"):
                call(k1=5, k2=2, slab_rows=slab)
        for k1 in (0, 64, 13, 2.5):                          # k1 + 1 <= 64, and k1 + 1 <= Q + G = 13
            with pytest.raises(ValueError, match="k1"):
                call(k1=k1, k2=1)
        for k2 in (0, 7, -1):                                # 1 <= k2 <= k1 + 1 = 6
            with pytest.raises(ValueError, match="k2"):
                call(k1=5, k2=k2)
    with pytest.raises(ValueError, match=r"X_q \[Q, d\]"):
        re_ranking_features(xq, np.zeros((9, 7), dtype=np.float32), k1=5, k2=2)
    with pytest.raises(ValueError, match=r"X_q \[Q, d\]"):
        re_ranking_features(np.zeros(8, dtype=np.float32), xg, k1=5, k2=2)
    with pytest.raises(ValueError, match="empty"):
        re_ranking_features(np.zeros((0, 8), dtype=np.float32), xg, k1=5, k2=2)
    for k in (0, 1025, 2.5, True):
        with pytest.raises(ValueError, match="k must be"):
            rerank_search_topk(xq, xg, k, k1=5, k2=2)
    with pytest.raises(ValueError, match="all four"):
        rerank_search_topk(xq, xg, 3, k1=5, k2=2, q_pids=np.zeros(4))
    with pytest.raises(ValueError, match="g_pids has 8 entries"):
        rerank_search_topk(xq, xg, 3, k1=5, k2=2, q_pids=np.zeros(4), q_camids=np.zeros(4), g_pids=np.zeros(8),
                           g_camids=np.zeros(9))


def test_pair_distances_checks_before_a_device_is_needed():
    import torch
    from ieee_amd.metrics import pair_distances
    from ieee_amd.metrics.distance import pair_distances as same
    assert pair_distances is same
    a, b = torch.zeros(4, 8), torch.zeros(9, 8)
    ok = torch.tensor([0, 1])
    with pytest.raises(ValueError, match="metric"):
        pair_distances(a, b, ok, ok, metric="manhattan")
    with pytest.raises(ValueError, match=r"input1 \[m, d\]"):
        pair_distances(a, torch.zeros(9, 7), ok, ok)
    with pytest.raises(ValueError, match=r"input1 \[m, d\]"):
        pair_distances(a, torch.zeros(0, 8), ok, ok)
    with pytest.raises(ValueError, match=r"idx1 has entries outside \[0, 4\)"):
        pair_distances(a, b, torch.tensor([0, 4]), ok)
    with pytest.raises(ValueError, match=r"idx2 has entries outside \[0, 9\)"):
        pair_distances(a, b, ok, np.array([-1, 3]))
    with pytest.raises(ValueError, match="1-D integer"):
        pair_distances(a, b, torch.tensor([0.0, 1.0]), ok)
    with pytest.raises(ValueError, match="1-D integer"):
        pair_distances(a, b, ok.view(1, 2), ok)
    with pytest.raises(ValueError, match="2 row indices for 3 column indices"):
        pair_distances(a, b, ok, torch.tensor([0, 1, 2]))


def test_precision_from_the_environment_is_checked_too(monkeypatch):
    from ieee_amd.rerank import re_ranking_features
    xq, xg = _x()
    monkeypatch.setenv("IEEE_DISTMAT_PRECISION", "bf16x3")
    with pytest.raises(ValueError, match="precision"):
        re_ranking_features(xq, xg, k1=5, k2=2)
    with pytest.raises(ValueError, match="precision"):
        re_ranking_features(xq, xg, k1=5, k2=2, precision="f16x2")


def test_engine_keyword():
    from ieee_amd.engine import MultiModalImageSoftmaxEngine
    eng = MultiModalImageSoftmaxEngine.__new__(MultiModalImageSoftmaxEngine)     # the checks come before self is touched
    for kw in (dict(rerank=True), dict(rerank='gnn'), dict()):
        with pytest.raises(ValueError, match="rerank_from.*'bogus'"):
            eng.test(rerank_from='bogus', **kw)
        with pytest.raises(ValueError, match="rerank_from.*'bogus'"):
            eng._evaluate(rerank_from='bogus', **kw)
        with pytest.raises(ValueError, match="rerank_from.*'bogus'"):
            eng.run(test_only=True, rerank_from='bogus', **kw)
    for rerank in (True, 'gnn'):                             # stream_eval with any rerank raises as before
        with pytest.raises(ValueError, match="stream_eval=True cannot be combined with rerank"):
            eng.test(stream_eval=True, rerank=rerank, rerank_from='descriptors')


def test_signatures():
    from ieee_amd.engine import Engine
    from ieee_amd.rerank import re_ranking_features, rerank_search_topk

    def defaults(fn):
        return [(n, p.default) for n, p in inspect.signature(fn).parameters.items() if n != "self"]
    E = inspect.Parameter.empty
    assert defaults(re_ranking_features) == [("X_q", E), ("X_g", E), ("k1", 20), ("k2", 6), ("lambda_value", 0.3),
                                             ("metric", "euclidean"), ("slab_rows", None), ("precision", None)]
    assert defaults(rerank_search_topk) == [("X_q", E), ("X_g", E), ("k", E), ("k1", 20), ("k2", 6), ("lambda_value", 0.3),
                                            ("metric", "euclidean"), ("q_pids", None), ("g_pids", None),
                                            ("q_camids", None), ("g_camids", None), ("slab_rows", None),
                                            ("precision", None)]
    for fn in (Engine.run, Engine.test, Engine._evaluate):
        assert dict(defaults(fn))["rerank_from"] == 'matrices'


@pytest.mark.parametrize("N", [1, 63, 64, 65, 763])
def test_schedule_covers_every_pair_exactly_once(N):
    from ieee_amd.rerank import stream_pieces, stream_schedule
    for slab in (1, 4, 100, N, 2 * N):
        for cut in sorted({None, 1, N // 3, N - 1} - {0}, key=lambda c: -1 if c is None else c):
            if cut is not None and not 0 < cut < N:
                continue
            blocks = stream_schedule(N, slab, cut)
            seen = np.zeros((N, N), dtype=np.int32)
            for a0, a1, i0, i1 in blocks:
                assert 0 <= a0 < a1 <= N and 0 <= i0 < i1 <= N
                assert a1 - a0 <= slab and i1 - i0 <= slab
                if cut is not None:                          # a block lies in one quadrant
                    assert (a1 <= cut or a0 >= cut) and (i1 <= cut or i0 >= cut)
                seen[a0:a1, i0:i1] += 1
            assert (seen == 1).all(), (N, slab, cut)
            # strip-major: all the slabs of one strip come together, so a strip's column maxima can be finished first
            strips = [b[2:] for b in blocks]
            assert strips == sorted(strips) and stream_schedule(N, slab, cut) == blocks
            assert sorted(set(strips)) == stream_pieces(N, slab, cut)


def test_default_slab_keeps_one_buffer_within_the_budget():
    from ieee_amd.metrics._stream import SLAB_BUDGET_BYTES
    from ieee_amd.rerank import stream_slab_rows
    s = stream_slab_rows(None)
    assert s % 128 == 0 and s * s * 4 <= SLAB_BUDGET_BYTES < (s + 128) * (s + 128) * 4
    assert stream_slab_rows(7) == 7


def test_c_abi_argument_checks():
    from ieee_amd import _lib
    lib = _lib.load()
    ws = lib.ieee_rerank_stream_workspace_bytes
    for Q, G, k1, k2, slab in ((0, 5, 2, 1, 4), (5, 0, 2, 1, 4), (5, 5, 0, 1, 4), (5, 5, 64, 1, 4), (3, 3, 6, 1, 4),
                               (5, 5, 4, 0, 4), (5, 5, 4, 6, 4), (5, 5, 4, 2, 0), (2 ** 30, 2 ** 30, 4, 2, 4)):
        assert ws(Q, G, k1, k2, slab) == -1
        assert b"rerank_stream" in lib.ieee_last_error()
    # the plan is the sparse one with the union region laid out for one strip and one gallery range
    small, large = ws(200, 40000, 10, 3, 2048), ws(200, 40000, 10, 3, 40200)
    assert 0 < small <= large and small <= lib.ieee_rerank_sparse_workspace_bytes(200, 40000, 10, 3)
    fields, sparse = (ctypes.c_int64 * 14)(), (ctypes.c_int64 * 11)()
    assert lib.ieee_rerank_stream_layout(10, 20, 5, 2, 8, ctypes.cast(fields, ctypes.c_void_p)) == 0
    assert lib.ieee_rerank_sparse_layout(10, 20, 5, 2, ctypes.cast(sparse, ctypes.c_void_p)) == 0
    assert list(fields)[:11] == list(sparse) and list(fields)[12:] == [8, 8]
    assert lib.ieee_rerank_stream_layout(10, 20, 5, 2, 0, ctypes.cast(fields, ctypes.c_void_p)) != 0
    one = ctypes.c_void_p(256)                               # never dereferenced: every call below fails its checks first
    nul = ctypes.c_void_p(0)
    n = ws(10, 20, 5, 2, 8)
    tail = (10, 20, 5, 2, 8, one, n, nul)
    assert lib.ieee_rerank_stream_begin(10, 20, 5, 2, 8, one, n - 1, nul) != 0
    assert b"workspace too small" in lib.ieee_last_error()
    assert lib.ieee_rerank_stream_begin(10, 20, 5, 2, 8, nul, n, nul) != 0
    for bad in ((2, one, 8, 1, 0, 8, 0, 8),                  # pass
                (0, nul, 8, 1, 0, 8, 0, 8),                  # buffer
                (0, one, 8, 1, 0, 9, 0, 8),                  # more rows than the slab
                (0, one, 8, 1, 0, 8, 8, 17),                 # more columns than the slab
                (0, one, 8, 1, 24, 31, 0, 8),                # rows past N
                (0, one, 4, 1, 0, 8, 0, 8),                  # row stride shorter than the row
                (0, one, 1, 4, 0, 8, 0, 8),
                (0, one, 8, 8, 0, 8, 0, 8)):                 # no unit stride
        assert lib.ieee_rerank_stream_block(*bad, *tail) != 0
        assert b"rerank_stream_block" in lib.ieee_last_error()
    for bad in ((nul, one, 4, 9, 8, one, one, 5, 0, one, one), (one, one, 0, 9, 8, one, one, 5, 0, one, one),
                (one, one, 4, 9, 7, one, one, 5, 0, one, one), (one, one, 4, 9, 8, one, one, 5, 3, one, one),
                (one, one, 4, 9, 8, one, one, -1, 0, one, one), (one, one, 4, 9, 8, nul, one, 5, 0, one, one)):
        assert lib.ieee_distmat_pairs(*bad, nul) != 0
        assert b"distmat_pairs" in lib.ieee_last_error()
    for bad in ((nul, 30, 8, 10, one, one, 12, 0, one, one), (one, 30, 12, 10, one, one, 12, 0, one, one),
                (one, 30, 8, 31, one, one, 12, 0, one, one), (one, 30, 8, 10, one, one, 0, 0, one, one),
                (one, 30, 8, 10, one, one, 12, 2, one, one)):
        assert lib.ieee_distmat_member_pairs(*bad, nul) != 0
        assert b"distmat_member_pairs" in lib.ieee_last_error()
    for bad in ((one, 8, 0, 9, 0.3, one, 9), (one, 4, 0, 8, 0.3, one, 8), (one, 8, 0, 8, 0.3, one, 4),
                (one, 8, 16, 24, 0.3, one, 8), (nul, 8, 0, 8, 0.3, one, 8), (one, 8, 0, 8, 0.3, nul, 8)):
        assert lib.ieee_rerank_stream_range(*bad, *tail) != 0
        assert b"rerank_stream_range" in lib.ieee_last_error()
