"""DBSCAN without a device: the numpy restatement of the definition (tests/util_cluster.py) against scikit-learn and
against an independent statement of its clauses, three deliberately wrong references that the clauses reject, the
argument checks of ieee_amd.cluster (each before a device is needed), dbscan_layout, and the round count of the
hook-and-shortcut restatement on a permuted chain."""
import inspect
import math

import numpy as np
import pytest
import torch

from tests import util_cluster as uc


def random_symmetric_cases(count=300, seed=1):
    """(D fp32 symmetric [N, N], eps, min_samples): N 1 .. 79, min_samples 1 .. 6, eps a dyadic number or one of the
    matrix's own values (pairs exactly on the threshold) -- either way a float32, so that a float64 compare agrees"""
    rng = np.random.RandomState(seed)
    for case in range(count):
        N = int(rng.randint(1, 80))
        A = rng.rand(N, N).astype(np.float32)
        D = np.minimum(A, A.T)
        np.fill_diagonal(D, 0)
        if case % 3 == 0 and N > 1:
            i, j = rng.choice(N, 2, replace=False)
            eps = float(D[i, j])
        else:
            eps = float(rng.choice([1 / 64., 1 / 32., 1 / 16., 1 / 8., 1 / 4., 1 / 2.]))
        yield D, eps, int(rng.randint(1, 7))


def test_restatement_equals_sklearn():
    pytest.importorskip("sklearn")
    from sklearn.cluster import DBSCAN
    sizes = set()
    for D, eps, ms in random_symmetric_cases():
        labels, core, clusters = uc.dbscan_ref(D, eps, ms)
        m = DBSCAN(eps=eps, min_samples=ms, metric="precomputed").fit(D)
        assert np.array_equal(labels, m.labels_), (D.shape, eps, ms)
        assert np.array_equal(np.nonzero(core)[0], m.core_sample_indices_), (D.shape, eps, ms)
        assert clusters == labels.max() + 1
        sizes.add(D.shape[0])
    assert min(sizes) == 1 and max(sizes) >= 75


def asymmetric_case(seed=5, N=40):
    rng = np.random.RandomState(seed)
    D = rng.rand(N, N).astype(np.float32)
    D[3] = np.nan                                  # a NaN row: reached only through its column
    return D


def test_restatement_passes_the_definitional_check():
    for D, eps, ms in random_symmetric_cases(120, seed=2):
        labels, core, _ = uc.dbscan_ref(D, eps, ms)
        assert uc.check_definition(D, eps, ms, labels, core) == []
    D = asymmetric_case()
    for eps, ms in ((0.05, 3), (0.1, 4), (0.02, 1)):
        labels, core, _ = uc.dbscan_ref(D, eps, ms)
        assert uc.check_definition(D, eps, ms, labels, core) == []


def two_clusters_one_border():
    """1-D points at eps = 2, min_samples = 4: 0 .. 3 sit at 0, 1, 2, 3 and 4 .. 7 at 7, 8, 9, 10 (the outer ends have 3
    neighbours: border points); point 8 at 5 touches core 3 and core 4, one of each cluster, and has 3 neighbours"""
    x = np.array([0, 1, 2, 3, 7, 8, 9, 10, 5], dtype=np.float32)
    return np.abs(x[:, None] - x[None, :]), 2.0, 4


def test_wrong_references_fail_the_definitional_check():
    # self not counted: fewer core points
    D, eps, ms = two_clusters_one_border()
    good = uc.dbscan_ref(D, eps, ms)
    assert uc.check_definition(D, eps, ms, good[0], good[1]) == []
    assert good[0].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0]
    assert good[1].tolist() == [False, True, True, True, True, True, True, False, False]
    wrong = uc.dbscan_ref(D, eps, ms, self_counts=False)
    assert not np.array_equal(wrong[1], good[1])
    assert uc.check_definition(D, eps, ms, wrong[0], wrong[1]) != []
    # the largest number at a border point
    wrong = uc.dbscan_ref(D, eps, ms, border="max")
    assert wrong[0].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1]
    assert any("smaller cluster" in b for b in uc.check_definition(D, eps, ms, wrong[0], wrong[1]))
    # AND instead of OR: on a matrix that is not symmetric the relation loses pairs
    D = asymmetric_case()
    for eps, ms in ((0.05, 3), (0.1, 4)):
        good, wrong = uc.dbscan_ref(D, eps, ms), uc.dbscan_ref(D, eps, ms, closure="and")
        assert uc.check_definition(D, eps, ms, good[0], good[1]) == []
        assert uc.check_definition(D, eps, ms, wrong[0], wrong[1]) != []


def defaults(fn):
    return [(n, p.default) for n, p in inspect.signature(fn).parameters.items()]


def test_signatures_and_export():
    import ieee_amd
    from ieee_amd import cluster
    E = inspect.Parameter.empty
    assert ieee_amd.dbscan is cluster.dbscan and ieee_amd.dbscan_layout is cluster.dbscan_layout
    assert defaults(cluster.dbscan) == [("X", E), ("eps", E), ("min_samples", 4), ("metric", "euclidean"), ("block", None),
                                        ("slab", None), ("precision", None), ("max_edges", None), ("return_info", False)]
    assert defaults(cluster.dbscan_layout) == [("N", E), ("d", E), ("edges", E), ("block", None), ("slab", None),
                                               ("metric", "euclidean")]
    assert "eps ** 2" in cluster.dbscan.__doc__


def test_argument_checks_come_before_the_device(monkeypatch):
    from ieee_amd import _lib, cluster
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("a check came after the device was asked for"))
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a check needed the library"))
    X = torch.zeros(5, 8)
    for kw, msg in ((dict(eps=-1), "eps must be"), (dict(eps=float("nan")), "eps must be"), (dict(eps=float("inf")), "eps must be"),
                    (dict(eps="a"), "eps must be"), (dict(eps=None), "eps must be"), (dict(eps=True), "eps must be"),
                    (dict(min_samples=0), "min_samples must be"), (dict(min_samples=2.5), "min_samples must be"),
                    (dict(min_samples=True), "min_samples must be"), (dict(min_samples="4"), "min_samples must be"),
                    (dict(metric="jaccard"), "metric must be"), (dict(precision="fp8"), "precision"),
                    (dict(block=0), "block must be"), (dict(block=True), "block must be"), (dict(slab=0), "slab must be"),
                    (dict(max_edges=-1), "max_edges must be"), (dict(max_edges=1.5), "max_edges must be")):
        args = dict(eps=1.0)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            cluster.dbscan(X, **args)
    for bad in (torch.zeros(5), torch.zeros(5, 0), np.zeros((5, 8), np.float32), [[0.0]]):
        with pytest.raises(ValueError, match=r"X must be an \[N, d\] tensor"):
            cluster.dbscan(bad, 1.0)
    for bad in (torch.zeros(5, 4), np.zeros((5, 4)), torch.zeros(5), [[0.0]]):
        with pytest.raises(ValueError, match="precomputed"):
            cluster.dbscan(bad, 1.0, metric="precomputed")

    huge = torch.empty(((1 << 31) - 1, 1), device="meta")    # rows nobody holds: the shape is all the check looks at
    with pytest.raises(ValueError, match="beyond the index range"):
        cluster.dbscan(huge, 1.0)
    # with every argument in order the next thing asked for is the device
    monkeypatch.setattr(_lib, "require_gpu", lambda: (_ for _ in ()).throw(_lib.IeeeAmdError("device")))
    for args, kw in (((X, 0), {}), ((X, 1.5), dict(min_samples=3.0, metric="cosine", block=2, slab=3, max_edges=0)),
                     ((np.zeros((4, 4)), 1.0), dict(metric="precomputed")), ((torch.zeros(0, 8), 1.0), {})):
        with pytest.raises(_lib.IeeeAmdError, match="device"):
            cluster.dbscan(*args, **kw)


def test_layout_argument_checks_and_totals():
    from ieee_amd.cluster import BLOCK_ROWS, dbscan_layout
    for args, kw, msg in (((-1, 8, 0), {}, "N must be"), ((5, 0, 0), {}, "d must be"), ((5, 8, -1), {}, "edges must be"),
                          ((5, 8, 2.5), {}, "edges must be"), ((5, 8, 0), dict(metric="x"), "metric must be"),
                          ((5, 8, 0), dict(block=0), "block must be"), ((5, 8, 0), dict(slab=-3), "slab must be"),
                          ((1 << 31, 8, 0), {}, "beyond the index range")):
        with pytest.raises(ValueError, match=msg):
            dbscan_layout(*args, **kw)
    for args, kw in (((100000, 768, 2000000), {}), ((2100, 64, 50000), dict(block=256, slab=512)), ((0, 8, 0), {}),
                     ((1, 1, 0), {}), ((500, 0, 1000), dict(metric="precomputed"))):
        lay = dbscan_layout(*args, **kw)
        assert lay["total"] == sum(v for key, v in lay.items() if key != "total")
        assert all(v % 512 == 0 for v in lay.values())
    lay = dbscan_layout(100000, 768, 2000000)
    assert lay["rows"] == 100000 * 768 * 4 and lay["distances"] == BLOCK_ROWS * 100000 * 4
    assert lay["lists"] == lay["mirror"] == 2000000 * 4
    assert lay["total"] < 100000 ** 2 * 4 // 20            # a twentieth of the N x N matrix is not reached
    # nothing grows like N^2: ten times the points and pairs at the same blocking, at most ten times the bytes
    small, big = dbscan_layout(10000, 64, 200000, slab=4096), dbscan_layout(100000, 64, 2000000, slab=4096)
    assert big["total"] <= 10 * small["total"]
    assert dbscan_layout(90, 8, 0, block=3, slab=7)["distances"] == 512       # 3 x 8 floats, rounded up
    assert "matrix" in dbscan_layout(500, 0, 0, metric="precomputed") and "rows" not in dbscan_layout(500, 0, 0, metric="precomputed")


@pytest.mark.parametrize("N", [600, 10000])
def test_hook_and_shortcut_rounds_on_the_permuted_chain(N):
    pos = uc.permuted_chain(N)
    u, v, core = uc.chain_edges(pos)
    f, rounds = uc.cc_rounds(N, u, v)
    print("N = %d: %d rounds" % (N, rounds))
    assert rounds <= 2 * math.ceil(math.log2(N)) + 2
    root = int(np.nonzero(core)[0][0])
    assert (f[core] == root).all() and (f[~core] == np.nonzero(~core)[0]).all()
    if N == 600:
        # the chain's edges are the dense relation's; the plain minimum-of-neighbours iteration needs hundreds of rounds
        D = np.abs(pos[:, None] - pos[None, :]).astype(np.float32)
        R = uc.relation(D, 1.0)
        du, dv = uc.core_edges(R, R.sum(axis=1) >= 3)
        assert sorted(zip(du.tolist(), dv.tolist())) == sorted(zip(u.tolist(), v.tolist()))
        assert uc.min_neighbour_rounds(N, u, v) > 10 * rounds
        labels, core_ref, clusters = uc.dbscan_ref(D, 1.0, 3)
        assert clusters == 1 and (labels == 0).all() and np.array_equal(core_ref, core)


def test_c_abi_argument_checks():
    """every ieee_cluster_* call refuses bad arguments before any launch (no device is needed to be refused)"""
    import ctypes
    from ieee_amd import _lib
    lib = _lib.load()
    null, one, two = ctypes.c_void_p(0), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)   # never dereferenced

    def refused(status, text):
        assert status == -1 and text in lib.ieee_last_error(), (status, lib.ieee_last_error())

    def count(dist=one, ldd=8, rows=3, cols=8, row0=0, col0=0, N=10, deg=one):
        return lib.ieee_cluster_eps_count(dist, ldd, rows, cols, row0, col0, N, 1.0, deg, null)

    def fill(dist=one, ldd=8, rows=3, cols=8, row0=0, col0=0, N=10, rowptr=one, cursor=one, col=two, cap=5):
        return lib.ieee_cluster_eps_fill(dist, ldd, rows, cols, row0, col0, N, 1.0, rowptr, cursor, col, cap, null)
    for call in (count, fill):
        for kw, msg in ((dict(N=0), b"N 0 out of range"), (dict(N=(1 << 31) - 1), b"out of range"),
                        (dict(row0=8), b"outside the 10 points"), (dict(col0=3), b"outside the 10 points"),
                        (dict(rows=-1), b"outside the 10 points"), (dict(ldd=7), b"row stride 7 below the 8 columns"),
                        (dict(dist=null), b"null pointer")):
            refused(call(**kw), msg)
        assert call(rows=0, dist=null) == 0 and call(cols=0, dist=null) == 0
    refused(count(deg=null), b"null pointer")
    refused(fill(rowptr=null), b"null pointer")
    refused(fill(cursor=null), b"null pointer")
    refused(fill(col=null), b"null pointer")
    refused(fill(cap=-1), b"cap -1")
    refused(lib.ieee_cluster_mirror_count(null, one, 10, one, null), b"null pointer")
    refused(lib.ieee_cluster_mirror_count(one, one, 0, one, null), b"N 0 out of range")
    refused(lib.ieee_cluster_mirror_fill(one, one, 10, null, one, one, 5, null), b"null pointer")
    refused(lib.ieee_cluster_mirror_fill(one, one, 10, one, one, null, 5, null), b"null pointer")
    refused(lib.ieee_cluster_mirror_fill(one, one, 1 << 31, one, one, one, 5, null), b"out of range")
    refused(lib.ieee_cluster_core(one, one, 10, 0, one, one, null), b"min_samples 0")
    refused(lib.ieee_cluster_core(one, null, 10, 1, one, one, null), b"null pointer")
    refused(lib.ieee_cluster_cc_round(one, one, one, one, one, 10, two, two, one, null), b"a round writes a second array")
    refused(lib.ieee_cluster_cc_round(one, one, one, one, one, 10, two, one, null, null), b"null pointer")
    refused(lib.ieee_cluster_cc_round(one, one, one, one, one, -1, two, one, one, null), b"out of range")
    refused(lib.ieee_cluster_roots(one, null, 10, one, null), b"null pointer")
    refused(lib.ieee_cluster_labels(one, one, one, one, one, one, null, 10, one, null), b"null pointer")
    refused(lib.ieee_cluster_labels(one, one, one, one, one, one, one, 0, one, null), b"N 0 out of range")


def test_kernel_data_flow_emulated_on_the_host():
    """lists, mirrored lists, rounds and labels as cluster.hip forms them (util_cluster.emulate_kernels) give the dense
    restatement's result on 300 random matrices: symmetric and not, with NaN rows, every min_samples from 1 to 6"""
    rng = np.random.RandomState(0)
    mirrored_seen = 0
    for case in range(300):
        N = int(rng.randint(1, 60))
        D = rng.rand(N, N).astype(np.float32)
        if case % 2:
            D = np.minimum(D, D.T)
        if case % 5 == 0 and N > 3:
            D[2] = np.nan
        eps, ms = float(rng.choice([0.02, 0.05, 0.1, 0.2])), int(rng.randint(1, 7))
        labels, core, clusters, mirrored, rounds = uc.emulate_kernels(D, eps, ms)
        ref = uc.dbscan_ref(D, eps, ms)
        assert np.array_equal(labels, ref[0]) and np.array_equal(core, ref[1]) and clusters == ref[2], (case, N, eps, ms)
        R = uc.relation(D, eps)
        u, v = uc.core_edges(R, core)
        assert rounds == uc.cc_rounds(N, u, v)[1] <= max(N, 1)
        with np.errstate(invalid="ignore"):
            H = D <= np.float32(eps)
        np.fill_diagonal(H, False)
        assert mirrored == int((H & ~H.T).sum())           # one mirrored entry per one-sided pair
        mirrored_seen += mirrored
    assert mirrored_seen > 100


def test_rounds_never_exceed_the_points():
    """dbscan gives up after N rounds: every graph on up to 5 vertices settles within N, the confirming round included"""
    import itertools
    for N in range(1, 6):
        pairs = list(itertools.combinations(range(N), 2))
        worst = 0
        for mask in range(1 << len(pairs)):
            e = [p for k, p in enumerate(pairs) if mask >> k & 1]
            u = np.array([a for a, b in e] + [b for a, b in e], dtype=np.int64)
            v = np.array([b for a, b in e] + [a for a, b in e], dtype=np.int64)
            worst = max(worst, uc.cc_rounds(N, u, v)[1])
        assert worst <= N, (N, worst)
