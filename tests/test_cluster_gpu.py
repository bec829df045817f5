"""DBSCAN on the device (ieee_amd/cluster.py, ieee_amd/csrc/cluster.hip) against the numpy restatement of
tests/util_cluster.py applied to compute_distance_matrix's matrix read back (or to the given matrix).  Labels, core
flags and the cluster count are integers: they must be equal, there is no tolerance."""
import numpy as np
import pytest
import torch

from tests import util_cluster as uc

pytestmark = pytest.mark.gpu
NAN = float("nan")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def matrix_of(X, metric, precision=None):
    from ieee_amd.metrics import compute_distance_matrix
    return compute_distance_matrix(X, X, metric, precision=precision).cpu().numpy()


def low_value(D, share):
    """one of the matrix's own off-diagonal values, `share` of the way up their order: pairs sit exactly on it"""
    off = np.sort(D[~np.eye(D.shape[0], dtype=bool)])
    off = off[np.isfinite(off)]
    return float(off[int(share * (off.size - 1))])


def run(X, eps, min_samples, metric="euclidean", D=None, **kw):
    """dbscan(...) checked against the restatement on D (by default the metric's matrix of X) -> (labels, info)"""
    from ieee_amd.cluster import dbscan
    labels, info = dbscan(X, eps, min_samples, metric, return_info=True, **kw)
    assert labels.is_cuda and labels.dtype == torch.int64 and info["core"].is_cuda and info["core"].dtype == torch.bool
    if D is None:
        D = X.cpu().numpy() if metric == "precomputed" else matrix_of(X, metric, kw.get("precision"))
    ref_labels, ref_core, ref_clusters = uc.dbscan_ref(D, eps, min_samples)
    got, core = labels.cpu().numpy(), info["core"].cpu().numpy()
    where = np.nonzero(got != ref_labels)[0]
    assert where.size == 0, ("labels differ at", where[:10], got[where[:10]], ref_labels[where[:10]])
    assert np.array_equal(core, ref_core) and info["clusters"] == ref_clusters
    assert all(isinstance(info[key], int) for key in ("clusters", "edges", "mirrored_edges", "rounds"))
    return labels, info


# ---------------------------------------------------------------- shapes and forms
@pytest.mark.parametrize("N", [1, 2])
def test_one_and_two_points(N):
    X = dev(np.array([[0.0, 0, 0], [1, 0, 0]], np.float32)[:N])
    for eps, ms in ((0.5, 1), (0.5, 2), (1.0, 1), (1.0, 2), (1.0, 3)):
        for metric in ("euclidean", "precomputed"):
            inp = dev(matrix_of(X, "euclidean")) if metric == "precomputed" else X
            labels, info = run(inp, eps, ms, metric)
            assert info["edges"] == (2 if N == 2 and eps >= 1 else 0) and info["mirrored_edges"] == 0


_RAGGED = {}


def ragged_fixture():
    if not _RAGGED:
        X = dev(np.random.RandomState(3).randn(257, 5).astype(np.float32))
        _RAGGED.update(X=X, euclidean=matrix_of(X, "euclidean"), cosine=matrix_of(X, "cosine"))
    return _RAGGED


@pytest.mark.parametrize("metric", ["euclidean", "cosine", "precomputed"])
def test_ragged_tails_and_blockings(metric):
    """257 x 5: d is padded, 257 is no multiple of a block, a slab, a 1024-column pass or four columns; as a
    'precomputed' matrix its rows (stride 257) are not 16-byte aligned and go through the scalar loads"""
    fx = ragged_fixture()
    D = fx["euclidean" if metric == "precomputed" else metric]
    X = dev(D) if metric == "precomputed" else fx["X"]
    eps = low_value(D, 0.01)
    results = []
    for block, slab in ((None, None), (100, 64), (7, 2048)):
        labels, info = run(X, eps, 4, metric, D=D, block=block, slab=slab)
        results.append((labels.cpu().numpy(), info["core"].cpu().numpy(), info["clusters"], info["edges"],
                        info["mirrored_edges"], info["rounds"]))
    print("clusters %d, noise %d, core %d, edges %d, mirrored %d" % (results[0][2], (results[0][0] < 0).sum(),
                                                                     results[0][1].sum(), results[0][3], results[0][4]))
    assert results[0][2] >= 1 and (results[0][0] < 0).any() and not results[0][1].all()      # a case with all kinds in it
    for other in results[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(results[0], other))
    if metric == "precomputed":                    # the same matrix in aligned rows: the 16-byte loads find the same lists
        wide = torch.full((257, 260), NAN, device="cuda")
        wide[:, :257] = X
        labels, info = run(wide[:, :257], eps, 4, metric, D=D)
        assert np.array_equal(labels.cpu().numpy(), results[0][0]) and info["edges"] == results[0][3]


_DENSE = {}


def dense_fixture():
    if not _DENSE:
        X = dev(0.01 * np.random.RandomState(4).randn(2100, 8).astype(np.float32))
        _DENSE.update(X=X, D=matrix_of(X, "euclidean"))
    return _DENSE


def test_every_point_within_eps():
    """lists of 2099 entries: longer than a 1024-column pass, a 2048-row block or a wave's stride; one cluster"""
    fx = dense_fixture()
    assert fx["D"].max() < 1.0
    labels, info = run(fx["X"], 1.0, 4, D=fx["D"])
    assert info["clusters"] == 1 and info["edges"] == 2100 * 2099 and info["mirrored_edges"] == 0
    assert int(labels.min()) == int(labels.max()) == 0 and bool(info["core"].all())
    labels, info = run(fx["X"], 1.0, 4, D=fx["D"], block=512, slab=1000)
    assert info["edges"] == 2100 * 2099


def test_max_edges_is_enforced():
    from ieee_amd.cluster import dbscan
    fx = dense_fixture()
    with pytest.raises(ValueError, match=r"mean degree of 2099\.0.*eps is too large for this memory"):
        dbscan(fx["X"], 1.0, 4, max_edges=1000)
    labels = dbscan(fx["X"], 1.0, 4, max_edges=2100 * 2099)
    assert int(labels.max()) == 0


def test_min_samples_one_and_all_noise():
    fx = ragged_fixture()
    D = fx["euclidean"]
    eps = low_value(D, 0.005)
    labels, info = run(fx["X"], eps, 1, D=D)
    assert bool(info["core"].all()) and int(labels.min()) == 0
    sizes = np.bincount(labels.cpu().numpy())
    assert (sizes == 1).any() and (sizes > 1).any()            # isolated points are singleton clusters
    labels, info = run(fx["X"], eps, 258, D=D)
    assert info["clusters"] == 0 and int(labels.max()) == -1 and not bool(info["core"].any())
    labels, info = run(fx["X"], float(D.max()), 257, D=D)      # N itself is reachable: the point counts
    assert info["clusters"] == 1 and bool(info["core"].all())


# ---------------------------------------------------------------- structure
@pytest.mark.parametrize("xs, expect", [
    # clusters {0..3} and {4..7}; point 8 at 5 touches core 3 (cluster 0) and core 4 (cluster 1)
    ([0, 1, 2, 3, 7, 8, 9, 10, 5], [0, 0, 0, 0, 1, 1, 1, 1, 0]),
    # cluster 0 is numbered by point 0, but its core next to the border point 5 is point 8; cluster 1's is point 1
    ([1, 7, 8, 9, 10, 5, 0, 2, 3], [0, 1, 1, 1, 1, 0, 0, 0, 0]),
])
def test_border_point_takes_the_smaller_cluster(xs, expect):
    x = np.array(xs, np.float32)
    X = dev(x[:, None])
    for metric, inp, eps in (("euclidean", X, 4.0), ("precomputed", dev(np.abs(x[:, None] - x[None, :])), 2.0)):
        labels, info = run(inp, eps, 4, metric)
        assert labels.cpu().tolist() == expect and info["clusters"] == 2
        assert not bool(info["core"][xs.index(5)])


def test_permuted_chain_needs_few_rounds():
    pos = uc.permuted_chain(600)
    D = np.abs(pos[:, None] - pos[None, :]).astype(np.float32)
    labels, info = run(dev(D), 1.0, 3, "precomputed", D=D)
    print("rounds", info["rounds"])
    assert info["clusters"] == 1 and int(labels.min()) == int(labels.max()) == 0
    assert int(info["core"].sum()) == 598 and info["edges"] == 2 * 599
    assert info["rounds"] <= 22
    u, v, _ = uc.chain_edges(pos)
    assert info["rounds"] == uc.cc_rounds(600, u, v)[1]        # a round is a function of the round before


# ---------------------------------------------------------------- values
def test_duplicate_rows():
    rng = np.random.RandomState(6)
    base = rng.randn(40, 24).astype(np.float32)
    X = dev(np.concatenate([base, base[:25], base[:10], rng.randn(30, 24).astype(np.float32)]))
    D = matrix_of(X, "euclidean")
    print("duplicates' distances: min %g max %g" % (D[:25, 40:65].diagonal().min(), D[:25, 40:65].diagonal().max()))
    for eps in (0.0, 1e-5):
        for ms in (2, 3):
            run(X, eps, ms, D=D)
    labels, info = run(X, 1e-3, 3, D=D)
    assert info["clusters"] == 10                              # the ten rows that occur three times


def symmetric_matrix(N, seed):
    A = np.random.RandomState(seed).rand(N, N).astype(np.float32)
    D = np.minimum(A, A.T)
    np.fill_diagonal(D, 0)
    return D


def test_nan_row_is_noise_or_its_own_cluster():
    D = symmetric_matrix(90, 7)
    D[3, :] = NAN
    D[:, 3] = NAN
    eps = low_value(D, 0.05)
    labels, info = run(dev(D), eps, 3, "precomputed", D=D)
    assert int(labels[3]) == -1 and info["clusters"] >= 1 and info["mirrored_edges"] == 0
    labels, info = run(dev(D), eps, 1, "precomputed", D=D)
    assert int(labels[3]) >= 0 and int((labels == labels[3]).sum()) == 1
    run(D, eps, 3, "precomputed", D=D)                         # a numpy matrix


def test_one_sided_entry_is_mirrored():
    D = symmetric_matrix(90, 8) + np.float32(1.0)
    np.fill_diagonal(D, 0)
    D[5, 6] = D[6, 5] = D[6, 7] = D[7, 6] = 0.25
    D[5, 40] = 0.25                                            # and D[40, 5] stays above: the OR makes them neighbours
    labels, info = run(dev(D), 0.5, 3, "precomputed", D=D)
    assert info["mirrored_edges"] == 1 and info["edges"] == 5
    assert labels.cpu().tolist()[5:8] == [0, 0, 0] and int(labels[40]) == 0 and info["clusters"] == 1
    assert bool(info["core"][5]) and not bool(info["core"][40])


def test_cosine_with_pairs_on_the_threshold():
    X = dev(np.random.RandomState(9).randn(300, 64).astype(np.float32))
    D = matrix_of(X, "cosine")
    eps = low_value(D, 0.02)
    assert (D == np.float32(eps)).any()
    labels, info = run(X, eps, 4, "cosine", D=D)
    asym = int(((D <= np.float32(eps)) != (D <= np.float32(eps)).T).sum()) // 2
    print("mirrored_edges %d of %d edges; one-sided pairs of the matrix %d" % (info["mirrored_edges"], info["edges"], asym))
    assert info["mirrored_edges"] == asym
    run(X, eps, 4, "cosine", D=D, block=64, slab=100)


def test_bf16x3_precision_and_the_host():
    from ieee_amd.cluster import dbscan
    Xh = torch.from_numpy(np.random.RandomState(10).randn(300, 64).astype(np.float32))
    X = Xh.cuda()
    D = matrix_of(X, "euclidean", "bf16x3")
    eps = low_value(D, 0.02)
    labels, info = run(X, eps, 4, precision="bf16x3", D=D)
    # X on the host gives the result of X on the device; two calls give identical tensors
    for inp in (Xh, X):
        again, info2 = dbscan(inp, eps, 4, precision="bf16x3", return_info=True)
        assert again.is_cuda and torch.equal(again, labels) and torch.equal(info2["core"], info["core"])
        assert {k: v for k, v in info2.items() if k != "core"} == {k: v for k, v in info.items() if k != "core"}
    empty = dbscan(X[:0], eps)
    assert empty.is_cuda and empty.dtype == torch.int64 and tuple(empty.shape) == (0,)


# ---------------------------------------------------------------- memory
@pytest.mark.parametrize("where", ["device", "host"])
def test_memory_stays_within_the_layout(where):
    """The layout's total is an upper bound with two terms that a run may not need: 'rows', the copy of X that is not
    made where X is on the device in operand form already (fp32, contiguous, d a multiple of 8), and 'mirror', counted
    at one entry per pair.  Both are taken out here where the run does without them, so that a second [block, slab]
    distance buffer (524 KB, less than either) would not fit under the bound."""
    from ieee_amd.cluster import dbscan, dbscan_layout
    N, d = 2100, 64
    Xh = torch.from_numpy(np.random.RandomState(11).randn(N, d).astype(np.float32))
    X = Xh.cuda()
    D = matrix_of(X, "cosine")
    eps = low_value(D, 0.01)
    del D
    inp = X if where == "device" else Xh
    labels, info = dbscan(inp, eps, 4, "cosine", block=256, slab=512, return_info=True)
    lay = dbscan_layout(N, d, info["edges"], block=256, slab=512, metric="cosine")
    assert lay["total"] < N * N * 4 // 2
    bound = lay["total"] - lay["mirror"] + (4 * info["mirrored_edges"] + 511) // 512 * 512
    if where == "device":
        bound -= lay["rows"]
    assert lay["distances"] == 256 * 512 * 4
    del labels
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = dbscan(inp, eps, 4, "cosine", block=256, slab=512, return_info=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("%s rows: peak %.3f MB, bound %.3f MB, layout %.3f MB, N x N %.2f MB, %d edges"
          % (where, peak / 1e6, bound / 1e6, lay["total"] / 1e6, N * N * 4 / 1e6, info["edges"]))
    assert out[1]["edges"] == info["edges"]
    assert peak <= bound
    assert peak + lay["distances"] > bound         # a second distance buffer would have been seen
