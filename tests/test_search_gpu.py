"""GPU: gallery search without the [Q, G] matrix.  TopKAccumulator (ieee_rank_topk_merge) on explicit distance slabs
against the numpy restatement of the whole matrix (tests/util_search.py), and search_topk from descriptors against an
integer oracle and against rank_topk on the same slabs' distances.  Everywhere: indices equal, distances equal as bits."""
import functools

import numpy as np
import pytest
import torch

from tests import util_search as U

pytestmark = pytest.mark.gpu

KS = [1, 10, 100, 1024]


def run(d, parts, k, labels=None, dev=None):
    """merge the column slabs of d (numpy; dev: the same matrix on the device, then device views are added in place)"""
    from ieee_amd.metrics import TopKAccumulator
    acc = TopKAccumulator(d.shape[0], k, *((labels[0], labels[2]) if labels is not None else ()))
    seen = 0
    for lo, hi in U.cuts(d.shape[1], parts):
        assert acc.num_seen == seen == lo
        src = d if dev is None else dev
        if labels is not None:
            acc.add(src[:, lo:hi], labels[1][lo:hi], labels[3][lo:hi])
        else:
            acc.add(src[:, lo:hi])
        seen = hi
    assert acc.num_seen == d.shape[1]
    idx, dist = acc.result()
    assert idx.is_cuda and dist.is_cuda
    return idx, dist


def check(d, parts, k, labels=None, ref=None, dev=None):
    ri, rd = ref if ref is not None else U.ref_topk(d, k, labels)
    idx, dist = run(d, parts, k, labels, dev)
    U.assert_same(idx, dist, ri, rd)
    return idx, dist


PARTITIONS = {
    (3, 7): [[7], [1, 1, 5]],
    (17, 2049): [[2048, 1], [1, 2048], [1000, 1049]],
    (9, 6150): [[2048, 2048, 2054], [4097, 2053]],
    (5, 20000): [3000],
}


@functools.lru_cache(maxsize=None)
def partition_case(shape, k, filt):
    """one matrix per shape, its labels, and the whole-matrix reference: computed once, shared by the partitions"""
    rng = np.random.RandomState(shape[0] * 31 + shape[1])
    d = (rng.rand(*shape) * 100).astype(np.float32)
    labels = U.make_labels(rng, *shape)
    ref = U.ref_topk(d, k, labels if filt else None)
    for a in (d,) + labels + ref:
        a.setflags(write=False)
    return d, (labels if filt else None), ref


@pytest.mark.parametrize("filt", [False, True])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("shape,parts", [(s, p) for s, ps in PARTITIONS.items() for p in ps],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, (tuple, list)) else str(v))
def test_partitions_equal_the_whole_matrix(shape, parts, k, filt):
    d, labels, ref = partition_case(shape, k, filt)
    check(d, parts, k, labels, ref)


@pytest.mark.parametrize("k", KS)
def test_ties_across_slabs_go_to_the_lower_global_index(k):
    rng = np.random.RandomState(k)
    d = rng.randint(0, 6, size=(12, 6000)).astype(np.float32)
    assert all(len(np.unique(r)) < r.size for r in d)
    check(d, 1500, k)
    check(d, 1500, k, U.make_labels(rng, 12, 6000, ids=3, cams=2))


def special_matrix():
    rng = np.random.RandomState(5)
    bits = np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFA00001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000,
                     0x3F800000, 0xBF800000], dtype=np.uint32)        # NaNs of both signs and other payloads, +-inf, +-0, +-1
    d = rng.choice(bits, size=(16, 4 * 1501)).view(np.float32).copy()
    nan_bits = rng.choice(bits[:4], size=d.shape[1])
    d[0] = nan_bits.view(np.float32)                 # a row of NaN only: index order, every payload kept
    d[1, ::2], d[1, 1::2] = -0.0, 0.0                # -0.0 equals +0.0: index order, every sign kept
    return rng, d


@pytest.mark.parametrize("k", KS)
def test_special_values_keep_their_bits_through_later_merges(k):
    rng, d = special_matrix()
    idx, dist = check(d, 1501, k)                     # four slabs
    got = dist.cpu().numpy().view(np.uint32)
    assert (idx[:2].cpu().numpy() == np.arange(k)).all()    # rows 0, 1: entries 0 ... k-1 of the FIRST slab, as stored
    np.testing.assert_array_equal(got[:2], d[:2, :k].view(np.uint32))
    check(d, 1501, k, U.make_labels(rng, 16, d.shape[1], ids=2, cams=2))


@pytest.mark.parametrize("k", KS)
def test_adversarial_rows(k):
    G, slab = 9000, 2500
    desc = np.tile(np.arange(G, 0, -1, dtype=np.float32), (5, 1))     # every slab replaces the whole list
    idx, _ = check(desc, slab, k)
    assert (idx[:, 0] == G - 1).all()
    check(np.full((5, G), 3.0, dtype=np.float32), slab, k)            # all equal: the first slab's list stays
    # query 0: the first two slabs wholly filtered, kept entries only later; query 1: kept entries only in the first
    # two slabs, the list is carried through wholly filtered slabs; query 2 keeps everything
    rng = np.random.RandomState(1)
    d = rng.rand(3, G).astype(np.float32)
    qp, qc = np.array([7, 8, 9]), np.array([1, 1, 1])
    gp, gc = np.full(G, 8), np.full(G, 1)
    gp[:2 * slab] = 7
    idx, _ = check(d, slab, k, (qp, gp, qc, gc))
    assert (idx[0] >= 2 * slab).all() and ((idx[1] >= 0) & (idx[1] < 2 * slab)).all() and (idx[2] >= 0).all()
    # three kept entries in all, in slabs 2, 3 and 4: padding at the end
    gp = np.full(G, 8)
    gp[[2600, 5100, 8999]] = 5
    idx, dist = check(d, slab, k, (qp, gp, qc, gc))
    few = idx[1][idx[1] >= 0].tolist()
    assert len(few) == min(k, 3) and set(few) <= {2600, 5100, 8999}
    assert (idx[1, 3:] == -1).all() and torch.isinf(dist[1, 3:]).all() and (idx[0] >= 0).all()


@pytest.mark.parametrize("k", [10, 1024])
def test_strided_slab_views_are_read_in_place(k):
    rng = np.random.RandomState(11)
    Q, G, off = 11, 7000, 5
    big = torch.from_numpy((rng.rand(Q, G + 13) * 10).astype(np.float32)).cuda()
    view = big[:, off:off + G]                      # row stride G + 13, first column 20 bytes in: not 16-byte aligned
    assert view.stride(0) == G + 13 and view.data_ptr() % 16 != 0
    host = view.cpu().numpy()
    check(host, [2048, 2500, 2452], k, dev=view)
    check(host, [2048, 2500, 2452], k, U.make_labels(rng, Q, G), dev=view)


@pytest.mark.parametrize("k", KS)
def test_one_slab_is_rank_topk(k):
    from ieee_amd.metrics import rank_topk
    rng = np.random.RandomState(k + 40)
    d = torch.from_numpy(rng.randint(0, 50, size=(13, 5003)).astype(np.float32)).cuda()
    labels = U.make_labels(rng, 13, 5003)
    for lab in (None, labels):
        idx, dist = run(d.cpu().numpy(), [5003], k, lab, dev=d)
        ri, rd = rank_topk(d, k, *(lab or ()))
        assert torch.equal(idx, ri) and torch.equal(dist.view(torch.int32), rd.view(torch.int32))


def test_the_same_sequence_twice_gives_the_same_bits():
    rng, d = special_matrix()
    d[2:] = (rng.rand(14, d.shape[1]) * 3).astype(np.float32).round(1)       # ties among ordinary values too
    labels = U.make_labels(rng, 16, d.shape[1])
    first = run(d, 1000, 100, labels)
    again = run(d, 1000, 100, labels)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1].view(torch.int32), again[1].view(torch.int32))


@pytest.mark.parametrize("k", [10, 1024])
def test_mid_size_every_row(k):
    Q, G = 64, 300000
    gen = torch.Generator(device="cuda").manual_seed(7)
    d = torch.rand(Q, G, device="cuda", generator=gen)
    rng = np.random.RandomState(7)
    labels = U.make_labels(rng, Q, G, ids=50, cams=3)
    host = d.cpu().numpy()
    check(host, 65536, k, labels, dev=d)


def test_argument_errors():
    from ieee_amd import _lib
    from ieee_amd.metrics import TopKAccumulator
    z3, z50 = np.zeros(3), np.zeros(50)
    for bad_k in (0, -1, 1025, 2.5, True):
        with pytest.raises(ValueError):
            TopKAccumulator(3, bad_k)
    for bad in [dict(q_pids=z3), dict(q_camids=z3), dict(q_pids=z3, q_camids=z50), dict(device="cpu")]:
        with pytest.raises(ValueError):
            TopKAccumulator(3, 5, **bad)
    with pytest.raises(ValueError):
        TopKAccumulator(-1, 5)
    d = torch.rand(3, 50, device="cuda")
    plain, filt = TopKAccumulator(3, 5), TopKAccumulator(3, 5, z3, z3)
    for acc, args in [(plain, (d, z50, z50)), (plain, (d, z50)), (filt, (d,)), (filt, (d, z50)), (filt, (d, z50, z3)),
                      (plain, (d[0],)), (plain, (torch.rand(4, 50, device="cuda"),))]:
        with pytest.raises(ValueError):
            acc.add(*args)
        assert acc.num_seen == 0
    # the C entry point refuses every bad argument itself (null pointers: it must not get as far as a launch)
    lib = _lib.load()
    si = torch.full((3, 5), -1, dtype=torch.int32, device="cuda")
    sd = torch.full((3, 5), float("inf"), device="cuda")
    one = (_lib.ptr(si), _lib.ptr(sd))

    def call(ldd=50, num_q=3, slab_g=50, g_base=0, labels=None, filt=0, k=5, state=one, slab=_lib.ptr(d)):
        state = state or (None, None)
        return lib.ieee_rank_topk_merge(slab, ldd, num_q, slab_g, g_base, labels, labels, labels, labels, filt, k,
                                        state[0], state[1], None)
    for bad_k in (0, -1, 1025):
        assert call(k=bad_k, state=None, slab=None) != 0
    assert call(num_q=-1, state=None, slab=None) != 0
    assert call(slab_g=-1, ldd=50, state=None, slab=None) != 0
    assert call(g_base=-1, state=None, slab=None) != 0
    assert call(ldd=49, state=None, slab=None) != 0
    assert call(g_base=2 ** 31 - 3 * 2048 - 50, state=None, slab=None) != 0        # g_base + slab_g = 2^31 - 3 * TOPK_CHUNK
    assert call(g_base=2 ** 40, state=None, slab=None) != 0
    assert call(state=None) != 0 and call(state=(one[0], None)) != 0               # null state, num_q > 0
    assert call(filt=1, labels=None) != 0                                          # filter without labels
    assert call(num_q=0, state=None, slab=None) == 0 and call(slab_g=0, slab=None) == 0   # no-ops
    torch.cuda.synchronize()
    assert plain.num_seen == 0 and (plain.result()[0] == -1).all() and (si == -1).all()


# ---- search_topk from descriptors

@functools.lru_cache(maxsize=None)
def integer_case(dim, filt):
    """integers in [-4, 4]: every product and sum is exact in fp32 in any order, so int64 numpy is the oracle"""
    rng = np.random.RandomState(dim)
    Q, G = 33, 5003
    q = rng.randint(-4, 5, size=(Q, dim)).astype(np.float32)
    g = rng.randint(-4, 5, size=(G, dim)).astype(np.float32)
    labels = U.make_labels(rng, Q, G, ids=12, cams=3) if filt else None
    return q, g, labels, U.ref_topk(U.int_distances(q, g), 100, labels)


@pytest.mark.parametrize("filt", [False, True])
@pytest.mark.parametrize("slab", [2048, 3000, 5003, 10000])
@pytest.mark.parametrize("dim", [72, 70])
def test_search_equals_the_integer_oracle(dim, slab, filt):
    from ieee_amd.metrics import search_topk
    q, g, labels, (ri, rd) = integer_case(dim, filt)
    kw = dict(zip(("q_pids", "g_pids", "q_camids", "g_camids"), labels)) if filt else {}
    qt, gt = torch.from_numpy(q), torch.from_numpy(g)
    edges = [0, 1, 1200, 1200, 3249, 5003]                                # uneven pieces, one of them empty
    pieces = [gt[a:b].cuda() if i % 2 else gt[a:b] for i, (a, b) in enumerate(zip(edges[:-1], edges[1:]))]
    for gallery in (gt.cuda(), gt, pieces, (p for p in pieces)):
        idx, dist = search_topk(qt.cuda(), gallery, 100, slab=slab, **kw)
        U.assert_same(idx, dist, ri, rd)


@pytest.mark.parametrize("metric,precision", [("euclidean", None), ("cosine", None), ("euclidean", "f16x2")])
def test_search_equals_rank_topk_on_the_same_slabs(metric, precision):
    from ieee_amd.metrics import compute_distance_matrix, rank_topk, search_topk
    rng = np.random.RandomState(21)
    Q, G, dim, slab, k = 40, 5003, 200, 2048, 50
    q = torch.from_numpy(rng.randn(Q, dim).astype(np.float32)).cuda()
    g = torch.from_numpy(rng.randn(G, dim).astype(np.float32)).cuda()
    labels = U.make_labels(rng, Q, G)
    dm = torch.cat([compute_distance_matrix(q, g[lo:hi], metric, precision) for lo, hi in U.cuts(G, slab)], 1)
    for lab in (None, labels):
        ri, rd = rank_topk(dm, k, *(lab or ()))
        kw = dict(zip(("q_pids", "g_pids", "q_camids", "g_camids"), lab)) if lab else {}
        idx, dist = search_topk(q, g, k, metric=metric, slab=slab, precision=precision, **kw)
        assert torch.equal(idx, ri) and torch.equal(dist.view(torch.int32), rd.view(torch.int32))
        assert ((idx >= 0) & (idx < G)).all()


def test_search_keeps_one_slab_on_the_device():
    from ieee_amd.metrics import search_topk
    Q, G, dim, slab = 256, 200000, 256, 8192
    gen = torch.Generator().manual_seed(3)
    q = torch.randn(Q, dim, generator=gen).cuda()
    pieces = [torch.randn(n, dim, generator=gen) for n in (50000, 70000, 80000)]       # on the host
    search_topk(q, pieces[:1], 10, slab=slab)                                          # code objects loaded
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    idx, dist = search_topk(q, pieces, 10, slab=slab)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak rise %.1f MB of a %.1f MB matrix" % (rise / 1e6, Q * G * 4 / 1e6))
    assert rise < Q * G * 4 / 4
    assert ((idx >= 0) & (idx < G)).all() and (dist[:, 1:] >= dist[:, :-1]).all()


def test_search_label_overrun_and_shortfall():
    from ieee_amd.metrics import search_topk
    q = torch.rand(3, 16).cuda()
    pieces = [torch.rand(40, 16), torch.rand(30, 16).cuda()]
    z3 = np.zeros(3)
    for n in (69, 71, 40, 0):
        for gallery in (pieces, (p for p in pieces), torch.cat([pieces[0], pieces[1].cpu()])):
            with pytest.raises(ValueError):
                search_topk(q, gallery, 5, q_pids=z3, g_pids=np.zeros(n), q_camids=z3, g_camids=np.zeros(n))
    with pytest.raises(ValueError):
        search_topk(q, pieces, 5, q_pids=z3, g_pids=np.zeros(70), q_camids=z3, g_camids=np.zeros(69))
    idx, _ = search_topk(q, pieces, 5, q_pids=z3 + 1, g_pids=np.zeros(70), q_camids=z3, g_camids=np.zeros(70))
    assert ((idx >= 0) & (idx < 70)).all()
    torch.cuda.synchronize()
