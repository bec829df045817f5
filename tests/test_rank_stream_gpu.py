"""GPU: CMC / mAP without the [Q, G] matrix.  RankAccumulator (ieee_rank_stream_*) fed explicit slabs of a matrix against
the whole-matrix evaluator on the device (ieee_rank_market1501_ws: CMC counts, number of valid queries and every first
position equal; AP equal as bits for a query with at most 1024 true matches, within nb * 2^-52 beyond) and, where the
distances have no ties, against the oracle; evaluate_rank_streamed from descriptors against
evaluate_rank(compute_distance_matrix(...)); the engine's stream_eval against its matrix path."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import util_search as U

pytestmark = pytest.mark.gpu

CAP = 1024          # RANK_CAP of ieee_amd/csrc/rank_common.h
EPS = 2.0 ** -52


def whole(d, labels, max_rank):
    """ieee_rank_market1501_ws on the whole matrix (numpy or device) -> counts, num_valid, AP sum, ap[], first[]"""
    from ieee_amd import _lib as L
    lib = L.require_gpu()
    d = d if isinstance(d, torch.Tensor) else torch.from_numpy(np.array(d, dtype=np.float32)).cuda()
    nq, ng = d.shape
    qp, gp, qc, gc = (torch.from_numpy(np.asarray(x).astype(np.int32)).cuda() for x in labels)
    max_rank = min(max_rank, ng)
    ap = torch.empty(nq, dtype=torch.float64, device="cuda")
    first = torch.empty(nq, dtype=torch.int32, device="cuda")
    summ = torch.empty(max_rank + 2, dtype=torch.int64, device="cuda")
    work = torch.empty(lib.ieee_rank_workspace_bytes(ng), dtype=torch.uint8, device="cuda")
    L.check(lib.ieee_rank_market1501_ws(L.ptr(d), d.stride(0), nq, ng, L.ptr(qp), L.ptr(gp), L.ptr(qc), L.ptr(gc), max_rank,
                                        L.ptr(ap), L.ptr(first), L.ptr(summ), L.ptr(work), work.numel(), L.stream()))
    s = summ.cpu().numpy()
    return dict(counts=s[:max_rank].copy(), nv=int(s[max_rank]), ap_sum=s[max_rank + 1:].view(np.float64)[0],
                ap=ap.cpu().numpy(), first=first.cpu().numpy())


def odd_stride(x):
    """the matrix as a device view whose row stride is 1 mod 4: most rows are not 16-byte aligned"""
    x = torch.from_numpy(np.array(x, dtype=np.float32)).cuda() if not isinstance(x, torch.Tensor) else x
    n = x.shape[1]
    wide = torch.full((x.shape[0], n + ((1 - n) % 4 or 4)), float("nan"), dtype=torch.float32, device="cuda")
    assert wide.stride(0) % 4 == 1
    wide[:, :n] = x
    return wide[:, :n]


def streamed(d, labels, parts, max_rank=20, order=None, device_views=False, chunk=1000):
    """both passes over explicit slabs of d (numpy): contiguous numpy slabs, or views of an odd-stride device matrix"""
    from ieee_amd.metrics import RankAccumulator
    qp, gp, qc, gc = labels
    acc = RankAccumulator(qp, qc, gp, gc, max_rank)
    mc = acc.match_columns
    gathered = np.ascontiguousarray(d[:, mc])
    src1, src2 = (odd_stride(gathered), odd_stride(d)) if device_views else (gathered, d)
    for lo, hi in U.cuts(mc.size, chunk):
        assert acc.num_collected == lo
        acc.collect(src1[:, lo:hi] if device_views else np.ascontiguousarray(src1[:, lo:hi]))
    assert acc.num_collected == mc.size
    acc.seal()
    cuts = U.cuts(d.shape[1], parts)
    for i in (range(len(cuts)) if order is None else order):
        lo, hi = cuts[i]
        acc.count(src2[:, lo:hi] if device_views else np.ascontiguousarray(src2[:, lo:hi]), lo)
    assert acc.num_counted == d.shape[1]
    return acc


def compare(acc, ref):
    """the contract of include/ieee_amd.h (ieee_rank_stream_*) against the whole-matrix result `ref`"""
    counts, nv, ap_sum = acc.result()
    ap, first = acc.per_query()
    assert ap.is_cuda and first.is_cuda and ap.dtype == torch.float64 and first.dtype == torch.int32
    ap, first = ap.cpu().numpy(), first.cpu().numpy()
    assert counts.dtype == np.int64
    np.testing.assert_array_equal(counts, ref["counts"])
    assert nv == ref["nv"]
    np.testing.assert_array_equal(first, ref["first"])
    nb = np.diff(acc.plan.m_off)
    assert ((first < 0) == (nb == 0)).all() and (ap[nb == 0] == -1.0).all()
    small = nb <= CAP                         # summed in the fast kernel's association by both sides: equal as bits
    np.testing.assert_array_equal(ap[small].view(np.int64), ref["ap"][small].view(np.int64))
    err = np.abs(ap - ref["ap"])
    print("AP beyond %d matches: nb %s, |difference| %s (bound nb * 2^-52)" % (CAP, nb[~small], err[~small]))
    assert (err[~small] <= nb[~small] * EPS).all()
    if small.all():
        assert np.float64(ap_sum).view(np.int64) == np.float64(ref["ap_sum"]).view(np.int64)
    else:       # the APs' own bounds, and nv additions of numbers <= 1 on either side
        assert abs(ap_sum - ref["ap_sum"]) <= (nb[~small] * EPS).sum() + nv * nv * EPS
    return ap, first


def against_oracle(acc, d, labels, max_rank=20):
    """no ties in d: the oracle's order is the evaluator's"""
    from oracle import evaluator as ev
    from ieee_amd.metrics.rank import finish_counts
    cmc_o, map_o, ap_o = ev.rank_market1501_c(d, *labels, max_rank, return_all_ap=True)
    cmc, m_ap = finish_counts(*acc.result())
    assert np.array_equal(cmc, cmc_o)
    ap, first = (x.cpu().numpy() for x in acc.per_query())
    nb = np.diff(acc.plan.m_off)
    valid = first >= 0
    assert (np.abs(ap - ap_o)[valid] <= nb[valid] * EPS).all()      # nb terms in (0, 1] summed in two orders
    assert abs(m_ap - map_o) <= nb.max() * EPS + valid.sum() * EPS


PARTITIONS = {
    (3, 7): [[7], [1, 1, 5]],
    (17, 2049): [[2048, 1], [1, 2048], [1000, 1049]],
    (9, 6150): [[2048, 2048, 2054], [4097, 2053]],
    (5, 20000): [[20000], [8200, 11800]],          # slabs of 8192 columns and more: the 16-byte loads of the row stream
}


@functools.lru_cache(maxsize=None)
def partition_case(shape):
    """one matrix per shape (no ties), its labels and the whole-matrix result: computed once, shared by the partitions"""
    rng = np.random.RandomState(shape[0] * 31 + shape[1])
    d = rng.permutation(shape[0] * shape[1]).reshape(shape).astype(np.float32) / 8.0     # exact in fp32, all distinct
    labels = U.make_labels(rng, *shape, ids=max(2, min(20, shape[1] // 3)), cams=3)
    ref = whole(d, labels, 20)
    for a in (d,) + labels:
        a.setflags(write=False)
    return d, labels, ref


@pytest.mark.parametrize("device_views", [False, True], ids=["numpy", "odd-stride-views"])
@pytest.mark.parametrize("shuffled", [False, True], ids=["ascending", "shuffled"])
@pytest.mark.parametrize("shape,parts", [(s, p) for s, ps in PARTITIONS.items() for p in ps],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, (tuple, list)) else str(v))
def test_partitions_equal_the_whole_matrix(shape, parts, shuffled, device_views):
    d, labels, ref = partition_case(shape)
    order = list(np.random.RandomState(len(parts)).permutation(len(parts))[::-1]) if shuffled else None
    acc = streamed(d, labels, parts, order=order, device_views=device_views, chunk=max(1, shape[1] // 3))
    compare(acc, ref)
    against_oracle(acc, d, labels)


@pytest.mark.parametrize("nr", [0, 1025])
@pytest.mark.parametrize("nm", [1023, 1024, 1025, 2500])
def test_the_1024_boundary(nm, nr):
    """query 0: one identity with nm true matches and nr removed entries; the AP's bits up to 1024 matches (whichever
    whole-matrix kernel served the query: up to 1024 matches both sum in one association), nb * 2^-52 beyond"""
    G = 6000
    rng = np.random.RandomState(nm + nr)
    d = rng.permutation(4 * G).reshape(4, G).astype(np.float32)
    where = rng.permutation(G)
    gp, gc = rng.randint(1, 6, G), rng.randint(0, 3, G)
    gp[where[:nm + nr]] = 0
    gc[where[:nm]] = 1 + rng.randint(0, 2, nm)
    gc[where[nm:nm + nr]] = 0
    labels = (np.array([0, 1, 2, 3]), gp, np.array([0, 1, 2, 0]), gc)
    acc = streamed(d, labels, 1500)
    assert np.diff(acc.plan.m_off)[0] == nm and np.diff(acc.plan.r_off)[0] == nr
    ref = whole(d, labels, 20)
    compare(acc, ref)
    against_oracle(acc, d, labels)
    compare(streamed(d, labels, 1500, order=[3, 1, 0, 2], device_views=True), ref)


def test_ties_across_slabs():
    rng = np.random.RandomState(4)
    d = rng.randint(0, 6, size=(12, 6000)).astype(np.float32)
    for ids, cams in ((3, 2), (40, 3)):           # ~1000 and ~100 matches a query: both kinds of query
        labels = U.make_labels(rng, 12, 6000, ids=ids, cams=cams)
        ref = whole(d, labels, 20)
        compare(streamed(d, labels, 1500), ref)
        compare(streamed(d, labels, 1500, order=[2, 0, 3, 1], device_views=True), ref)


def test_special_values_keep_the_raw_order():
    """+-0.0, +-inf, NaNs of both signs and several payloads: the evaluator's order is the raw IEEE order, and the
    streamed evaluation returns what it returns"""
    from tests.test_search_gpu import special_matrix
    rng, d = special_matrix()
    for ids, cams in ((2, 2), (40, 2), (700, 2)):         # ~1500, ~75 and ~4 matches a query
        labels = U.make_labels(rng, 16, d.shape[1], ids=ids, cams=cams)
        ref = whole(d, labels, 20)
        compare(streamed(d, labels, 1501), ref)
        compare(streamed(d, labels, 1501, order=[3, 2, 1, 0], device_views=True), ref)
    # signed zeros on one row, two matches: -0.0 at a higher index goes before +0.0 at a lower one
    row = np.zeros((1, 10), dtype=np.float32)
    row[0, 7] = -0.0
    row[0, 2] = 1.0
    labels = (np.array([1]), np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0]), np.array([0]), np.ones(10, dtype=np.int64))
    ap, first = compare(streamed(row, labels, [4, 6]), whole(row, labels, 20))
    assert first[0] == 0          # the -0.0 match (index 7) is first, before every +0.0


@pytest.mark.parametrize("max_rank", [1, 20, 50, 1024])
def test_placement_and_max_rank(max_rank):
    G, slab = 4500, 1500
    rng = np.random.RandomState(max_rank)
    d = rng.permutation(5 * G).reshape(5, G).astype(np.float32)
    gp, gc = np.full(G, 9), np.zeros(G, dtype=np.int64)
    gp[2 * slab + 5:2 * slab + 40] = 1           # query 0: every match in the last slab
    gp[3:30] = 2                                 # query 1: every match in the first
    gp[slab - 2:slab + 2] = 3                    # query 2: matches on both sides of a cut
    gp[2000:2010] = 4                            # query 3: its identity on its own camera only: no kept match
    qp, qc = np.array([1, 2, 3, 4, 77]), np.array([1, 1, 1, 0, 0])      # query 4: an identity the gallery lacks
    labels = (qp, gp, qc, gc)
    ref = whole(d, labels, max_rank)
    for order in (None, [2, 0, 1]):
        acc = streamed(d, labels, slab, max_rank=max_rank, order=order)
        ap, first = compare(acc, ref)
        assert (first[3:] == -1).all() and (ap[3:] == -1.0).all() and (first[:3] >= 0).all()
        assert acc.result()[1] == 3 and acc.result()[0].shape == (max_rank,)
    against_oracle(acc, d, labels, max_rank)


def test_a_gallery_smaller_than_max_rank(capsys):
    from ieee_amd.metrics import compute_distance_matrix, evaluate_rank, evaluate_rank_streamed
    rng = np.random.RandomState(0)
    d = rng.permutation(3 * 7).reshape(3, 7).astype(np.float32)
    labels = (np.array([0, 1, 2]), np.array([0, 1, 2, 0, 1, 2, 0]), np.zeros(3, dtype=np.int64), np.ones(7, dtype=np.int64))
    acc = streamed(d, labels, [3, 4], max_rank=20)
    assert acc.max_rank == 7 and acc.result()[0].shape == (7,)
    compare(acc, whole(d, labels, 20))
    q, g = torch.from_numpy(rng.randint(0, 4, (3, 8)).astype(np.float32)), torch.from_numpy(rng.randint(0, 4, (7, 8)).astype(np.float32))
    capsys.readouterr()
    cmc_s, map_s = evaluate_rank_streamed(q, g, labels[0], labels[1], labels[2], labels[3])
    said = capsys.readouterr().out
    cmc, m_ap = evaluate_rank(compute_distance_matrix(q.cuda(), g.cuda()), *labels)
    assert said == capsys.readouterr().out == 'Note: number of gallery samples is quite small, got 7\n'
    assert cmc_s.shape == (7,) and cmc_s.dtype == np.float32 and np.array_equal(cmc_s, cmc) and map_s == m_ap


def test_two_runs_give_the_same_bits():
    d, labels, _ = partition_case((9, 6150))
    runs = [streamed(d, labels, [2048, 2048, 2054], order=o) for o in (None, None, [1, 2, 0])]
    aps = [r.per_query()[0].cpu().numpy().view(np.int64) for r in runs]
    sums = [np.float64(r.result()[2]).view(np.int64) for r in runs]
    assert np.array_equal(aps[0], aps[1]) and np.array_equal(aps[0], aps[2]) and sums[0] == sums[1] == sums[2]
    rng = np.random.RandomState(8)                 # and beyond 1024 matches a query
    big = U.make_labels(rng, 9, 6150, ids=2, cams=3)
    aps = [streamed(d, big, 2048, order=o).per_query()[0].cpu().numpy().view(np.int64) for o in (None, [2, 1, 0, 3])]
    assert np.array_equal(aps[0], aps[1])


def test_abi_argument_checks():
    from ieee_amd import _lib as L
    lib = L.require_gpu()
    assert lib.ieee_rank_stream_workspace_bytes(-1, 0, 0) == -1 and lib.ieee_rank_stream_workspace_bytes(0, 0, 0) > 0
    nbytes = lib.ieee_rank_stream_workspace_bytes(2, 3, 1)
    assert nbytes >= 3 * 8 + 1 * 8 + 3 * 4 + 2 * 8 + 2 * 4
    state = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 2, 3], dtype=torch.int64, device="cuda")
    roff = torch.tensor([0, 0, 1], dtype=torch.int64, device="cuda")
    slab = torch.zeros(2, 8, device="cuda")
    summ = torch.zeros(22, dtype=torch.int64, device="cuda")
    count = lambda ldd, g, base, st=state, nb=nbytes: lib.ieee_rank_stream_count(
        L.ptr(slab), ldd, 2, g, base, L.ptr(off), L.ptr(roff), 3, 1, L.ptr(st), nb, L.stream())
    assert count(8, 8, -1) != 0 and b"out of range" in lib.ieee_last_error()
    assert count(8, 8, (1 << 31) - 8) != 0
    assert count(4, 8, 0) != 0 and b"ldd" in lib.ieee_last_error()
    assert count(8, 8, 0, nb=nbytes - 1) != 0 and b"needed" in lib.ieee_last_error()
    assert count(8, 8, 0, st=None) != 0
    assert count(8, 0, 5) == 0                                       # an empty slab: a no-op
    finish = lambda r: lib.ieee_rank_stream_finish(2, L.ptr(off), L.ptr(roff), 3, 1, L.ptr(state), nbytes, r, None, None,
                                                   L.ptr(summ), L.stream())
    assert finish(0) != 0 and finish(1025) != 0 and b"max_rank" in lib.ieee_last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- from descriptors
@functools.lru_cache(maxsize=None)
def descriptor_case(dim):
    """integer-grid descriptors: every squared distance is an integer below 2^24, exact in fp32 whatever the order of
    the sums.  90 % of the gallery rows carry identities no query has."""
    Q, G = 33, 5000
    rng = np.random.RandomState(dim)
    q = rng.randint(-3, 4, (Q, dim)).astype(np.float32)
    g = rng.randint(-3, 4, (G, dim)).astype(np.float32)
    qp, qc = np.arange(Q) % 12, rng.randint(0, 3, Q)                 # every one of the 12 identities has a query
    gp, gc = rng.randint(100, 5000, G), rng.randint(0, 3, G)
    known = rng.permutation(G)[:G // 10]
    gp[known] = rng.randint(0, 12, known.size)
    for a in (qp, gp, qc, gc):
        a.setflags(write=False)
    return q, g, (qp, gp, qc, gc), np.sort(known)


@functools.lru_cache(maxsize=None)
def matrix_result(dim, metric, precision):
    from ieee_amd.metrics import compute_distance_matrix, evaluate_rank
    q, g, labels, _ = descriptor_case(dim)
    dm = compute_distance_matrix(torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda(), metric, precision)
    return evaluate_rank(dm, *labels), dm.cpu().numpy()


def gallery_as(g, form):
    t = torch.from_numpy(g)
    if form == "device":
        return t.cuda()
    if form == "host":
        return t
    return [t[:1700].cuda(), t[1700:1700], t[1700:3001], t[3001:].cuda()]      # mixed devices, an empty piece


@pytest.mark.parametrize("form", ["device", "host", "pieces"])
@pytest.mark.parametrize("slab", [2048, 1000])
@pytest.mark.parametrize("dim", [24, 20])
@pytest.mark.parametrize("metric,precision", [("euclidean", "fp32"), ("euclidean", "f16x2"), ("cosine", "fp32"),
                                              ("cosine", "f16x2")])
def test_from_descriptors(metric, precision, dim, slab, form):
    from ieee_amd.metrics import RankAccumulator, evaluate_rank_streamed, rank_counts_streamed
    from ieee_amd.metrics.rank import finish_counts
    q, g, labels, known = descriptor_case(dim)
    (cmc, m_ap), dm = matrix_result(dim, metric, precision)
    acc = RankAccumulator(labels[0], labels[2], labels[1], labels[3])
    assert acc.match_columns.size == known.size == 500 and np.array_equal(acc.match_columns, known)
    cmc_s, map_s = evaluate_rank_streamed(torch.from_numpy(q).cuda(), gallery_as(g, form), *labels, metric=metric,
                                          slab=slab, precision=precision)
    assert cmc_s.dtype == np.float32 and cmc_s.shape == (20,) and isinstance(map_s, float)
    assert np.array_equal(cmc_s, cmc) and map_s == m_ap            # every query has far fewer than 1024 matches
    if slab == 1000 and form == "pieces":
        triple = rank_counts_streamed(torch.from_numpy(q), gallery_as(g, form), *labels, metric=metric, slab=slab,
                                      precision=precision)
        assert finish_counts(*triple)[1] == m_ap and np.array_equal(finish_counts(*triple)[0], cmc)
    if metric == "euclidean" and precision == "fp32":
        from oracle import evaluator as ev
        assert np.array_equal(dm, U.int_distances(q, g))           # the distances are exact ...
        # ... but tie among themselves; the oracle's stable order is the evaluator's on these non-negative values
        cmc_o, map_o = ev.rank_market1501_c(dm, *labels, 20)
        nb = np.diff(acc.plan.m_off)                               # nb terms in (0, 1] summed in two orders, then the mean
        assert np.array_equal(cmc_s, cmc_o) and abs(map_s - map_o) <= nb.max() * EPS + len(nb) * EPS


def test_streamed_evaluation_holds_one_slab():
    """the memory the device holds at the peak is the slab buffer's order, not the matrix's"""
    from ieee_amd.metrics import evaluate_rank_streamed
    q, g, labels, _ = descriptor_case(24)
    qd, gd = torch.from_numpy(q).cuda(), torch.from_numpy(g)
    evaluate_rank_streamed(qd, gd, *labels, slab=512)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    evaluate_rank_streamed(qd, gd, *labels, slab=512)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < 33 * 5000 * 4 // 2


# ---------------------------------------------------------------- the engine
class StreamDM(object):
    num_train_pids = 10
    sources = ["synthetic"]
    train_loader = []
    test_loader = {"synthetic": {"query": "query", "gallery": "gallery"}}
    data_type = "image"
    width, height = 32, 64

    def __init__(self, root, labels):
        from tests.test_visrank_gpu import records
        qp, gp, qc, gc = labels
        mk = lambda side, n: [("%s/%03d_RGB.png" % (side, i),) for i in range(n)]
        self.records = (records(root, mk("q", len(qp)), qp, qc, 4), records(root, mk("g", len(gp)), gp, gc, 5))

    def fetch_test_loaders(self, name):
        assert name == "synthetic"
        return self.records


def test_engine_stream_eval(tmp_path, capsys, monkeypatch):
    from ieee_amd import engine as E
    rng = np.random.RandomState(2)
    Q, G = 12, 300
    labels = U.make_labels(rng, Q, G, ids=6, cams=3)
    qf = torch.from_numpy(rng.randint(-3, 4, (Q, 24)).astype(np.float32)).cuda()
    gf = torch.from_numpy(rng.randint(-3, 4, (G, 24)).astype(np.float32)).cuda()
    fixed = {"query": (qf, labels[0], labels[2]), "gallery": (gf, labels[1], labels[3])}
    eng = E.Engine(StreamDM(tmp_path / "img", labels), use_gpu=True)
    eng._descriptors = lambda loader, clock: fixed[loader]
    report = lambda: [ln for ln in capsys.readouterr().out.splitlines() if not ln.startswith("Speed:")]
    args = dict(dataset_name="synthetic", query_loader="query", gallery_loader="gallery", ranks=[1, 5, 10])
    for metric in ("euclidean", "cosine"):
        plain = eng._evaluate(dist_metric=metric, **args)
        plain_said = report()
        formed = []
        real = E.compute_distance_matrix
        monkeypatch.setattr(E, "compute_distance_matrix", lambda *a, **k: formed.append(a) or real(*a, **k))
        got = eng._evaluate(dist_metric=metric, stream_eval=True, **args)
        monkeypatch.setattr(E, "compute_distance_matrix", real)
        assert formed == [] and got == plain and report() == plain_said
        assert any(ln.startswith("mAP:") for ln in plain_said) and any(ln.startswith("Rank-10") for ln in plain_said)
    # the figures: the same files, by name, and the same ranking inside them
    from ieee_amd import reidtools
    drawn = []
    real_vis = reidtools.visualize_ranked_results
    monkeypatch.setattr(reidtools, "visualize_ranked_results", lambda *a, **k: drawn.append(real_vis(*a, **k)))
    eng._evaluate(visrank=True, visrank_topk=5, save_dir=str(tmp_path / "a"), **args)
    said_a = report()
    eng._evaluate(visrank=True, visrank_topk=5, save_dir=str(tmp_path / "b"), stream_eval=True, **args)
    assert [ln.replace(str(tmp_path / "b"), str(tmp_path / "a")) for ln in report()] == said_a
    names = sorted(os.listdir(str(tmp_path / "a" / "visrank_synthetic")))
    assert names == sorted("%03d_RGB.jpg" % i for i in range(Q))
    assert sorted(os.listdir(str(tmp_path / "b" / "visrank_synthetic"))) == names
    assert len(drawn) == 2 and drawn[0] == drawn[1]
    # through test() and run(): the keyword reaches _evaluate
    assert eng.test(dist_metric="cosine", stream_eval=True, ranks=[1]) == plain[1]
    eng.run(test_only=True, dist_metric="cosine", stream_eval=True, ranks=[1], save_dir=str(tmp_path / "c"))
    assert "mAP: {:.2%}".format(plain[1]) in report()
