"""GNN re-ranking on the device (ieee_gnn_rerank, ieee_amd.rerank.gnn_distmat / gnn_reranking, Engine rerank='gnn'):
against the float64 restatement (tests/util_gnn_rerank.py) and the reference's own lists
(tests/golden/gnn_rerank_golden.npz).

Tolerance, per case, from reference-side arithmetic only: err32 = max |sim_fp32 - sim_fp64| of the restatement run in
float32 and in float64, T = 8 * max(err32, 2^-23 * max|sim_fp64|).  A list position is compared only where it is clear
(the float64 similarity differs from both sorted neighbours by more than 2 T), and at least 20 % of the positions of
every k2 != 1 case must be clear.  Each test prints err32, T and the device's error."""
import numpy as np
import pytest
import torch

from tests import util_gnn_rerank as ug

pytestmark = pytest.mark.gpu

CASES = ug.golden_cases()
IDS = [c[0] for c in CASES]


def _reference_side(xq, xg, k1, k2, **kw):
    r64, r32 = ug.restate(xq, xg, k1, k2, torch.float64, **kw), ug.restate(xq, xg, k1, k2, torch.float32, **kw)
    err32, T = ug.tolerance(r32["sim"], r64["sim"])
    return r64, err32, T


def _view(work, offset, rows, cols, dtype):
    return work[offset:offset + rows * cols * 4].view(dtype).reshape(rows, cols)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_distmat_equals_the_float64_restatement(case):
    from ieee_amd.rerank import gnn_distmat
    name, xq, xg, k1, k2, _ = case
    r64, err32, T = _reference_side(xq, xg, k1, k2)
    if k2 != 1:
        clear = ug.clear_positions(r64["sim"], 2 * T).mean()
        assert clear >= 0.2, clear
    dist = gnn_distmat(torch.from_numpy(xq).cuda(), torch.from_numpy(xg).cuda(), k1, k2)
    assert dist.is_cuda and dist.dtype == torch.float32 and dist.shape == (len(xq), len(xg))
    sim = 1.0 - dist.double().cpu()
    if k2 == 1:
        sim = k1 * sim                   # shared-neighbour counts; here err32 is 0 and the floor term of T decides
    err = float((sim - r64["sim"]).abs().max())
    print("%s: err32 %.3g T %.3g device error %.3g" % (name, err32, T, err))
    assert err <= T


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lists_equal_the_reference_at_clear_positions(case):
    from ieee_amd.rerank import gnn_reranking
    name, xq, xg, k1, k2, L = case
    r64, err32, T = _reference_side(xq, xg, k1, k2)
    clear = ug.clear_positions(r64["sim"], 2 * T if k2 != 1 else 0.5)
    if k2 != 1:
        assert clear.mean() >= 0.2
    got = gnn_reranking(torch.from_numpy(xq).cuda(), torch.from_numpy(xg).cuda(), k1, k2)
    assert isinstance(got, np.ndarray) and got.shape == L.shape and np.issubdtype(got.dtype, np.integer)
    print("%s: clear share %.3f, agreement overall %.4f" % (name, clear.mean(), (got == L).mean()))
    assert np.array_equal(got[clear], L[clear])
    assert np.array_equal(np.sort(got, axis=1), np.tile(np.arange(L.shape[1]), (L.shape[0], 1)))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_intermediates_through_the_layout(case):
    from ieee_amd.rerank import _gnn, gnn_layout
    name, xq, xg, k1, k2, _ = case
    Q, G, d = len(xq), len(xg), xq.shape[1]
    N = Q + G
    r64 = ug.restate(xq, xg, k1, k2, torch.float64)
    _, work = _gnn(torch.from_numpy(xq).cuda(), torch.from_numpy(xg).cuda(), k1, k2)
    lay = gnn_layout(Q, G, d, k1, k2)
    rank = _view(work, lay["rank"], N, k1, torch.int32).cpu().long()
    score = -_view(work, lay["S"], N, k1, torch.float32).cpu().double()       # the layout keeps -S, not squared
    for lo, hi in ((0, k2), (k2, k1)):      # no ties across k2 | k2+1 and k1 | k1+1: compare as sets inside
        assert torch.equal(torch.sort(rank[:, lo:hi], dim=1)[0], torch.sort(r64["rank"][:, lo:hi], dim=1)[0])
        assert torch.equal(score[:, lo:hi], r64["S"][:, lo:hi])
    want = torch.gather(torch.cat([torch.from_numpy(xq), torch.from_numpy(xg)]).double() @
                        torch.cat([torch.from_numpy(xq), torch.from_numpy(xg)]).double().t(), 1, rank)
    assert torch.equal(score, want)
    if k2 == 1:
        ld = lay["ld"]
        rows = _view(work, lay["rows"], N, ld, torch.float32).cpu()
        assert lay["rows"] == lay["M0"]
        assert torch.equal(rows[:, :N].double(), r64["rows"]) and not rows[:, N:].any()
        assert torch.equal(rows.sum(1), torch.full((N,), float(k1)))


@pytest.mark.parametrize("Q,G,d,ids,normalise", [(333, 2001, 2304, 80, True), (64, 515, 100, 20, False)])
def test_real_valued_descriptors(Q, G, d, ids, normalise):
    """N not a multiple of 8, d padded.  The device's own rank and S feed the restatement, so a near-tie of two fp32
    scores cannot fail the test; rank itself is checked against a stable sort of the device's own score matrix."""
    from ieee_amd.metrics.distance import _distmat
    from ieee_amd.rerank import _gnn, gnn_layout
    k1, k2 = 26, 7
    xq, xg, _, _ = ug.clustered_features(Q + G, Q, G, d, ids)
    if normalise:
        xq, xg = torch.nn.functional.normalize(xq, p=2, dim=1), torch.nn.functional.normalize(xg, p=2, dim=1)
    N = Q + G
    dist, work = _gnn(xq.cuda(), xg.cuda(), k1, k2)
    lay = gnn_layout(Q, G, (d + 7) // 8 * 8, k1, k2)
    assert lay["ld"] == (N + 7) // 8 * 8
    rank = _view(work, lay["rank"], N, k1, torch.int32).long()
    negs = _view(work, lay["S"], N, k1, torch.float32)
    xu = torch.cat([xq, xg]).cuda()
    neg_score = _distmat(xu, xu, 2)                     # the same GEMM and epilogue, in one call
    order = torch.sort(neg_score, dim=1, stable=True)[1][:, :k1]
    assert torch.equal(rank, order)
    assert torch.equal(negs, torch.gather(neg_score, 1, order))
    kw = dict(rank=rank.cpu(), S=-negs.cpu())
    r64, err32, T = _reference_side(xq, xg, k1, k2, **kw)
    err = float(((1.0 - dist.double().cpu()) - r64["sim"]).abs().max())
    print("(%d, %d, %d): err32 %.3g T %.3g device error %.3g" % (Q, G, d, err32, T, err))
    assert err <= T


def test_two_calls_return_the_same_bits():
    from ieee_amd.rerank import gnn_distmat
    xq, xg, _, _ = ug.clustered_features(5, 150, 1100, 64, 40)
    xq, xg = xq.cuda(), xg.cuda()
    first = gnn_distmat(xq, xg, 26, 7)
    for _ in range(3):
        assert torch.equal(gnn_distmat(xq, xg, 26, 7), first)
    assert torch.equal(gnn_distmat(xq, xg, 12, 1), gnn_distmat(xq, xg, 12, 1))


def test_input_kinds():
    from ieee_amd.rerank import gnn_distmat, gnn_reranking
    xq, xg, _, _ = ug.clustered_features(6, 40, 260, 20, 15)
    L = gnn_reranking(xq.cuda(), xg.cuda(), 10, 3)
    assert np.array_equal(gnn_reranking(xq, xg, 10, 3), L)
    assert np.array_equal(gnn_reranking(xq.numpy(), xg.numpy(), 10, 3), L)
    on_device = gnn_distmat(xq.cuda(), xg.cuda(), 10, 3)
    assert isinstance(on_device, torch.Tensor) and on_device.is_cuda
    on_host = gnn_distmat(xq.numpy(), xg.numpy(), 10, 3)
    assert isinstance(on_host, np.ndarray) and np.array_equal(on_host, on_device.cpu().numpy())
    assert np.array_equal(np.argsort(on_host, axis=1, kind="stable"), L)
    with pytest.raises(ValueError, match="precision"):
        gnn_distmat(xq, xg, 10, 3, precision="fp8")


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
def test_split_precisions_stay_close(precision):
    """the split schemes are fp32-grade GEMMs (2^-24 / 2^-22 relative): same rule, the device's own rank and S"""
    from ieee_amd.rerank import _gnn, gnn_layout
    Q, G, d, k1, k2 = 90, 700, 64, 26, 7
    xq, xg, _, _ = ug.clustered_features(9, Q, G, d, 30)
    xq, xg = torch.nn.functional.normalize(xq, p=2, dim=1), torch.nn.functional.normalize(xg, p=2, dim=1)
    dist, work = _gnn(xq.cuda(), xg.cuda(), k1, k2, precision)
    lay = gnn_layout(Q, G, d, k1, k2, precision)
    N = Q + G
    kw = dict(rank=_view(work, lay["rank"], N, k1, torch.int32).long().cpu(),
              S=-_view(work, lay["S"], N, k1, torch.float32).cpu())
    r64, err32, T = _reference_side(xq, xg, k1, k2, **kw)
    err = float(((1.0 - dist.double().cpu()) - r64["sim"]).abs().max())
    print("%s: err32 %.3g T %.3g device error %.3g" % (precision, err32, T, err))
    assert err <= (T if precision == "bf16x3" else 4 * T)     # f16x2 carries 22 of the 24 mantissa bits


def test_engine_rerank_gnn(capsys):
    from ieee_amd.engine import MultiModalImageSoftmaxEngine
    from ieee_amd.metrics import compute_distance_matrix, evaluate_rank
    from ieee_amd.models import build_model
    from ieee_amd.optim import build_optimizer
    from ieee_amd.rerank import gnn_distmat, re_ranking
    Q, G = 200, 3000
    qf, gf, q_pids, g_pids = ug.clustered_features(0, Q, G, 32, 150)
    qf, gf = qf.cuda(), gf.cuda()
    q_cam, g_cam = np.zeros(Q, dtype=np.int64), np.ones(G, dtype=np.int64)
    labels = {"query": (qf, q_pids, q_cam), "gallery": (gf, g_pids, g_cam)}

    class DM(object):
        num_train_pids = 10
        train_loader = []
        test_loader = {"synthetic": {"query": "query", "gallery": "gallery"}}
        sources = ["synthetic"]
    m = build_model("ieee3modalPart", num_classes=10, loss="softmax", pretrained=False, compute_dtype=torch.float32)
    eng = MultiModalImageSoftmaxEngine(DM(), m, build_optimizer(m, optim="sgd", lr=1e-3), use_gpu=True)
    eng._descriptors = lambda loader, clock: labels[loader]

    mAP_gnn = eng.test(rerank='gnn', ranks=[1, 5])
    out = capsys.readouterr().out
    assert "Applying person re-ranking ... (gnn)" in out and "mAP:" in out and "Rank-1" in out
    norm = torch.nn.functional.normalize
    _, direct = evaluate_rank(gnn_distmat(norm(qf, p=2, dim=1), norm(gf, p=2, dim=1)), q_pids, g_pids, q_cam, g_cam)
    assert mAP_gnn == direct
    # dist_metric does not reach the GNN step; the two keywords do
    assert eng.test(rerank='gnn', ranks=[1], dist_metric='cosine') == direct
    _, other = evaluate_rank(gnn_distmat(norm(qf, p=2, dim=1), norm(gf, p=2, dim=1), 12, 3), q_pids, g_pids, q_cam, g_cam)
    assert eng.test(rerank='gnn', ranks=[1], rerank_k1=12, rerank_k2=3) == other
    capsys.readouterr()

    mAP_plain = eng.test(rerank=False, ranks=[1, 5])
    assert "re-ranking" not in capsys.readouterr().out
    print("mAP: gnn %.4f, plain %.4f" % (mAP_gnn, mAP_plain))
    assert mAP_gnn > mAP_plain

    mAP_kr = eng.test(rerank=True, ranks=[1, 5], rerank_k1=3, rerank_k2=2)       # the k-reciprocal branch ignores them
    out = capsys.readouterr().out
    assert "Applying person re-ranking ...\n" in out and "(gnn)" not in out
    dm = lambda a, b: compute_distance_matrix(a, b, 'euclidean')
    _, want = evaluate_rank(re_ranking(dm(qf, gf), dm(qf, qf), dm(gf, gf)), q_pids, g_pids, q_cam, g_cam)
    assert mAP_kr == want
    with pytest.raises(ValueError, match="rerank"):
        eng.test(rerank='bogus')


def test_memory_guard(monkeypatch):
    """N = 40 000 needs two 6.4 GB matrices: with 1 GB reported free the call raises before it allocates"""
    from ieee_amd.rerank import gnn_distmat
    xq, xg = torch.zeros(1000, 8, device="cuda"), torch.zeros(39000, 8, device="cuda")
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (10 ** 9, 288 * 10 ** 9))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with pytest.raises(RuntimeError, match=r"N = Q \+ G = 40000 .*\b\d{11} bytes.*\b1000000000 bytes free"):
        gnn_distmat(xq, xg)
    assert torch.cuda.max_memory_allocated() - before < (64 << 20)


@pytest.mark.parametrize("Q,G,d,k1,k2", [(333, 1201, 64, 26, 7), (64, 200, 24, 8, 1)])
def test_separate_query_and_gallery_arrays_give_the_same_bits(Q, G, d, k1, k2):
    """gnn_distmat hands the library one array (the scores are then one GEMM); a caller of the C ABI with two arrays
    gets the four-block form, here with Q not a multiple of 4 (score blocks that start off a 16-byte boundary)"""
    from ieee_amd import _lib
    from ieee_amd.rerank import gnn_distmat
    xq, xg, _, _ = ug.clustered_features(Q, Q, G, d, 30)
    buf = torch.empty(Q * d + 8 + G * d, dtype=torch.float32, device="cuda")     # a gap: the two arrays never join up
    xq, xg = buf[:Q * d].view(Q, d).copy_(xq), buf[Q * d + 8:].view(G, d).copy_(xg)
    lib = _lib.require_gpu()
    nbytes = int(lib.ieee_gnn_rerank_workspace_bytes(Q, G, d, k1, k2, 0))
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.empty((Q, G), dtype=torch.float32, device="cuda")
    assert xg.data_ptr() != xq.data_ptr() + Q * d * 4
    _lib.check(lib.ieee_gnn_rerank(_lib.ptr(xq), _lib.ptr(xg), Q, G, d, k1, k2, 0, _lib.ptr(out), _lib.ptr(work), nbytes,
                                   _lib.stream()))
    assert torch.equal(out, gnn_distmat(xq, xg, k1, k2))
