"""GNN re-ranking on sparse rows (ieee_gnn_sparse_*, ieee_amd.rerank.gnn_distmat / gnn_reranking with
formulation='sparse', gnn_search_topk, Engine rerank_formulation): against the float64 restatement
(tests/util_gnn_rerank.py), the reference's own lists (tests/golden/gnn_rerank_golden.npz) and the dense formulation.

The rule is the dense tests': err32 = max |sim_fp32 - sim_fp64| of the restatement, T = 8 * max(err32, 2^-23 max|sim_fp64|)
(util_gnn_rerank.tolerance); the same rule on the restatement's rows (rows_fp32 against rows_fp64) bounds the final
rows, which are compared normalised, i.e. at the scale the rule is stated for, and a stored norm is compared as
norm / |row|, at that scale too.  Sparse against dense on the device: 2 T.  Where the float64 similarity is exactly 0 the
sparse distance is exactly 1.  Lists are compared at clear positions only.  Each test prints err32, T and its errors."""
import ctypes

import numpy as np
import pytest
import torch

from tests import util_gnn_rerank as ug

pytestmark = pytest.mark.gpu

CASES = ug.golden_cases()
IDS = [c[0] for c in CASES]
normalize = torch.nn.functional.normalize


def _reference_side(xq, xg, k1, k2, **kw):
    r64, r32 = ug.restate(xq, xg, k1, k2, torch.float64, **kw), ug.restate(xq, xg, k1, k2, torch.float32, **kw)
    err32, T = ug.tolerance(r32["sim"], r64["sim"])
    return r64, r32, err32, T


def _view(work, offset, rows, cols, dtype):
    return work[offset:offset + rows * cols * 4].view(dtype).reshape(rows, cols)


def _features(seed, Q, G, d, ids, normalise=True):
    xq, xg, pq, pg = ug.clustered_features(seed, Q, G, d, ids)
    if normalise:
        xq, xg = normalize(xq, p=2, dim=1), normalize(xg, p=2, dim=1)
    return xq, xg, pq, pg


def _dense_rank_and_scores(xq, xg, k1, k2, precision="fp32"):
    from ieee_amd.rerank import _gnn, gnn_layout
    Q, G, d = xq.shape[0], xg.shape[0], (xq.shape[1] + 7) // 8 * 8
    dist, work = _gnn(xq.cuda(), xg.cuda(), k1, k2, precision)
    lay = gnn_layout(Q, G, d, k1, k2, precision)
    return (dist, _view(work, lay["rank"], Q + G, k1, torch.int32).clone(),
            _view(work, lay["S"], Q + G, k1, torch.float32).clone())


def _csr_on_host(st):
    N = st["N"]
    rowptr = st["rowptr"].cpu()
    nnz = int(rowptr[N])
    return rowptr, st["col"].cpu()[:nnz].long(), st["val"].cpu()[:nnz], st["norm"].cpu()


def _check_csr(rowptr, col, N):
    assert rowptr.dtype == torch.int64 and rowptr.shape == (N + 1,) and int(rowptr[0]) == 0
    length = rowptr[1:] - rowptr[:-1]
    assert bool((length >= 0).all())
    assert col.numel() == int(rowptr[N]) and bool((col >= 0).all()) and bool((col < N).all())
    row = torch.repeat_interleave(torch.arange(N), length)
    inside = row[1:] == row[:-1]
    assert bool((col[1:][inside] > col[:-1][inside]).all()), "columns not strictly ascending inside a row"
    return row


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_goldens_values(case):
    """the goldens' final rows are as long as N (in-degrees 460 of 460, 917 of 1000, 295 of 340, 100 of 120)"""
    from ieee_amd.rerank import gnn_distmat
    name, xq, xg, k1, k2, _ = case
    r64, _, err32, T = _reference_side(xq, xg, k1, k2)
    dist = gnn_distmat(torch.from_numpy(xq).cuda(), torch.from_numpy(xg).cuda(), k1, k2, formulation='sparse')
    assert dist.is_cuda and dist.dtype == torch.float32 and dist.shape == (len(xq), len(xg))
    sim = 1.0 - dist.double().cpu()
    if k2 == 1:
        sim = k1 * sim                   # shared-neighbour counts; err32 is 0 and the floor term of T decides
    err = float((sim - r64["sim"]).abs().max())
    print("%s: err32 %.3g T %.3g device error %.3g" % (name, err32, T, err))
    assert err <= T
    zero = r64["sim"] == 0
    assert bool((dist.cpu()[zero] == 1.0).all())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_goldens_lists(case):
    from ieee_amd.rerank import gnn_reranking
    name, xq, xg, k1, k2, L = case
    r64, _, err32, T = _reference_side(xq, xg, k1, k2)
    clear = ug.clear_positions(r64["sim"], 2 * T if k2 != 1 else 0.5)
    if k2 != 1:
        assert clear.mean() >= 0.2
    got = gnn_reranking(torch.from_numpy(xq).cuda(), torch.from_numpy(xg).cuda(), k1, k2, formulation='sparse')
    assert isinstance(got, np.ndarray) and got.shape == L.shape and np.issubdtype(got.dtype, np.integer)
    print("%s: clear share %.3f, agreement overall %.4f" % (name, clear.mean(), (got == L).mean()))
    assert np.array_equal(got[clear], L[clear])
    assert np.array_equal(np.sort(got, axis=1), np.tile(np.arange(L.shape[1]), (L.shape[0], 1)))


@pytest.mark.parametrize("slab_rows", [700, None])
def test_neighbour_lists_equal_the_dense_path_bit_for_bit(slab_rows):
    """N = 2334: slab_rows = 700 is four slabs with a ragged last one"""
    from ieee_amd.rerank import _gnn_sparse
    xq, xg, _, _ = _features(333 + 2001, 333, 2001, 64, 80)
    _, rank, S = _dense_rank_and_scores(xq, xg, 26, 7)
    st = _gnn_sparse(xq.cuda(), xg.cuda(), 26, 7, slab_rows=slab_rows)
    assert st["rank"].dtype == torch.int32 and st["S"].dtype == torch.float32
    assert torch.equal(st["rank"], rank)
    assert torch.equal(st["S"].view(torch.int32), S.view(torch.int32))


@pytest.mark.parametrize("Q,G,d,ids,normalise,k1,k2", [(333, 2001, 2304, 80, True, 26, 7), (64, 515, 100, 20, False, 26, 7),
                                                       (333, 2001, 64, 80, True, 26, 7), (333, 2001, 64, 80, True, 10, 3)])
def test_real_valued_descriptors(Q, G, d, ids, normalise, k1, k2):
    """the device's own rank and S feed the restatement, as in the dense test.  On the d = 64 shape 8.2 % (26, 7) and
    94.9 % (10, 3) of the pairs have similarity exactly 0 (tests/test_gnn_sparse_cpu.py holds both shares away from 0
    and 1), on the d = 2304 shape 53.9 %."""
    from ieee_amd.rerank import _gnn_sparse, _gnn_sparse_distmat
    xq, xg, _, _ = _features(Q + G, Q, G, d, ids, normalise)
    N = Q + G
    st = _gnn_sparse(xq.cuda(), xg.cuda(), k1, k2)
    dist = _gnn_sparse_distmat(xq.cuda(), xg.cuda(), k1, k2)
    dense, rank, S = _dense_rank_and_scores(xq, xg, k1, k2)
    assert torch.equal(st["rank"], rank) and torch.equal(st["S"], S)
    assert bool((S != 0).all())          # then the structural support is the numerical one
    r64, r32, err32, T = _reference_side(xq, xg, k1, k2, rank=rank.cpu().long(), S=-S.cpu())
    err = float(((1.0 - dist.double().cpu()) - r64["sim"]).abs().max())
    # the final rows
    rowptr, col, val, norm = _csr_on_host(st)
    row = _check_csr(rowptr, col, N)
    support = torch.zeros((N, N), dtype=torch.bool)
    support[row, col] = True
    assert torch.equal(support, r64["rows"] != 0)
    rows = torch.zeros((N, N), dtype=torch.float64)
    rows[row, col] = val.double()
    own = rows.norm(p=2, dim=1)
    err_rows32, T_rows = ug.tolerance(r32["rows"], r64["rows"])
    err_rows = float((rows / own.clamp_min(1e-12)[:, None] - r64["rows"]).abs().max())
    err_norm = float((norm.double() / own.clamp_min(1e-300) - 1.0)[own > 0].abs().max())
    assert bool((norm[own == 0] == 0).all())
    gap = float((dist - dense).abs().max())
    zero = r64["sim"] == 0
    print("(%d, %d, %d, %d, %d): err32 %.3g T %.3g device error %.3g; rows: err32 %.3g T %.3g device error %.3g, norm "
          "%.3g; sparse - dense %.3g; exact zeros %.3f; stored %s"
          % (Q, G, d, k1, k2, err32, T, err, err_rows32, T_rows, err_rows, err_norm, gap, float(zero.double().mean()),
             st["entries"]))
    assert err <= T
    assert err_rows <= T_rows
    assert err_norm <= T_rows
    assert gap <= 2 * T
    assert bool((dist.cpu()[zero] == 1.0).all())


def test_same_bits_however_the_work_is_cut():
    from ieee_amd.metrics import rank_topk
    from ieee_amd.rerank import gnn_distmat, gnn_search_topk
    Q, G = 150, 1100
    xq, xg, pq, pg = _features(5, Q, G, 64, 40)
    xq, xg = xq.cuda(), xg.cuda()
    cq, cg = np.arange(Q) % 3, np.arange(G) % 3
    first = gnn_distmat(xq, xg, 26, 7, formulation='sparse')
    for _ in range(2):
        assert torch.equal(gnn_distmat(xq, xg, 26, 7, formulation='sparse'), first)
    for slab_rows in (1, 257):
        assert torch.equal(gnn_distmat(xq, xg, 26, 7, formulation='sparse', slab_rows=slab_rows), first)
    one = gnn_distmat(xq, xg, 12, 1, formulation='sparse')
    assert torch.equal(gnn_distmat(xq, xg, 12, 1, formulation='sparse', slab_rows=257), one)
    labels = dict(q_pids=pq, g_pids=pg, q_camids=cq, g_camids=cg)
    # four identities on one camera: a quarter of the gallery is filtered out of every row, fewer than 1024 are kept
    coarse = dict(q_pids=pq % 4, g_pids=pg % 4, q_camids=0 * cq, g_camids=0 * cg)
    for k, kw in ((10, {}), (10, labels), (1024, coarse)):
        want_i, want_d = rank_topk(first, k, **kw)
        if k == 1024:
            assert bool((want_i == -1).any(dim=1).all()) and bool(torch.isinf(want_d).any(dim=1).all())
        for slab_rows in (1, 257, None):
            got_i, got_d = gnn_search_topk(xq, xg, k, 26, 7, slab_rows=slab_rows, **kw)
            assert got_i.dtype == torch.int64 and got_d.dtype == torch.float32 and got_i.is_cuda
            assert torch.equal(got_i, want_i), (k, slab_rows)
            assert torch.equal(got_d.view(torch.int32), want_d.view(torch.int32)), (k, slab_rows)


def test_memory_stays_below_one_dense_matrix(monkeypatch):
    """N = 12 000: the dense path's two matrices are 576 MB each; the restatement counts 7.5 M stored entries over the
    four stages.  The restatement runs on the device here (float64 and float32, util_gnn_rerank.restate unchanged,
    its factory calls placed there by torch.device) so that the test stays within seconds."""
    from ieee_amd.metrics import rank_topk
    from ieee_amd.rerank import _gnn_sparse, gnn_distmat, gnn_search_topk
    Q, G, k1, k2 = 1000, 11000, 26, 7
    xq, xg, _, _ = _features(12, Q, G, 64, 500)
    xq, xg = xq.cuda(), xg.cuda()
    N = Q + G
    ld = (N + 7) // 8 * 8
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    idx, dist = gnn_search_topk(xq, xg, 10, k1, k2, slab_rows=2048)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak %.1f MB against %.1f MB for one dense matrix" % (peak / 1e6, N * ld * 4 / 1e6))
    assert peak < N * ld * 4
    assert idx.shape == (Q, 10) and dist.shape == (Q, 10)

    sparse = gnn_distmat(xq, xg, k1, k2, formulation='sparse')
    real = torch.cuda.mem_get_info
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (600 * 10 ** 6, 288 * 10 ** 9))
    with pytest.raises(RuntimeError, match=r"N = Q \+ G = 12000 .*\b600000000 bytes free"):
        gnn_distmat(xq, xg, k1, k2)
    auto = gnn_distmat(xq, xg, k1, k2, formulation='auto')
    monkeypatch.setattr(torch.cuda, "mem_get_info", real)
    assert torch.equal(auto, sparse)
    want_i, want_d = rank_topk(sparse, 10)
    assert torch.equal(idx, want_i) and torch.equal(dist.view(torch.int32), want_d.view(torch.int32))

    st = _gnn_sparse(xq, xg, k1, k2)
    print("stored entries per stage %s" % (st["entries"],))
    rows = torch.linspace(0, Q - 1, 64).long()
    with torch.device("cuda"):
        sims = []
        for dtype in (torch.float64, torch.float32):
            r = ug.restate(xq, xg, k1, k2, dtype, rank=st["rank"].long(), S=-st["S"])
            sims.append(r["sim"][rows.cuda()].cpu())
            del r
    err32, T = ug.tolerance(sims[1], sims[0])
    err = float(((1.0 - sparse[rows.cuda()].double().cpu()) - sims[0]).abs().max())
    print("64 rows: err32 %.3g T %.3g device error %.3g" % (err32, T, err))
    assert err <= T


def test_split_precision_stays_close():
    from ieee_amd.rerank import _gnn_sparse, _gnn_sparse_distmat
    Q, G, d, k1, k2 = 90, 700, 64, 26, 7
    xq, xg, _, _ = _features(9, Q, G, d, 30)
    st = _gnn_sparse(xq.cuda(), xg.cuda(), k1, k2, "bf16x3")
    dist = _gnn_sparse_distmat(xq.cuda(), xg.cuda(), k1, k2, "bf16x3")
    _, rank, S = _dense_rank_and_scores(xq, xg, k1, k2, "bf16x3")
    assert torch.equal(st["rank"], rank) and torch.equal(st["S"], S)
    r64, _, err32, T = _reference_side(xq, xg, k1, k2, rank=rank.cpu().long(), S=-S.cpu())
    err = float(((1.0 - dist.double().cpu()) - r64["sim"]).abs().max())
    print("bf16x3: err32 %.3g T %.3g device error %.3g" % (err32, T, err))
    assert err <= T


def test_engine_rerank_formulation(capsys):
    from ieee_amd.engine import MultiModalImageSoftmaxEngine
    from ieee_amd.metrics import evaluate_rank
    from ieee_amd.models import build_model
    from ieee_amd.optim import build_optimizer
    from ieee_amd.rerank import gnn_distmat
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

    mAP_sparse = eng.test(rerank='gnn', rerank_formulation='sparse', ranks=[1, 5])
    assert "Applying person re-ranking ... (gnn)" in capsys.readouterr().out
    direct = gnn_distmat(normalize(qf, p=2, dim=1), normalize(gf, p=2, dim=1), formulation='sparse')
    _, want = evaluate_rank(direct, q_pids, g_pids, q_cam, g_cam)
    assert mAP_sparse == want
    mAP_plain = eng.test(rerank=False, ranks=[1, 5])
    assert eng.test(rerank=False, rerank_formulation='sparse', ranks=[1, 5]) == mAP_plain
    mAP_kr = eng.test(rerank=True, ranks=[1])
    assert eng.test(rerank=True, rerank_formulation='sparse', ranks=[1]) == mAP_kr
    capsys.readouterr()
    print("mAP: gnn sparse %.4f, plain %.4f" % (mAP_sparse, mAP_plain))
    assert mAP_sparse > mAP_plain
    with pytest.raises(ValueError, match="formulation"):
        eng.test(rerank='gnn', rerank_formulation='bogus')


def test_argument_errors_through_the_c_abi():
    from ieee_amd import _lib
    lib = _lib.require_gpu()
    bad = -1                             # IEEE_ERR_BAD_ARG
    assert lib.ieee_gnn_sparse_scratch_bytes(10, 20, 4, 5) == -1 and b"k2 out of range" in lib.ieee_last_error()
    assert lib.ieee_gnn_sparse_scratch_bytes(10, 20, 31, 3) == -1 and b"k1 out of range" in lib.ieee_last_error()
    assert lib.ieee_gnn_sparse_scratch_bytes(10, 20, 1025, 3) == -1 and b"k1 out of range" in lib.ieee_last_error()
    assert lib.ieee_gnn_sparse_scratch_bytes(0, 20, 4, 2) == -1 and b"empty" in lib.ieee_last_error()
    assert lib.ieee_gnn_sparse_scratch_bytes(1 << 30, 20, 4, 2) == -1 and b"2^31" in lib.ieee_last_error()
    N, k1 = 30, 4
    nbytes = int(lib.ieee_gnn_sparse_scratch_bytes(10, 20, k1, 2))
    assert nbytes > 0
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    ptr64 = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    i32 = torch.zeros(N * k1, dtype=torch.int32, device="cuda")
    f32 = torch.zeros(N * k1, dtype=torch.float32, device="cuda")
    p, null, s = _lib.ptr, ctypes.c_void_p(0), _lib.stream()
    calls = {
        "gnn_sparse_propagate_count: k2": lambda: lib.ieee_gnn_sparse_propagate_count(
            p(ptr64), p(i32), p(i32), N, k1, k1 + 1, p(scratch), nbytes, p(ptr64), s),
        "gnn_sparse_propagate_count: k1": lambda: lib.ieee_gnn_sparse_propagate_count(
            p(ptr64), p(i32), p(i32), N, N + 1, 2, p(scratch), nbytes, p(ptr64), s),
        "gnn_sparse_propagate_fill: k2": lambda: lib.ieee_gnn_sparse_propagate_fill(
            p(ptr64), p(i32), p(f32), p(i32), p(f32), N, k1, 0, p(scratch), nbytes, p(ptr64), p(i32), p(f32), p(f32), 1, s),
        "gnn_sparse_propagate_fill: null": lambda: lib.ieee_gnn_sparse_propagate_fill(
            p(ptr64), p(i32), p(f32), p(i32), null, N, k1, 2, p(scratch), nbytes, p(ptr64), p(i32), p(f32), p(f32), 1, s),
        "gnn_sparse_propagate_count: scratch too small": lambda: lib.ieee_gnn_sparse_propagate_count(
            p(ptr64), p(i32), p(i32), N, k1, 2, p(scratch), nbytes - 1, p(ptr64), s),
        "gnn_sparse_symmetrise_count: null": lambda: lib.ieee_gnn_sparse_symmetrise_count(
            p(ptr64), null, p(ptr64), p(i32), N, p(scratch), nbytes, p(ptr64), s),
        "gnn_sparse_symmetrise_fill: null": lambda: lib.ieee_gnn_sparse_symmetrise_fill(
            p(ptr64), p(i32), p(f32), null, p(ptr64), p(i32), p(f32), N, p(scratch), nbytes, p(ptr64), null, p(f32), null, 1, s),
        "gnn_sparse_transpose: null": lambda: lib.ieee_gnn_sparse_transpose(
            p(ptr64), p(i32), p(f32), null, N, 0, N, null, p(ptr64), p(i32), p(f32), 1, s),
        "gnn_sparse_transpose: rows": lambda: lib.ieee_gnn_sparse_transpose(
            p(ptr64), p(i32), p(f32), null, N, 5, N + 1, p(i32), p(ptr64), p(i32), p(f32), 1, s),
        "gnn_sparse_cosine: null": lambda: lib.ieee_gnn_sparse_cosine(
            p(ptr64), p(i32), p(f32), p(f32), p(ptr64), p(i32), p(f32), 10, 20, 0, 20, null, 20, s),
        "gnn_sparse_cosine: range": lambda: lib.ieee_gnn_sparse_cosine(
            p(ptr64), p(i32), p(f32), p(f32), p(ptr64), p(i32), p(f32), 10, 20, 4, 21, p(f32), 20, s),
    }
    for what, call in calls.items():
        assert call() == bad, what
        assert what.split(":")[0].encode() in lib.ieee_last_error(), (what, lib.ieee_last_error())
    torch.cuda.synchronize()
    assert not scratch.any()             # nothing was launched
    from ieee_amd.rerank import gnn_distmat
    x = torch.rand(40, 8, device="cuda")
    with pytest.raises(_lib.IeeeAmdError, match="k2 out of range"):
        gnn_distmat(x[:10], x[10:], 5, 6, formulation='sparse')
    with pytest.raises(_lib.IeeeAmdError, match="k1 out of range"):
        gnn_distmat(x[:10], x[10:], 41, 6, formulation='sparse')


def test_a_range_wider_than_the_lds_accumulator():
    """ranges up to 16 384 columns accumulate in LDS, wider ones in the output row: G = 17 000 in one range against
    ranges of 4 096 (equal bits) and against the dense formulation (2 T)"""
    from ieee_amd.rerank import _gnn_sparse, gnn_distmat
    Q, G, k1, k2 = 8, 17000, 6, 3
    xq, xg, _, _ = _features(3, Q, G, 16, 600)
    xq, xg = xq.cuda(), xg.cuda()
    wide = gnn_distmat(xq, xg, k1, k2, formulation='sparse', slab_rows=G)
    assert torch.equal(wide, gnn_distmat(xq, xg, k1, k2, formulation='sparse', slab_rows=4096))
    st = _gnn_sparse(xq, xg, k1, k2)
    with torch.device("cuda"):
        kw = dict(rank=st["rank"].long(), S=-st["S"])
        sim64, sim32 = (ug.restate(xq, xg, k1, k2, dtype, **kw)["sim"].cpu() for dtype in (torch.float64, torch.float32))
    err32, T = ug.tolerance(sim32, sim64)
    err = float(((1.0 - wide.double().cpu()) - sim64).abs().max())
    gap = float((wide - gnn_distmat(xq, xg, k1, k2)).abs().max())
    print("wide range: err32 %.3g T %.3g device error %.3g, sparse - dense %.3g" % (err32, T, err, gap))
    assert err <= T and gap <= 2 * T
    assert bool((wide.cpu()[sim64 == 0] == 1.0).all())


def test_more_columns_than_the_lds_bitmap_holds():
    """N > 262 144 keeps the touched-column bitmap in the scratch row: symmetrise and propagate on a synthetic first
    ranking (k1 = 3, k2 = 2, in-degrees up to 16), against torch's sparse operations in float64 on the host.  B + B^T is
    exact.  A propagated value is a sum of at most two products of a rounded square and 1 or 2: three roundings, so
    4 * 2^-24 relative bounds it.  A norm is the root of a sum of n <= 38 squares, added in a chain of at most n + 8
    steps (a thread's own entries, then the tree over the workgroup): (n + 9) / 2 + 1 < 32 units of 2^-24 more."""
    from ieee_amd import _lib
    from ieee_amd.rerank import _Csr, _gs_propagate, _gs_symmetrise
    lib = _lib.require_gpu()
    N, k1, k2 = 262200, 3, 2
    i = torch.arange(N)
    rank = torch.stack([i % 20000, (i * 7919 + 13) % N, (i * 104729 + 7) % N], 1)
    assert not bool((rank[:, 1:] == rank[:, :1]).any()) and not bool((rank[:, 1] == rank[:, 2]).any())
    S = (0.5 + 0.5 * torch.rand(N, k1, generator=torch.Generator().manual_seed(0))).float()
    rows = i[:, None].expand(N, k1)
    B = torch.sparse_coo_tensor(torch.stack([rows.reshape(-1), rank.reshape(-1)]), torch.ones(N * k1, dtype=torch.float64), (N, N))
    M0 = (B + B.t()).coalesce()
    W = (S * S).double()
    sel = torch.sparse_coo_tensor(torch.stack([rows[:, :k2].reshape(-1), rank[:, :k2].reshape(-1)]), W[:, :k2].reshape(-1), (N, N))
    P = torch.sparse.mm(sel, M0).coalesce()

    sbytes = int(lib.ieee_gnn_sparse_scratch_bytes(200, N - 200, k1, k2))
    assert sbytes == 512 * ((N + (N + 31) // 32 + 63) // 64 * 64) * 4
    scratch = torch.zeros(sbytes, dtype=torch.uint8, device="cuda")
    rank_d, S_d = rank.int().cuda().contiguous(), S.cuda()
    b = _Csr(torch.arange(N + 1, dtype=torch.int64, device="cuda") * k1, rank_d.view(-1),
             torch.ones(N * k1, dtype=torch.float32, device="cuda"), None, N * k1)
    m0 = _gs_symmetrise(lib, b, N, scratch)
    p = _gs_propagate(lib, m0, rank_d, S_d, N, k1, k2, scratch)
    torch.cuda.synchronize()
    assert not bool(scratch.view(torch.int64).any()), "the scratch rows are left zero"
    for got, want, rel in ((m0, M0, 0.0), (p, P, 4 * 2.0 ** -24)):
        assert got.nnz == want._nnz()
        wr, wc = want.indices()
        assert torch.equal(got.rowptr.cpu(), torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(wr, minlength=N).cumsum(0)]))
        assert torch.equal(got.col.cpu()[:got.nnz].long(), wc)
        err = ((got.val.cpu()[:got.nnz].double() - want.values()).abs() / want.values().abs()).max()
        norm = torch.zeros(N, dtype=torch.float64).index_add_(0, wr, want.values() ** 2).sqrt()
        err_norm = ((got.norm.cpu().double() - norm).abs() / norm).max()
        print("N = %d: %d entries, value error %.3g (bound %.3g), norm error %.3g" % (N, got.nnz, err, rel, err_norm))
        assert err <= rel
        assert err_norm <= rel + 32 * 2.0 ** -24
