"""Query expansion on the device (ieee_amd/expansion.py, ieee_amd/csrc/expand.hip) against the float64 restatement of
tests/util_expansion.py, inside the bounds derived there; the lists against search_topk; the bits across blockings,
rounds and gallery forms; the memory picture; the engine keyword; the command."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import util_expansion as ux

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def inside(got, val, bound, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - val)
    share = float((err / np.where(bound > 0, bound, 1.0))[bound > 0].max()) if (bound > 0).any() else 0.0
    print("%s: %.1f %% of the bound" % (what, 100 * share))
    assert np.all(np.isfinite(got)), what
    assert np.all(err <= bound), (what, share)


# ---------------------------------------------------------------- 1. the sum kernel
# (d, k, n, n_src): every d, k, n and n_src of the issue's lists occurs; the kernel's path edges are d % 4 (16-byte or
# scalar loads) and d = 4096 (a row in registers, or tiles stored and scaled in a second pass): 4095, 4096, 4097, 4100
# sit on both sides of the second in both load forms, 8200 needs a third tile, 1024 / 1025 fill and overflow the first
# float4 of every thread
SUM_CASES = ((1, 1, 1, 1), (3, 2, 3, 7), (4, 5, 257, 300), (5, 64, 3, 7), (8, 1024, 3, 300), (64, 1024, 257, 300),
             (1023, 5, 3, 300), (1024, 2, 257, 7), (1025, 5, 3, 7), (2304, 5, 257, 300), (2304, 64, 3, 300),
             (4095, 5, 3, 7), (4096, 5, 3, 300), (4097, 2, 3, 7), (4100, 5, 3, 7), (8200, 5, 3, 7))
SPECIAL = (-1, None, -7, 2 ** 31 - 1)          # None stands for n_src


def sum_inputs(d, k, n, n_src, seed):
    """row-strided views into buffers whose padding is NaN (an index of 0 behind the lists): nothing reads it"""
    rng = np.random.RandomState(seed)
    src = rng.randn(n_src, d).astype(np.float32)
    if n_src > 1:
        src[1] = 0                                             # a zero row: rinv 1e12, contributes zero
    idx = rng.randint(0, n_src, (n, k)).astype(np.int64)
    if k > 1:
        idx[:, 1] = idx[:, 0]                                  # duplicates
        hit = rng.rand(n, k) < 0.25
        hit[:, 0] = False
        special = np.array([n_src if s is None else s for s in SPECIAL], np.int64)
        idx = np.where(hit, special[rng.randint(0, 4, (n, k))], idx)
    w = rng.rand(n, k).astype(np.float32)
    w[rng.rand(n, k) < 0.1] = 0
    own = rng.randn(n, d).astype(np.float32)
    pad = lambda a, cols, fill: np.concatenate([a, np.full((a.shape[0], cols), fill, a.dtype)], 1)
    big = dict(src=dev(pad(src, 4, NAN)), idx=dev(pad(idx.astype(np.int32), 3, 0)), w=dev(pad(w, 3, NAN)),
               own=dev(pad(own, 8, NAN)))
    views = dict(src=big["src"][:, :d], idx=big["idx"][:, :k], w=big["w"][:, :k], own=big["own"][:, :d])
    return dict(src=src, idx=idx, w=w, own=own), views


@pytest.mark.parametrize("case", SUM_CASES, ids=lambda c: "d%d-k%d-n%d-src%d" % c)
def test_neighbour_sum_against_float64(case):
    from ieee_amd.expansion import neighbour_sum, row_rinv
    d, k, n, n_src = case
    host, v = sum_inputs(d, k, n, n_src, seed=d + k)
    rinv, own_rinv = row_rinv(dev(host["src"])), row_rinv(dev(host["own"]))
    for use_rinv, own, normalize in itertools.product((False, True), (None, "plain", "scaled"), (False, True)):
        out = torch.full((n, d + 4), NAN, device="cuda")
        kw = dict(rinv=rinv if use_rinv else None, self_rows=v["own"] if own else None,
                  self_rinv=own_rinv if own == "scaled" else None, normalize=normalize)
        got = neighbour_sum(v["src"], v["idx"], v["w"], out=out[:, :d], **kw)
        assert got.data_ptr() == out.data_ptr() and bool(torch.isnan(out[:, d:]).all())     # the padding is not written
        val, _, bound = ux.restate_round(host["src"], host["idx"], host["w"], use_rinv=use_rinv,
                                         self_rows=host["own"] if own else None, self_scaled=own == "scaled",
                                         normalize=normalize)
        inside(got, val, bound, "rinv %s, self %s, normalize %s" % (use_rinv, own, normalize))
        # the same bits: again, into a contiguous output, and the rows in two calls
        assert np.array_equal(bits(neighbour_sum(v["src"], v["idx"], v["w"], **kw)), bits(got))
        if n > 1:
            h = n // 2
            halves = [neighbour_sum(v["src"], v["idx"][a:b], v["w"][a:b], rinv=kw["rinv"],
                                    self_rows=kw["self_rows"][a:b] if own else None,
                                    self_rinv=kw["self_rinv"][a:b] if own == "scaled" else None, normalize=normalize)
                      for a, b in ((0, h), (h, n))]
            assert np.array_equal(bits(torch.cat(halves)), bits(got))


def test_neighbour_sum_scalar_and_vector_loads_give_the_same_bits():
    """a misaligned view of the same values takes the scalar loads"""
    from ieee_amd.expansion import neighbour_sum, row_rinv
    for d, k in ((8, 5), (2304, 5), (4100, 3)):
        host, v = sum_inputs(d, k, 5, 7, seed=3)
        src = dev(host["src"])
        shifted = torch.empty(7 * d + 1, device="cuda")[1:].view(7, d).copy_(src)
        assert src.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
        rinv = row_rinv(src)
        a = neighbour_sum(src, v["idx"], v["w"], rinv=rinv)
        b = neighbour_sum(shifted, v["idx"], v["w"], rinv=rinv)
        assert np.array_equal(bits(a), bits(b))


def test_neighbour_sum_exact_cases():
    from ieee_amd import _lib
    from ieee_amd.expansion import neighbour_sum, row_rinv
    rng = np.random.RandomState(5)
    for d in (5, 8, 2304, 4100):
        src = dev(rng.randn(7, d).astype(np.float32))
        pick = dev(np.array([[3], [0], [6], [3]], np.int32))
        one = torch.ones(4, 1, device="cuda")
        got = neighbour_sum(src, pick, one, normalize=False)                  # k = 1, w = 1: the source row's bits
        assert np.array_equal(bits(got), bits(src[pick[:, 0].long()]))
        idx = dev(rng.randint(0, 7, (4, 5)).astype(np.int32))
        zeros = neighbour_sum(src, idx, torch.zeros(4, 5, device="cuda"), rinv=row_rinv(src), normalize=True)
        assert not bits(zeros).any()                                          # all-zero weights: +0.0 everywhere, no NaN
        src0 = src.clone()
        src0[2] = 0
        only = dev(np.full((3, 4), 2, np.int32))
        z = neighbour_sum(src0, only, torch.ones(3, 4, device="cuda"), rinv=row_rinv(src0), normalize=True)
        assert not bits(z).any()                                              # a zero row (rinv 1e12) contributes zero
        none = neighbour_sum(src, dev(np.array([[-1, 7, -7, 2 ** 31 - 1]], np.int32)), torch.ones(1, 4, device="cuda"))
        assert not bits(none).any()
        # no source rows at all: what is left is the self term
        empty = neighbour_sum(torch.empty(0, d, device="cuda"), pick, one, self_rows=src[:4].clone(), normalize=False)
        assert np.array_equal(bits(empty), bits(src[:4]))
    with pytest.raises(_lib.IeeeAmdError, match="out overlaps src"):
        neighbour_sum(src, pick, one, out=src[:4])
    with pytest.raises(_lib.IeeeAmdError, match="out overlaps the self rows"):
        own = torch.zeros(4, 4100, device="cuda")
        neighbour_sum(src, pick, one, self_rows=own, out=own)


# ---------------------------------------------------------------- 2. the weights and rinv
def test_weights_bit_for_bit():
    from ieee_amd.expansion import expand_weights
    dist = np.array([0, -1e-7, 0.25, 1, 1 + 1e-7, 2, np.inf, np.nan], np.float32)
    more = np.random.RandomState(1).rand(300).astype(np.float32) * np.float32(1.2)
    dist = np.concatenate([dist, dist, more]).reshape(4, -1)
    idx = np.zeros(dist.shape, np.int32)
    idx[0, 8:] = -1
    idx[1, :8] = -1
    idx[2, ::3] = -1
    idx[3] = 12345
    for alpha in (0, 1, 2, 3, 7, 64):
        got = expand_weights(dev(idx), dev(dist), alpha)
        assert np.array_equal(bits(got), ux.weights_fp32(idx, dist, alpha).view(np.uint32)), alpha


@pytest.mark.parametrize("d", (1, 5, 8, 24, 64, 1025, 2304))
def test_rinv_against_float64(d):
    from ieee_amd.expansion import row_rinv
    x = np.random.RandomState(d).randn(37, d).astype(np.float32) * np.float32(3)
    x[5] = 0
    x[6] = np.float32(1e-20)                                   # below the clamp as well
    got = row_rinv(dev(x)).cpu().numpy()
    want = ux.rinv64(x)
    assert got[5] == np.float32(1e12) and got[6] == np.float32(1e12)
    assert np.all(np.abs(got.astype(np.float64) - want) <= ux.c_r(d) * ux.U32 * want)


# ---------------------------------------------------------------- 3. the driver
@pytest.fixture(scope="module")
def fixtures():
    return {shape: ux.make_fixture(*shape) for shape in ux.FIXTURES}


def run_round(q, g, k, alpha, mode, **kw):
    from ieee_amd.expansion import expand_descriptors
    q2, g2, (idx, dist) = expand_descriptors(q, g, k=k, alpha=alpha, mode=mode, return_neighbours=True, **kw)
    return q2, g2, idx, dist


@pytest.mark.parametrize("mode", ("both", "query"))
@pytest.mark.parametrize("shape", ux.FIXTURES, ids=str)
def test_expand_descriptors_lists_and_values(fixtures, shape, mode):
    """k = N + 3 pads the lists; where N + 3 is beyond TOPK_MAX (the third fixture) the longest list there is, 1024,
    stands in for it"""
    from ieee_amd.metrics import search_topk
    from ieee_amd.metrics._stream import TOPK_MAX
    qh, gh = fixtures[shape]
    q, g = dev(qh), dev(gh)
    N = qh.shape[0] + gh.shape[0]
    rows_h = np.concatenate([qh, gh]) if mode == "both" else qh
    cand_h = rows_h if mode == "both" else gh
    rows, cand = (torch.cat([q, g]),) * 2 if mode == "both" else (q, g)
    for k in (1, 5, 64, min(N + 3, TOPK_MAX)):
        ref_idx, ref_dist = search_topk(rows, cand, k, metric="cosine")
        assert (N + 3 > TOPK_MAX) or (k < N + 3) or bool((ref_idx[:, -3:] == -1).all())
        for alpha in (0, 1, 3):
            q2, g2, idx, dist = run_round(q, g, k, alpha, mode)
            assert idx.dtype == torch.int64 and torch.equal(idx, ref_idx) and np.array_equal(bits(dist), bits(ref_dist))
            assert q2.dtype == torch.float32 and q2.is_cuda and tuple(q2.shape) == qh.shape
            if mode == "query":
                assert g2 is g
            w = ux.weights_fp32(idx.cpu().numpy(), dist.cpu().numpy(), alpha)
            val, _, bound = ux.restate_round(cand_h, idx.cpu().numpy(), w, self_rows=qh if mode == "query" else None)
            got = torch.cat([q2, g2]) if mode == "both" else q2
            inside(got, val, bound, "%s %s k=%d alpha=%d" % (shape, mode, k, alpha))


@pytest.mark.parametrize("mode", ("both", "query"))
@pytest.mark.parametrize("shape", ux.FIXTURES, ids=str)
def test_expand_descriptors_bits_do_not_depend_on_the_blocking(fixtures, shape, mode):
    """slab in {1, 100, None} x block in {1, 5, None}: all nine on the first fixture; on the larger ones the
    combinations of more than 25 000 (block, slab) distance launches (some 50 us each) are left to it, which keeps a
    case within seconds (every slab and every block value still occurs on every fixture)"""
    from ieee_amd.expansion import BLOCK_ROWS
    qh, gh = fixtures[shape]
    q, g = dev(qh), dev(gh)
    n_rows = sum(shape[:2]) if mode == "both" else shape[0]
    n_cand = sum(shape[:2]) if mode == "both" else shape[1]
    want = run_round(q, g, 5, 3, mode)
    ran = set()
    for slab, block in itertools.product((1, 100, None), (1, 5, None)):
        if -(-n_rows // (block or BLOCK_ROWS)) * -(-n_cand // (slab or n_cand)) > 25000:
            continue
        ran.add((slab, block))
        got = run_round(q, g, 5, 3, mode, slab=slab, block=block)
        assert np.array_equal(bits(got[0]), bits(want[0])) and torch.equal(got[2], want[2])
        assert np.array_equal(bits(got[3]), bits(want[3]))
        if mode == "both":
            assert np.array_equal(bits(got[1]), bits(want[1]))
    assert {s for s, _ in ran} == {1, 100, None} and {b for _, b in ran} == {1, 5, None}
    assert shape != ux.FIXTURES[0] or len(ran) == 9


@pytest.mark.parametrize("mode", ("both", "query"))
def test_expand_descriptors_rounds_chain(fixtures, mode):
    from ieee_amd.expansion import expand_descriptors
    for shape in ux.FIXTURES[:2]:
        q, g = (dev(a) for a in fixtures[shape])
        twice = expand_descriptors(q, g, 5, 3, times=2, mode=mode)
        once = expand_descriptors(q, g, 5, 3, mode=mode)
        chained = expand_descriptors(once[0].contiguous(), once[1].contiguous(), 5, 3, mode=mode)
        assert np.array_equal(bits(twice[0]), bits(chained[0])) and np.array_equal(bits(twice[1]), bits(chained[1]))
        assert not np.array_equal(bits(twice[0]), bits(once[0]))


@pytest.mark.parametrize("shape", ux.FIXTURES, ids=str)
def test_query_mode_gallery_forms(fixtures, shape):
    """host tensor, and host and device pieces with an empty one among them: the device tensor's bits"""
    qh, gh = fixtures[shape]
    q, g = dev(qh), dev(gh)
    want = run_round(q, g, 5, 3, "query")
    host = torch.from_numpy(gh)
    G = gh.shape[0]
    a, b = G // 3, G // 3 + max(1, G // 4)
    pieces = [host[:a], g[a:b], host[:0], host[b:].double()]
    for gallery, kw in ((host, {}), (pieces, {}), (tuple(pieces), dict(slab=3 if G < 100 else 700, block=2))):
        got = run_round(q, gallery, 5, 3, "query", **kw)
        assert got[1] is gallery
        assert np.array_equal(bits(got[0]), bits(want[0])) and torch.equal(got[2], want[2])
    # fp16 and float64 queries are taken to fp32 like any distance input
    q16 = run_round(q.half(), g, 5, 3, "query")[0]
    assert np.array_equal(bits(q16), bits(run_round(q.half().float(), g, 5, 3, "query")[0]))


@pytest.mark.parametrize("shape", ux.FIXTURES, ids=str)
def test_k1_alpha0_is_normalisation(fixtures, shape):
    """every row of these fixtures is its own nearest neighbour (tests/test_expansion_cpu.py checks that)"""
    qh, gh = fixtures[shape]
    X = np.concatenate([qh, gh])
    q2, g2, idx, _ = run_round(dev(qh), dev(gh), 1, 0, "both")
    assert np.array_equal(idx.cpu().numpy()[:, 0], np.arange(len(X)))
    val, _, bound = ux.restate_round(X, np.arange(len(X))[:, None], np.ones((len(X), 1)))
    assert np.abs(val - X.astype(np.float64) * ux.rinv64(X)[:, None]).max() < 1e-15
    inside(torch.cat([q2, g2]), val, bound, "%s normalise" % (shape,))
    want = torch.nn.functional.normalize(dev(X).double(), p=2, dim=1).cpu().numpy()
    inside(torch.cat([q2, g2]), want, bound, "%s F.normalize" % (shape,))


def test_empty_sides(fixtures):
    from ieee_amd.expansion import expand_descriptors
    qh, gh = fixtures[ux.FIXTURES[1]]
    q = dev(qh)
    q2, g2, (idx, dist) = expand_descriptors(q, torch.zeros(0, 64), 5, 3, mode="query", return_neighbours=True)
    assert tuple(g2.shape) == (0, 64) and bool((idx == -1).all()) and bool(torch.isinf(dist).all())
    val, _, bound = ux.restate_round(np.zeros((0, 64), np.float32), idx.cpu().numpy(), np.zeros(idx.shape), self_rows=qh)
    assert np.abs(val - qh.astype(np.float64) * ux.rinv64(qh)[:, None]).max() < 1e-15
    inside(q2, val, bound, "G = 0")
    a, b = expand_descriptors(q[:0], dev(gh), 5, 3)
    assert tuple(a.shape) == (0, 64) and tuple(b.shape) == gh.shape
    a, b = expand_descriptors(q[:0], dev(gh)[:0], 5, 3)
    assert tuple(a.shape) == (0, 64) and tuple(b.shape) == (0, 64)
    a, b = expand_descriptors(q[:0], dev(gh), 5, 3, mode="query")
    assert tuple(a.shape) == (0, 64)


# ---------------------------------------------------------------- 4. memory
def test_memory_stays_within_the_layout():
    from ieee_amd.expansion import expand_descriptors, expansion_layout
    Q, G, d, k = 5000, 15000, 64, 5
    gen = torch.Generator().manual_seed(0)
    q, g = torch.randn(Q, d, generator=gen).cuda(), torch.randn(G, d, generator=gen).cuda()
    total = expansion_layout(Q, G, d, k)["total"]
    assert total < (Q + G) ** 2 * 4 // 5
    out = expand_descriptors(q, g, k, 3)
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = expand_descriptors(q, g, k, 3, return_neighbours=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak %.1f MB, layout %.1f MB, N x N %.1f MB" % (peak / 1e6, total / 1e6, (Q + G) ** 2 * 4 / 1e6))
    assert peak <= total


# ---------------------------------------------------------------- 5. the engine
class DM(object):
    num_train_pids = 10
    sources = ["synthetic"]
    train_loader = []
    test_loader = {"synthetic": {"query": "query", "gallery": "gallery"}}


def test_engine_query_expansion(capsys, monkeypatch, tmp_path):
    from ieee_amd import engine as E
    from ieee_amd.expansion import expand_descriptors
    from ieee_amd.metrics import compute_distance_matrix, evaluate_rank, evaluate_rank_streamed
    from ieee_amd.rerank import re_ranking
    qh, gh = ux.make_fixture(17, 300, 64)
    rng = np.random.RandomState(2)
    labels = (rng.randint(0, 12, 17), rng.randint(0, 12, 300), rng.randint(0, 3, 17), rng.randint(0, 3, 300))
    qf, gf = dev(qh), dev(gh)
    fixed = {"query": (qf, labels[0], labels[2]), "gallery": (gf, labels[1], labels[3])}
    eng = E.Engine(DM(), use_gpu=True)
    eng._descriptors = lambda loader, clock: fixed[loader]
    report = lambda: [ln for ln in capsys.readouterr().out.splitlines() if not ln.startswith("Speed:")]
    eq, eg = expand_descriptors(qf, gf, 3, 3)
    dm = compute_distance_matrix(eq, eg)
    cmc, m_ap = evaluate_rank(dm, *labels)
    assert eng.test(query_expansion=dict(k=3, alpha=3), ranks=[1, 5]) == m_ap
    said = report()
    assert "Applying query expansion (k=3, alpha=3, times=1, mode=both) ..." in said
    assert "mAP: {:.2%}".format(m_ap) in said and "Rank-1  : {:.2%}".format(cmc[0]) in said
    # the streamed evaluation and re-ranking take the expanded descriptors unchanged
    cmc_s, map_s = evaluate_rank_streamed(eq, eg, *labels)
    assert eng.test(query_expansion=dict(k=3, alpha=3), stream_eval=True, ranks=[1]) == map_s
    assert "mAP: {:.2%}".format(map_s) in report()
    rr = re_ranking(dm, compute_distance_matrix(eq, eq), compute_distance_matrix(eg, eg))
    assert eng.test(query_expansion=dict(k=3, alpha=3), rerank=True, ranks=[1]) == evaluate_rank(rr, *labels)[1]
    report()
    # True: the defaults; through run() as well
    dflt = evaluate_rank(compute_distance_matrix(*expand_descriptors(qf, gf)), *labels)[1]
    eng.run(test_only=True, query_expansion=True, ranks=[1], save_dir=str(tmp_path))
    said = report()
    assert "Applying query expansion (k=5, alpha=3, times=1, mode=both) ..." in said and "mAP: {:.2%}".format(dflt) in said
    # off: the report of the call without the keyword, and no expansion line
    plain = eng.test(ranks=[1, 5])
    plain_said = report()
    assert not any("query expansion" in ln for ln in plain_said)
    for off in (None, False):
        assert eng.test(query_expansion=off, ranks=[1, 5]) == plain and report() == plain_said
    assert plain != m_ap                            # the step does something on this fixture


# ---------------------------------------------------------------- 6. the command
def test_evaluate_gallery_command():
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "evaluate_gallery.py"), "--synthetic", "50,400,64", "--ids", "20"]
    with_qe = subprocess.run(cmd + ["--qe-k", "5"], capture_output=True, text=True, timeout=600, env=env)
    assert with_qe.returncode == 0, with_qe.stderr[-2000:]
    lines = with_qe.stdout.splitlines()
    assert sum(ln.startswith("streamed: mAP") for ln in lines) == 1
    assert sum(ln.startswith("streamed after query expansion (k=5, alpha=3, times=1, mode=both): mAP") for ln in lines) == 1
    without = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert without.returncode == 0, without.stderr[-2000:]
    assert "expansion" not in without.stdout and sum(ln.startswith("streamed: mAP") for ln in without.stdout.splitlines()) == 1
    assert [ln for ln in lines if ln.startswith("streamed: mAP")] == \
        [ln for ln in without.stdout.splitlines() if ln.startswith("streamed: mAP")]
