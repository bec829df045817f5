"""CPU: the host side of the streamed CMC / mAP (ieee_amd/metrics/rank_stream.py).  The plan -- per query the gallery
indices of its true matches and of its removed entries, and match_columns -- against a brute-force double loop, and
every ValueError that is raised before a device is needed, the engine's stream_eval checks among them."""
import numpy as np
import pytest
import torch


def brute(qp, qc, gp, gc):
    matches, removed, cols = [], [], set()
    for q in range(len(qp)):
        m = [j for j in range(len(gp)) if gp[j] == qp[q] and gc[j] != qc[q]]
        r = [j for j in range(len(gp)) if gp[j] == qp[q] and gc[j] == qc[q]]
        matches.append(m)
        removed.append(r)
        cols |= set(m) | set(r)
    return matches, removed, sorted(cols)


def check_plan(qp, qc, gp, gc):
    from ieee_amd.metrics.rank_stream import RankAccumulator
    acc = RankAccumulator(qp, qc, gp, gc)
    p = acc.plan
    matches, removed, cols = brute(qp, qc, gp, gc)
    assert acc.num_q == len(qp) and acc.num_g == len(gp) and acc.num_collected == 0 and acc.num_counted == 0
    assert acc.match_columns.dtype == np.int64 and acc.match_columns.tolist() == cols
    assert p.m_off.dtype == np.int64 and p.r_off.dtype == np.int64 and p.m_idx.dtype == np.int32
    assert p.m_off.shape == p.r_off.shape == (len(qp) + 1,) and p.m_off[0] == 0 and p.r_off[0] == 0
    for q in range(len(qp)):
        assert sorted(p.m_idx[p.m_off[q]:p.m_off[q + 1]].tolist()) == matches[q], q      # each once, in any order
        assert sorted(p.r_idx[p.r_off[q]:p.r_off[q + 1]].tolist()) == removed[q], q
    assert p.m_off[-1] == p.m_idx.size == p.m_pos.size and p.r_off[-1] == p.r_idx.size == p.r_pos.size
    assert (acc.match_columns[p.m_pos] == p.m_idx).all() and (acc.match_columns[p.r_pos] == p.r_idx).all()
    return acc


@pytest.mark.parametrize("seed", range(12))
def test_plan_against_a_double_loop(seed):
    rng = np.random.RandomState(seed)
    for _ in range(6):
        Q, G = rng.randint(1, 41), rng.randint(1, 501)
        ids, cams = rng.randint(1, 40), rng.randint(1, 5)
        # identities 0 ... ids-1 on the query side, shifted on the gallery side: some are absent from either
        qp, gp = rng.randint(0, ids, Q), rng.randint(0, ids, G) + rng.randint(0, 3)
        check_plan(qp, rng.randint(0, cams, Q), gp, rng.randint(0, cams, G))


def test_plan_edges():
    # negative and extreme labels sort like any other
    big = np.iinfo(np.int32).max
    qp, qc = np.array([-5, big, -big - 1, 0]), np.array([-1, big, 0, -big - 1])
    gp = np.array([0, -5, big, -5, -big - 1, big, 0, 7])
    gc = np.array([-big - 1, -1, big, 3, 0, 0, 2, 7])
    check_plan(qp, qc, gp, gc)
    # a query whose matches are all on its own camera: no true match, only removed entries
    acc = check_plan(np.array([1, 2]), np.array([0, 0]), np.array([1, 1, 2, 3]), np.array([0, 0, 1, 0]))
    assert acc.plan.m_off.tolist() == [0, 0, 1] and acc.plan.r_off.tolist() == [0, 2, 2]
    # no identity in common, an empty query set, an empty gallery
    assert check_plan(np.array([1, 2]), np.array([0, 0]), np.array([3, 4]), np.array([0, 1])).match_columns.size == 0
    acc = check_plan(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.array([3, 4]), np.array([0, 1]))
    assert acc.match_columns.size == 0 and acc.plan.m_off.tolist() == [0]
    check_plan(np.array([1]), np.array([0]), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    # torch labels are taken too
    check_plan(torch.tensor([1, 2]), torch.tensor([0, 1]), torch.tensor([2, 1, 1]), torch.tensor([0, 0, 1]))


def test_an_empty_query_set_needs_no_device():
    from ieee_amd.metrics.rank_stream import RankAccumulator
    acc = RankAccumulator(np.zeros(0), np.zeros(0), np.array([3, 4, 5]), np.array([0, 1, 1]), max_rank=2)
    acc.seal()
    with pytest.raises(ValueError, match="0 of the 3 gallery columns"):
        acc.result()
    acc.count(np.zeros((0, 3), dtype=np.float32), 0)
    counts, nv, ap = acc.result()
    assert counts.tolist() == [0, 0] and counts.dtype == np.int64 and nv == 0.0 and ap == 0.0


def labels(Q=4, G=30):
    rng = np.random.RandomState(3)
    return rng.randint(0, 5, Q), rng.randint(0, 3, Q), rng.randint(0, 5, G), rng.randint(0, 3, G)


def test_label_checks():
    from ieee_amd.metrics.rank_stream import RankAccumulator
    qp, qc, gp, gc = labels()
    with pytest.raises(ValueError, match="q_camids has 3 entries, expected 4"):
        RankAccumulator(qp, qc[:3], gp, gc)
    with pytest.raises(ValueError, match="g_camids has 29 entries, expected 30"):
        RankAccumulator(qp, qc, gp, gc[:29])
    for i, name in enumerate(("q_pids", "q_camids", "g_pids", "g_camids")):
        args = [np.asarray(a, dtype=np.int64).copy() for a in (qp, qc, gp, gc)]
        args[i][0] = 1 << 31
        with pytest.raises(ValueError, match="%s does not fit int32" % name):
            RankAccumulator(*args)
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(ValueError, match="max_rank"):
            RankAccumulator(qp, qc, gp, gc, max_rank=bad)
    with pytest.raises(ValueError, match="device"):
        RankAccumulator(qp, qc, gp, gc, device="cpu")
    assert RankAccumulator(qp, qc, gp, gc, max_rank=50).max_rank == 30      # rank.py:110-115


def test_call_order_and_ranges_are_checked_before_the_device():
    from ieee_amd.metrics.rank_stream import RankAccumulator
    qp, qc, gp, gc = labels()
    acc = RankAccumulator(qp, qc, gp, gc)
    n = acc.match_columns.size
    assert 0 < n < 30
    slab = lambda w: np.zeros((4, w), dtype=np.float32)
    with pytest.raises(ValueError, match="before seal"):
        acc.count(slab(30), 0)
    with pytest.raises(ValueError, match=r"must be \[4, n\]"):
        acc.collect(np.zeros((3, 2), dtype=np.float32))
    with pytest.raises(ValueError, match=r"must be \[4, n\]"):
        acc.collect(np.zeros(4, dtype=np.float32))
    with pytest.raises(ValueError, match="run past the %d match columns" % n):
        acc.collect(slab(n + 1))
    with pytest.raises(ValueError, match="0 of the %d match columns were collected" % n):
        acc.seal()
    with pytest.raises(ValueError, match="gallery columns were counted"):
        acc.result()
    assert acc.num_collected == 0 and acc.num_counted == 0 and not acc.sealed


def test_counted_ranges():
    """the interval book-keeping of count(), which runs before any launch"""
    from ieee_amd.metrics.rank_stream import RankAccumulator
    qp, qc, gp, gc = labels()
    acc = RankAccumulator(qp, qc, gp, gc)
    acc.sealed = True                              # the checks below come before the device is asked for
    with pytest.raises(ValueError, match="run past the gallery's 30"):
        acc.count(np.zeros((4, 5), dtype=np.float32), 26)
    with pytest.raises(ValueError, match="run past"):
        acc.count(np.zeros((4, 5), dtype=np.float32), -1)
    acc._claim(10, 5)
    acc._claim(0, 10)
    acc._claim(20, 10)
    assert acc.num_counted == 25
    for lo, w in ((10, 5), (14, 1), (9, 2), (0, 30), (12, 1), (19, 2), (29, 1)):
        with pytest.raises(ValueError, match="overlap a range counted before"):
            acc.count(np.zeros((4, w), dtype=np.float32), lo)
    assert acc.num_counted == 25
    acc._claim(15, 0)                              # an empty slab claims nothing
    acc._claim(15, 5)
    assert acc.num_counted == acc.num_g == 30


def test_streamed_evaluation_checks():
    from ieee_amd.metrics import evaluate_rank_streamed, rank_counts_streamed
    qp, qc, gp, gc = labels()
    q, g = torch.zeros(4, 8), torch.zeros(30, 8)
    for fn in (evaluate_rank_streamed, rank_counts_streamed):
        with pytest.raises(ValueError, match="walked twice.*one-shot iterator"):
            fn(q, (piece for piece in (g[:10], g[10:])), qp, gp, qc, gc)
        with pytest.raises(ValueError, match="walked twice"):
            fn(q, iter([g]), qp, gp, qc, gc)
        with pytest.raises(ValueError, match=r"must be a \[g, 8\] tensor"):
            fn(q, [g[:10], torch.zeros(20, 9)], qp, gp, qc, gc)
        with pytest.raises(ValueError, match="g_pids has 30 entries, expected 29"):
            fn(q, g[:29], qp, gp, qc, gc)
        with pytest.raises(ValueError, match="q_camids has 3 entries, expected 4"):
            fn(q, g, qp, gp, qc[:3], gc)
        with pytest.raises(ValueError, match="Unknown distance metric"):
            fn(q, g, qp, gp, qc, gc, metric="manhattan")
        with pytest.raises(ValueError, match="Unknown distmat precision"):
            fn(q, g, qp, gp, qc, gc, precision="fp8")
        with pytest.raises(ValueError, match="slab must be a positive integer"):
            fn(q, g, qp, gp, qc, gc, slab=0)
        with pytest.raises(ValueError, match=r"query must be a \[Q, d\] tensor"):
            fn(np.zeros((4, 8)), g, qp, gp, qc, gc)


def test_engine_refuses_stream_eval_with_rerank_and_cuhk03():
    from ieee_amd.engine import Engine

    class DM(object):
        num_train_pids = 3
        sources = ["synthetic"]
        train_loader = []
        test_loader = {"synthetic": {"query": "query", "gallery": "gallery"}}
    eng = Engine(DM(), use_gpu=False)
    seen = []
    eng._descriptors = lambda loader, clock: seen.append(loader)
    for rerank in (True, 'gnn'):
        with pytest.raises(ValueError, match="stream_eval=True cannot be combined with rerank"):
            eng.test(stream_eval=True, rerank=rerank)
        with pytest.raises(ValueError, match="stream_eval=True cannot be combined with rerank"):
            eng.run(test_only=True, stream_eval=True, rerank=rerank)
        with pytest.raises(ValueError, match="stream_eval=True cannot be combined with rerank"):
            eng._evaluate(dataset_name="synthetic", stream_eval=True, rerank=rerank)
    with pytest.raises(ValueError, match="use_metric_cuhk03"):
        eng.test(stream_eval=True, use_metric_cuhk03=True)
    with pytest.raises(ValueError, match="use_metric_cuhk03"):
        eng.run(test_only=True, stream_eval=True, use_metric_cuhk03=True)
    with pytest.raises(ValueError, match="use_metric_cuhk03"):
        eng._evaluate(dataset_name="synthetic", stream_eval=True, use_metric_cuhk03=True)
    assert seen == []


def test_engine_refuses_stream_eval_over_several_ranks(monkeypatch):
    from ieee_amd import dist as ddp
    from ieee_amd.engine import Engine

    class DM(object):
        num_train_pids = 3
        sources = ["synthetic"]
        train_loader = []
        test_loader = {}
    monkeypatch.setattr(ddp, "world_size", lambda: 2)
    with pytest.raises(ValueError, match="stream_eval=True runs on one rank"):
        Engine(DM(), use_gpu=False)._evaluate(dataset_name="x", stream_eval=True)
