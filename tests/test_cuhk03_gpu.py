"""GPU: ieee_rank_cuhk03 (the CUHK03 single-gallery-shot protocol in closed form) through cuhk03_sums / eval_cuhk03 /
eval_regdb / evaluate_rank / Engine.test, against the float64 restatement tests/util_cuhk03.py (itself checked on the
CPU against the enumerated protocol and the sampled reference, tests/test_cuhk03_cpu.py).

The bound on a per-query curve value or AP is derived, not fitted: every value is at most 1, each of the P recurrence
steps costs at most 3 roundings, the sums over max_rank and over the n_t true matches one each, so
(3 P + max_rank + n_t) * 2^-52; totals over the valid queries get that bound times their number."""
import os

import numpy as np
import pytest
import torch

from tests.util_cuhk03 import cuhk03_reference, error_bound
from tests.util_model import C, id_loader

pytestmark = pytest.mark.gpu

RANKS = (1, 5, 20, 50)
SHAPES = [(1, 1, 1), (3, 7, 2), (17, 2049, 40), (9, 4096, 300), (33, 5003, 751)]


def labels(rng, Q, G, ids, cams=3, times=2):
    return (rng.randint(0, ids, Q), rng.randint(0, ids, G), rng.randint(0, cams, Q), rng.randint(0, cams, G),
            rng.randint(0, times, Q), rng.randint(0, times, G))


def random_case(Q, G, ids, seed):
    rng = np.random.RandomState(seed)
    qp, gp, qc, gc, qt, gt = labels(rng, Q, G, ids)
    d = rng.rand(Q, G).astype(np.float32)
    # every other query has its identity near the top, so that the curves are neither all ~0 nor saturated
    near = (qp[:, None] == gp[None, :]) & (np.arange(Q)[:, None] % 2 == 0)
    d[near] *= np.float32(0.05)
    return d, qp, gp, qc, gc, qt, gt


def check_against(case, max_rank, ref, what):
    """one cuhk03_sums call at max_rank against `ref`, the restatement at a max_rank at least as large (its leading
    columns are the curve for any smaller one); returns the call's results"""
    from ieee_amd.metrics.rank import cuhk03_sums
    sums, nv, ap_sum, cmc, ap = cuhk03_sums(*case, max_rank)
    cmc, ap = cmc.cpu().numpy(), ap.cpu().numpy()
    P = len(np.unique(case[2]))
    want = ref["cmc"][:, :max_rank]
    assert cmc.dtype == np.float64 and cmc.shape == want.shape and sums.dtype == np.float64
    assert np.array_equal(ap >= 0, ref["valid"]), what
    assert nv == ref["num_valid"]
    bound = np.array([error_bound(P, max_rank, n) for n in ref["n_true"]])
    e_cmc = np.abs(cmc - want).max(1)
    e_ap = np.abs(ap - ref["ap"])
    print(what, "max_rank", max_rank, "worst curve error %.3g AP error %.3g of bound %.3g" %
          (e_cmc.max(), e_ap.max(), bound.min()))
    assert np.all(e_cmc <= bound), (what, max_rank, e_cmc.max(), bound.min())
    assert np.all(e_ap <= bound), (what, max_rank, e_ap.max(), bound.min())
    assert np.all(cmc[~ref["valid"]] == 0) and np.all(ap[~ref["valid"]] == -1)
    total = bound.max() * max(nv, 1)
    assert np.all(np.abs(sums - want[ref["valid"]].sum(0)) <= total)
    assert abs(ap_sum - ref["ap_sum"]) <= total
    return sums, nv, ap_sum, cmc, ap


@pytest.fixture(scope="module")
def cases():
    """the random cases and their restatement at the largest max_rank, computed once"""
    out = {}
    for i, (Q, G, ids) in enumerate(SHAPES):
        case = random_case(Q, G, ids, 100 + i)
        out[(Q, G, ids)] = (case, cuhk03_reference(*case, max(RANKS)))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_curves_and_aps_match_the_restatement(cases, shape, capsys):
    from ieee_amd.metrics import eval_cuhk03
    case, ref = cases[shape]
    for max_rank in RANKS:                       # beyond the identity count the tail of ones appears
        check_against(case, max_rank, ref, str(shape))
    if shape[2] < max(RANKS) and ref["num_valid"]:
        assert np.all(np.abs(ref["cmc"][ref["valid"]][:, shape[2]:] - 1.0) < 1e-12)
    # the public entry point: float32 curve, clamped to the gallery size with the reference's note
    capsys.readouterr()
    if ref["num_valid"] == 0:
        with pytest.raises(AssertionError, match="all query identities"):
            eval_cuhk03(*case, 20)
        return
    all_cmc, m_ap = eval_cuhk03(*case, 20)
    note = capsys.readouterr().out
    R = min(20, shape[1])
    assert ("quite small, got {}".format(shape[1]) in note) == (shape[1] < 20)
    assert all_cmc.dtype == np.float32 and all_cmc.shape == (R,) and isinstance(m_ap, float)
    want = (ref["cmc"][ref["valid"]][:, :R].sum(0) / ref["num_valid"])
    assert np.all(np.abs(all_cmc.astype(np.float64) - want) <= 2.0 ** -24)        # one float32 rounding of a value <= 1
    assert abs(m_ap - ref["mAP"]) <= error_bound(shape[2], 20, ref["n_true"].max())


@pytest.mark.parametrize("ids", [3, 20])
def test_integer_distances_tie_to_the_lower_gallery_index(ids):
    rng = np.random.RandomState(ids)
    Q, G = 12, 6000
    qp, gp, qc, gc, qt, gt = labels(rng, Q, G, ids)
    d = rng.randint(0, 6, size=(Q, G)).astype(np.float32)
    case = (d, qp, gp, qc, gc, qt, gt)
    check_against(case, 20, cuhk03_reference(*case, 20), "integer distances, %d identities" % ids)


def big_identity_case():
    """identity 7 owns 1 500 of 2 000 gallery images, 800 of them under key (0, 0): query 0 has identity 7 and that key
    (700 kept true matches, 800 removed: many batches), query 1 has identity 7 and a key nobody has (1 500 kept),
    queries 2 and 3 another identity (identity 7 is then an OTHER identity with a long segment)"""
    rng = np.random.RandomState(77)
    G = 2000
    gp = np.concatenate([np.full(1500, 7), rng.randint(8, 30, 500)])
    gc = np.concatenate([np.zeros(800, dtype=np.int64), rng.randint(1, 3, 700), rng.randint(0, 3, 500)])
    gt = np.concatenate([np.zeros(800, dtype=np.int64), rng.randint(0, 2, 700), rng.randint(0, 2, 500)])
    perm = rng.permutation(G)
    gp, gc, gt = gp[perm], gc[perm], gt[perm]
    qp, qc, qt = np.array([7, 7, 9, 12]), np.array([0, 5, 1, 0]), np.array([0, 0, 1, 0])
    d = rng.rand(4, G).astype(np.float32)
    return d, qp, gp, qc, gc, qt, gt


def test_long_segments_and_many_true_matches():
    case = big_identity_case()
    ref = cuhk03_reference(*case, 20)
    assert ref["n_true"].tolist()[:2] == [700, 1500]
    check_against(case, 20, ref, "one identity owns 1500 of 2000")


def test_a_gallery_of_the_query_identity_gives_a_curve_of_ones():
    from ieee_amd.metrics.rank import cuhk03_sums
    rng = np.random.RandomState(3)
    G = 300
    d = rng.rand(2, G).astype(np.float32)
    qp, gp = np.array([5, 5]), np.full(G, 5)
    qc, gc, qt, gt = np.array([0, 1]), rng.randint(0, 2, G), np.array([0, 1]), rng.randint(0, 2, G)
    sums, nv, ap_sum, cmc, ap = cuhk03_sums(d, qp, gp, qc, gc, qt, gt, 10)
    assert nv == 2 and np.all(cmc.cpu().numpy() == 1.0) and np.all(ap.cpu().numpy() == 1.0)
    assert np.all(sums == 2.0) and ap_sum == 2.0


def test_every_query_skipped_trips_the_assertion():
    from ieee_amd.metrics import eval_cuhk03, evaluate_rank
    rng = np.random.RandomState(4)
    d = rng.rand(3, 40).astype(np.float32)
    gp = rng.randint(0, 5, 40)
    z = np.zeros(40, dtype=np.int64)
    # identities the gallery lacks, and one whose every entry has the query's camera and time id
    with pytest.raises(AssertionError, match="all query identities do not appear in gallery"):
        eval_cuhk03(d, np.array([9, 10, 0]), gp, np.zeros(3), z, np.zeros(3), z, 5)
    with pytest.raises(AssertionError, match="all query identities do not appear in gallery"):
        evaluate_rank(d, np.array([9, 10, 11]), gp, np.zeros(3), z, max_rank=5, use_metric_cuhk03=True)


def test_row_stride_and_input_kinds(cases):
    """a view into a wider matrix (row stride > num_g), a device tensor and a NumPy array give the same bits"""
    from ieee_amd.metrics.rank import cuhk03_sums
    case, ref = cases[(17, 2049, 40)]
    d = case[0]
    wide = torch.full((17, 2049 + 37), -1.0, device="cuda")
    wide[:, :2049] = torch.from_numpy(d).cuda()
    view = wide[:, :2049]
    assert view.stride(0) == 2049 + 37
    a = cuhk03_sums(d, *case[1:], 20)
    b = cuhk03_sums(view, *case[1:], 20)
    c = cuhk03_sums(torch.from_numpy(d).cuda(), *case[1:], 20)
    for other in (b, c):
        assert np.array_equal(a[0], other[0]) and a[1:3] == other[1:3]
        assert torch.equal(a[3], other[3]) and torch.equal(a[4], other[4])
    assert np.all(np.abs(a[3].cpu().numpy() - ref["cmc"][:, :20]).max(1) <=
                  [error_bound(40, 20, n) for n in ref["n_true"]])


def test_single_shot_gallery_equals_the_market_protocol():
    """with one image per identity nothing is left to draw: the curve is the Market protocol's, with the folded
    (camera, time id) keys as cameras -- equal float32 curves and the same float for the mAP"""
    from ieee_amd.metrics import eval_cuhk03, eval_market1501
    from ieee_amd.metrics.rank import fold_keys
    rng = np.random.RandomState(8)
    Q, G = 60, 700
    gp = rng.permutation(G) + 3
    qp = np.concatenate([gp[rng.randint(0, G, Q - 4)], [0, 1, 2, 5000]])       # four queries the gallery lacks
    qc, gc, qt, gt = rng.randint(0, 2, Q), rng.randint(0, 2, G), rng.randint(0, 2, Q), rng.randint(0, 2, G)
    d = rng.rand(Q, G).astype(np.float32)
    d[qp[:, None] == gp[None, :]] *= np.float32(0.02)
    qk, gk = fold_keys(qc, gc, qt, gt)
    assert qk.dtype == np.int32 and len(np.unique(np.concatenate([qk, gk]))) == 4
    a_cmc, a_map = eval_cuhk03(d, qp, gp, qc, gc, qt, gt, 50)
    m_cmc, m_map = eval_market1501(d, qp, gp, qk, gk, 50)
    assert a_cmc.dtype == m_cmc.dtype == np.float32
    assert np.array_equal(a_cmc, m_cmc) and a_map == m_map
    assert 0 < a_cmc[0] < a_cmc[-1] <= 1


def test_null_time_ids_equal_all_zero_time_ids(cases):
    from ieee_amd.metrics import eval_cuhk03, evaluate_rank
    d, qp, gp, qc, gc, qt, gt = cases[(9, 4096, 300)][0]
    a = eval_cuhk03(d, qp, gp, qc, gc, None, None, 20)
    b = eval_cuhk03(d, qp, gp, qc, gc, 0 * qt, 0 * gt, 20)
    c = evaluate_rank(d, qp, gp, qc, gc, max_rank=20, use_metric_cuhk03=True)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert np.array_equal(a[0], c[0]) and a[1] == c[1]
    with_time = evaluate_rank(d, qp, gp, qc, gc, max_rank=20, use_metric_cuhk03=True, q_timeids=qt, g_timeids=gt)
    assert with_time[1] != a[1]                                      # the time ids do reach the filter


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cuhk03_golden.npz"))


@pytest.mark.parametrize("name", ["a", "b"])
def test_golden_reference_runs_on_the_device(golden, name):
    from ieee_amd.metrics import eval_cuhk03
    g = {k[2:]: golden[k] for k in golden.files if k.startswith(name + "_")}
    cmc, m_ap = eval_cuhk03(g["distmat"], g["q_pids"], g["g_pids"], g["q_camids"], g["g_camids"], g["q_timeids"],
                            g["g_timeids"], int(g["max_rank"]))
    z = np.abs(cmc.astype(np.float64) - g["cmc_mean"]) / g["cmc_sem"]
    print(name, "z-scores", z)
    assert np.all(z <= 5.0), z
    assert abs(m_ap - float(g["mAP"])) <= 1e-12 * abs(float(g["mAP"]))


def test_regdb_equals_the_reference(golden, capsys):
    from ieee_amd.metrics import eval_regdb
    cmc, m_ap = eval_regdb(golden["b_distmat"], golden["b_q_pids"], golden["b_g_pids"], golden["b_q_timeids"],
                           golden["b_g_timeids"])
    assert capsys.readouterr().out == ""                              # none of the reference's debug prints
    print("regdb mAP", repr(m_ap), "stored", repr(float(golden["b_regdb_mAP"])))
    assert cmc.dtype == np.float32 and np.array_equal(cmc, golden["b_regdb_cmc"])
    assert m_ap == float(golden["b_regdb_mAP"])


def test_two_calls_give_the_same_bits():
    from ieee_amd.metrics.rank import cuhk03_sums
    case = big_identity_case()
    a = cuhk03_sums(*case, 50)
    b = cuhk03_sums(*case, 50)
    assert np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and a[1:3] == b[1:3]
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])


def test_bad_arguments_are_refused_before_a_launch():
    from ieee_amd import _lib
    lib = _lib.load()
    need = lib.ieee_rank_cuhk03_workspace_bytes(50)
    assert need >= 4 * (3 * 50 + 2)
    d = torch.rand(3, 50, device="cuda")
    i3, i50 = torch.zeros(3, dtype=torch.int32, device="cuda"), torch.zeros(50, dtype=torch.int32, device="cuda")
    cmc, ap = torch.full((3, 5), 7.0, dtype=torch.float64, device="cuda"), torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
    summary = torch.full((7,), 7.0, dtype=torch.float64, device="cuda")
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    P = _lib.ptr

    k50 = torch.ones(50, dtype=torch.int32, device="cuda")           # the query's identity under another key: all kept

    def call(ldd, max_rank, work_bytes):
        return lib.ieee_rank_cuhk03(P(d), ldd, 3, 50, P(i3), P(i50), P(i3), P(k50), max_rank, P(cmc), P(ap), P(summary),
                                    P(work), work_bytes, _lib.stream())
    for bad_rank in (0, -1, 1025):
        assert call(50, bad_rank, need) != 0
    assert call(49, 5, need) != 0                                    # ldd < num_g
    assert call(50, 5, need - 1) != 0                                # workspace too small
    assert b"workspace" in lib.ieee_last_error()
    torch.cuda.synchronize()
    assert bool((cmc == 7.0).all()) and bool((ap == 7.0).all()) and bool((summary == 7.0).all())   # nothing ran
    assert call(50, 5, need) == 0
    torch.cuda.synchronize()
    assert bool((ap == 1.0).all()) and bool((cmc == 1.0).all())      # a gallery of kept true matches only
    assert summary.cpu().tolist() == [3.0] * 5 + [3.0, 3.0]


class TimeDM(object):
    """a synthetic data manager (as VisDM of test_visrank_gpu.py) whose items carry time ids: gallery entries share the
    query's identity and camera under both time ids, so the three-way filter removes fewer entries than a camera filter"""
    num_train_pids = C
    sources = ["synthetic"]
    data_type = "image"
    width, height = 32, 64
    q_pids, q_cams, q_time = np.arange(12) % 6, np.zeros(12, dtype=np.int64), np.arange(12) // 6
    g_pids, g_cams, g_time = np.arange(24) % 6, (np.arange(24) // 6) % 2, (np.arange(24) // 12) % 2

    def __init__(self, zero_time=False):
        self.train_loader = []
        # three of a gallery identity's four images are drawn as another identity's: the true matches are spread over
        # the ranking instead of all on top (mAP 1 whatever is removed)
        drawn_as = (self.g_pids + np.arange(24) // 6) % 6
        query, gallery = id_loader(12, 1, self.q_pids, self.q_cams), id_loader(24, 2, drawn_as, self.g_cams)
        for batches, time, pids in ((query, self.q_time, self.q_pids), (gallery, self.g_time, self.g_pids)):
            for b, batch in enumerate(batches):
                batch["pid"] = torch.as_tensor(pids[4 * b:4 * b + 4])
                batch["timeid"] = torch.as_tensor(0 * time[4 * b:4 * b + 4] if zero_time else time[4 * b:4 * b + 4])
        self.test_loader = {"synthetic": {"query": query, "gallery": gallery}}


def test_engine_passes_the_time_ids_to_the_cuhk03_protocol(tmp_path, capsys):
    from ieee_amd.engine import MultiModalImageSoftmaxEngine
    from ieee_amd.meters import AverageMeter
    from ieee_amd.metrics import compute_distance_matrix, eval_cuhk03
    from ieee_amd.models import build_model
    from ieee_amd.optim import build_optimizer
    m = build_model("ieee3modalPart", num_classes=C, loss="softmax", pretrained=False, compute_dtype=torch.float32)
    dm = TimeDM()
    eng = MultiModalImageSoftmaxEngine(dm, m, build_optimizer(m, optim="sgd", lr=1e-3), use_gpu=True)
    got = eng.test(use_metric_cuhk03=True, ranks=[1, 5])
    report = capsys.readouterr().out
    # the same descriptors, ranked by hand with the items' time ids
    loaders = dm.test_loader["synthetic"]
    qf, q_pids, q_cams = eng._descriptors(loaders["query"], AverageMeter())
    assert np.array_equal(eng._timeids_seen, dm.q_time)
    gf, g_pids, g_cams = eng._descriptors(loaders["gallery"], AverageMeter())
    assert np.array_equal(eng._timeids_seen, dm.g_time)
    distmat = compute_distance_matrix(qf, gf)
    cmc, want = eval_cuhk03(distmat, q_pids, g_pids, q_cams, g_cams, dm.q_time, dm.g_time, 20)
    assert got == want
    assert "mAP: {:.2%}".format(want) in report and "Rank-1  : {:.2%}".format(cmc[0]) in report
    # Engine.run reaches the same call
    eng.run(test_only=True, use_metric_cuhk03=True, ranks=[1, 5], save_dir=str(tmp_path))
    assert "mAP: {:.2%}".format(want) in capsys.readouterr().out
    # with the time ids zeroed the camera filter alone decides, and more entries go: another answer
    zeroed = MultiModalImageSoftmaxEngine(TimeDM(zero_time=True), m, build_optimizer(m, optim="sgd", lr=1e-3), use_gpu=True)
    other = zeroed.test(use_metric_cuhk03=True, ranks=[1, 5])
    assert other == eval_cuhk03(distmat, q_pids, g_pids, q_cams, g_cams, None, None, 20)[1]
    assert other != got
