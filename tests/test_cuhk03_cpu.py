"""CPU: tests/util_cuhk03.py -- the float64 restatement the device evaluator (ieee_rank_cuhk03) is tested against --
is itself checked three ways: against the protocol with every joint draw enumerated, against 1 000 seeded runs of the
reference's eval_cuhk03 (tests/golden/cuhk03_golden.npz, gen_cuhk03_golden.py), and by showing that three plausible
wrong restatements leave the brute-force bound.  No GPU."""
import os

import numpy as np
import pytest

from tests.util_cuhk03 import brute_force, cuhk03_reference

MAX_RANK = 5


def small_case():
    """4 gallery identities (0..3) with 4, 3, 2 and 4 images (product 96 at most), two cameras, two time ids; integer
    distances, so true matches tie with other identities' images on both sides of the gallery index"""
    g_pids = np.array([0, 1, 0, 2, 1, 0, 3, 1, 2, 3, 0, 3, 3])
    g_cams = np.array([0, 0, 1, 0, 1, 0, 0, 0, 1, 1, 0, 0, 1])
    g_time = np.array([0, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 1, 0])
    #                 query 0: pid 0, cam 0, time 0 -> gallery 0 and 10 removed, 2 and 5 kept (5: same camera, other time)
    #                 query 1: pid 1, cam 1, time 0 -> 4 removed, 1 and 7 kept
    #                 query 2: pid 2, cam 0, time 1 -> 3 removed, 8 kept
    #                 query 3: pid 7: not in the gallery -> skipped
    #                 query 4: pid 2, cam 1, time 0 and query 5: the same -> 8 removed, 3 kept
    #                 query 6: pid 3, cam 1, time 1 -> nothing removed, four true matches
    q_pids = np.array([0, 1, 2, 7, 2, 2, 3])
    q_cams = np.array([0, 1, 0, 0, 1, 1, 1])
    q_time = np.array([0, 0, 1, 0, 0, 0, 1])
    rng = np.random.RandomState(5)
    d = rng.randint(0, 4, size=(len(q_pids), len(g_pids))).astype(np.float32)
    # a true match of query 0 (gallery 2) ties with an other-identity image after it (gallery 3) and before it (1)
    d[0, [1, 2, 3]] = 2.0
    # query 2: its only kept true match ties with a later image of another identity; its removed entry comes first
    d[2, 3], d[2, 8], d[2, 9] = 0.0, 1.0, 1.0
    # a query whose every same-identity entry is removed: pid 2 with the key of gallery 3 AND of gallery 8 cannot be,
    # so a second skipped query is made from pid 1 below
    return d, q_pids, g_pids, q_cams, g_cams, q_time, g_time


@pytest.fixture(scope="module")
def case():
    return small_case()


@pytest.fixture(scope="module")
def exact(case):
    return brute_force(*case, MAX_RANK)


def worst(got, exact_cmc, valid):
    return float(np.abs(got["cmc"][valid] - exact_cmc[valid]).max())


def test_restatement_equals_the_enumerated_protocol(case, exact):
    exact_cmc, valid = exact
    got = cuhk03_reference(*case, MAX_RANK)
    assert valid.tolist() == [True, True, True, False, True, True, True]
    assert np.array_equal(got["valid"], valid)
    assert got["n_true"].tolist() == [2, 2, 1, 0, 1, 1, 4]            # two true matches, none, several
    assert worst(got, exact_cmc, valid) <= 1e-12
    assert np.all(got["cmc"][~valid] == 0) and np.all(got["ap"][~valid] == -1)
    # the curves rise to at most 1, and are not trivially flat
    assert np.all(np.diff(got["cmc"][valid], axis=1) >= -1e-15) and got["cmc"].max() <= 1 + 1e-15
    assert 0 < got["cmc"][valid][:, 0].min() < 1


def test_a_query_with_every_same_identity_entry_removed_is_skipped():
    d, q_pids, g_pids, q_cams, g_cams, q_time, g_time = small_case()
    # identity 2 has gallery 3 (cam 0, time 1) and 8 (cam 1, time 0): give both the query's key
    g_cams, g_time = g_cams.copy(), g_time.copy()
    g_cams[[3, 8]], g_time[[3, 8]] = 1, 0
    got = cuhk03_reference(d, q_pids, g_pids, q_cams, g_cams, q_time, g_time, MAX_RANK)
    exact_cmc, valid = brute_force(d, q_pids, g_pids, q_cams, g_cams, q_time, g_time, MAX_RANK)
    assert not valid[4] and not valid[5] and valid[2]
    assert np.array_equal(got["valid"], valid) and worst(got, exact_cmc, valid) <= 1e-12


def test_fewer_identities_than_max_rank_gives_a_tail_of_ones(case):
    got = cuhk03_reference(*case, 9)
    exact_cmc, valid = brute_force(*case, 9)
    assert worst(got, exact_cmc, valid) <= 1e-12
    assert np.allclose(got["cmc"][valid][:, 3:], 1.0, rtol=0, atol=1e-12)   # 4 identities: ranks 0..3
    # a curve for a smaller max_rank is a prefix of the longer one
    assert np.array_equal(cuhk03_reference(*case, MAX_RANK)["cmc"], got["cmc"][:, :MAX_RANK])


def test_totals_are_formed_like_the_market_evaluator(case):
    got = cuhk03_reference(*case, MAX_RANK)
    nv = got["num_valid"]
    assert nv == 6 and got["all_cmc"].dtype == np.float32
    assert np.array_equal(got["all_cmc"], (got["cmc"][got["valid"]].sum(0) / nv).astype(np.float32))
    assert got["mAP"] == pytest.approx(got["ap"][got["valid"]].mean(), rel=1e-15)


def test_null_time_ids_mean_all_equal(case):
    d, q_pids, g_pids, q_cams, g_cams, q_time, g_time = case
    a = cuhk03_reference(d, q_pids, g_pids, q_cams, g_cams, None, None, MAX_RANK)
    b = cuhk03_reference(d, q_pids, g_pids, q_cams, g_cams, 0 * q_time, 0 * g_time, MAX_RANK)
    assert np.array_equal(a["cmc"], b["cmc"]) and np.array_equal(a["ap"], b["ap"])


@pytest.mark.parametrize("variant", ["camera_only", "ties_le", "all_true"])
def test_wrong_restatements_leave_the_bound(case, exact, variant):
    """the brute-force check has teeth: a filter on identity and camera only, c_j counted with <= on ties, and an
    average over all true matches (removed ones included) are each far outside 1e-12"""
    exact_cmc, valid = exact
    got = cuhk03_reference(*case, MAX_RANK, variant=variant)
    both = valid & got["valid"]
    assert not np.array_equal(got["valid"], valid) or worst(got, exact_cmc, both) > 1e-3


# ---- the reference itself, sampled ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cuhk03_golden.npz"))


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_within_5_standard_errors_of_the_reference(golden, name):
    """the golden is one draw of 1 000 seeded reference runs per fixture; 5 standard errors make an unlucky draw a
    less-than-1e-5 event over all 15 ranks, so a miss means the formula is wrong"""
    g = {k[2:]: golden[k] for k in golden.files if k.startswith(name + "_")}
    R = int(g["max_rank"])
    got = cuhk03_reference(g["distmat"], g["q_pids"], g["g_pids"], g["q_camids"], g["g_camids"], g["q_timeids"],
                           g["g_timeids"], R)
    assert got["num_valid"] > 0 and np.all(g["cmc_sem"] > 0)
    mine = got["cmc"][got["valid"]].sum(0) / got["num_valid"]
    z = np.abs(mine - g["cmc_mean"]) / g["cmc_sem"]
    print(name, "z-scores", z)
    assert np.all(z <= 5.0), z
    assert abs(got["mAP"] - float(g["mAP"])) <= 1e-12 * abs(float(g["mAP"]))


def test_golden_fixtures_are_what_the_issue_asks(golden):
    assert golden["a_distmat"].shape == (12, 90) and int(golden["a_max_rank"]) == 5
    assert golden["b_distmat"].shape == (20, 300) and int(golden["b_max_rank"]) == 10
    assert len(np.unique(golden["a_g_pids"])) == 15 and len(np.unique(golden["b_g_pids"])) == 40
    for n in "ab":
        d = golden[n + "_distmat"]
        assert all(len(np.unique(r)) == d.shape[1] for r in d)           # distinct distances
    assert golden["b_regdb_cmc"].dtype == np.float32 and golden["b_regdb_cmc"].shape == (20,)
