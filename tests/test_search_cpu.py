"""CPU: the parts of the streamed gallery search that never reach the device -- default_slab_rows, the argument checks
of TopKAccumulator and search_topk (ValueError before the library or a GPU is asked for), and visualize_ranked_results
drawing a ranking that exists already (indices=...), which never calls rank_topk."""
import os

import numpy as np
import pytest
import torch


def test_default_slab_rows():
    from ieee_amd.metrics import default_slab_rows
    from ieee_amd.metrics import search as S
    assert S.TOPK_CHUNK == 2048 and S.SLAB_BUDGET_BYTES % (4 * S.TOPK_CHUNK) == 0
    last = None
    for num_q in list(range(1, 70)) + [100, 255, 256, 1000, 4096, 10000, 16383, 16384, 16385, 10 ** 5, 10 ** 6, 10 ** 9]:
        rows = default_slab_rows(num_q)
        assert rows % S.TOPK_CHUNK == 0 and rows >= S.TOPK_CHUNK
        assert last is None or rows <= last
        if rows > S.TOPK_CHUNK:
            assert num_q * rows * 4 <= S.SLAB_BUDGET_BYTES
            assert num_q * (rows + S.TOPK_CHUNK) * 4 > S.SLAB_BUDGET_BYTES      # the largest such multiple
        last = rows
    assert default_slab_rows(10000) == S.SLAB_BUDGET_BYTES // 40000 // 2048 * 2048
    assert default_slab_rows(0) == default_slab_rows(1) == S.SLAB_BUDGET_BYTES // 4


@pytest.mark.parametrize("k", [0, -3, 1025, 2.5, True])
def test_k_is_checked_first(k):
    from ieee_amd.metrics import TopKAccumulator, search_topk
    with pytest.raises(ValueError):
        TopKAccumulator(4, k)
    with pytest.raises(ValueError):
        search_topk(torch.zeros(4, 8), torch.zeros(9, 8), k)


def test_accumulator_argument_errors():
    from ieee_amd.metrics import TopKAccumulator
    z4 = np.zeros(4)
    for bad in [dict(q_pids=z4), dict(q_camids=z4), dict(q_pids=z4, q_camids=np.zeros(5)),
                dict(q_pids=np.zeros(3), q_camids=z4), dict(q_pids=z4 + 2.0 ** 40, q_camids=z4), dict(device="cpu")]:
        with pytest.raises(ValueError):
            TopKAccumulator(4, 5, **bad)
    for num_q in (-1, 2.5, True):
        with pytest.raises(ValueError):
            TopKAccumulator(num_q, 5)


def test_search_argument_errors():
    from ieee_amd.metrics import search_topk
    q, g = torch.zeros(4, 8), torch.zeros(9, 8)
    z4, z9 = np.zeros(4), np.zeros(9)
    full = dict(q_pids=z4, g_pids=z9, q_camids=z4, g_camids=z9)
    bad_calls = [
        dict(metric="manhattan"), dict(precision="fp8"), dict(slab=0), dict(slab=-5), dict(slab=2.5), dict(slab=True),
        dict(q_pids=z4), dict(q_pids=z4, g_pids=z9, q_camids=z4),                          # all four labels or none
        dict(full, g_pids=np.zeros(8)), dict(full, g_camids=np.zeros(10)),                 # gallery labels: 9 rows
        dict(full, g_pids=np.zeros(10), g_camids=np.zeros(10)),
        dict(full, q_pids=np.zeros(5)), dict(full, q_camids=np.zeros(3)),
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            search_topk(q, g, 3, **kw)
    for gallery in (torch.zeros(9, 7), torch.zeros(9), [g, torch.zeros(2, 7)], [g, np.zeros((2, 8))], "gallery", 5):
        with pytest.raises(ValueError):
            search_topk(q, gallery, 3)
    for query in (torch.zeros(8), np.zeros((4, 8))):
        with pytest.raises(ValueError):
            search_topk(query, g, 3)
    with pytest.raises(ValueError):                                                        # a list's length is known too
        search_topk(q, [g[:4], g[4:4], g[4:]], 3, **dict(full, g_pids=np.zeros(8), g_camids=np.zeros(8)))


def _dataset(tmp_path, num_q, num_g):
    from PIL import Image
    rng = np.random.RandomState(0)

    def rec(name, pid, cam):
        path = str(tmp_path / (name + ".png"))
        Image.fromarray(rng.randint(0, 255, size=(12, 6, 3)).astype(np.uint8)).save(path)
        return (path, pid, cam)
    return ([rec("q%d" % i, i % 2, 0) for i in range(num_q)], [rec("g%d" % i, i % 2, 1) for i in range(num_g)])


def test_visualize_a_ranking_that_exists_already(tmp_path, monkeypatch):
    from PIL import Image
    from ieee_amd import reidtools
    from ieee_amd.metrics import topk as topk_mod

    def never(*a, **k):
        raise AssertionError("rank_topk must not be called when indices are given")
    monkeypatch.setattr(topk_mod, "rank_topk", never)
    dataset = _dataset(tmp_path, 3, 5)
    indices = np.array([[4, 0, 2, -1], [1, -1, -1, -1], [-1, -1, -1, -1]])
    out = str(tmp_path / "ranked")
    rows = reidtools.visualize_ranked_results(None, dataset, width=6, height=12, save_dir=out, topk=3, indices=indices)
    assert rows == [[4, 0, 2], [1], []]                                   # the first topk columns, -1 entries skipped
    assert sorted(os.listdir(out)) == ["q0.jpg", "q1.jpg", "q2.jpg"]
    w = 4 * 6 + 3 * reidtools.GRID_SPACING + reidtools.QUERY_EXTRA_SPACING
    for i in range(3):
        img = np.asarray(Image.open(os.path.join(out, "q%d.jpg" % i)))
        assert img.shape == (12, w, 3)
        first_tile = img[:, 6 + reidtools.GRID_SPACING + reidtools.QUERY_EXTRA_SPACING:][:, :6]
        assert (first_tile.min() > 200) == (i == 2)                       # white where nothing was drawn
    same = reidtools.visualize_ranked_results(None, dataset, width=6, height=12, save_dir=out, topk=4,
                                              indices=torch.from_numpy(indices))
    assert same == [[4, 0, 2], [1], []]


def test_visualize_wants_exactly_one_of_distmat_and_indices(tmp_path):
    from ieee_amd import reidtools
    dataset = _dataset(tmp_path, 2, 3)
    idx = np.zeros((2, 2), dtype=np.int64)
    with pytest.raises(ValueError):
        reidtools.visualize_ranked_results(np.zeros((2, 3), dtype=np.float32), dataset, save_dir=str(tmp_path), indices=idx)
    with pytest.raises(ValueError):
        reidtools.visualize_ranked_results(None, dataset, save_dir=str(tmp_path))
    for bad in (np.zeros((3, 2), dtype=np.int64), np.full((2, 2), 3), np.full((2, 2), -2), np.zeros((2, 2))):
        with pytest.raises(ValueError):
            reidtools.visualize_ranked_results(None, dataset, save_dir=str(tmp_path), indices=bad)
