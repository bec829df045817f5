"""CPU: the parts of ranked retrieval that never reach the device -- rank_topk's argument checks (raised before the
library or a GPU is asked for) and how Engine finds the records it draws (fetch_test_loaders, else the loaders'
datasets), and the refusal of visrank in a sharded evaluation."""
import numpy as np
import pytest


class _DM(object):
    train_loader = []
    test_loader = {}
    sources = []


class _Loader(list):
    class dataset(object):
        data = None


def _engine(dm):
    from ieee_amd.engine import Engine
    return Engine(dm, use_gpu=False)


@pytest.mark.parametrize("k", [0, -3, 1025, 2.5, True, None])
def test_rank_topk_rejects_k(k):
    from ieee_amd.metrics import rank_topk
    with pytest.raises((ValueError, TypeError)):
        rank_topk(np.zeros((2, 5), dtype=np.float32), k)


def test_rank_topk_needs_all_four_labels_or_none():
    from ieee_amd.metrics import rank_topk
    d = np.zeros((2, 5), dtype=np.float32)
    with pytest.raises(ValueError):
        rank_topk(d, 3, np.zeros(2))
    with pytest.raises(ValueError):
        rank_topk(d, 3, np.zeros(2), np.zeros(5), np.zeros(2), None)
    with pytest.raises(ValueError):
        rank_topk(np.zeros(5, dtype=np.float32), 3)


def test_records_from_fetch_test_loaders():
    class DM(_DM):
        def fetch_test_loaders(self, name):
            return ["q-" + name], ["g-" + name]
    assert _engine(DM())._test_records("market", None, None) == (["q-market"], ["g-market"])


def test_records_from_the_loaders_datasets():
    q, g = _Loader(), _Loader()
    q.dataset, g.dataset = type("D", (), {"data": [1, 2]})(), type("D", (), {"data": [3]})()
    assert _engine(_DM())._test_records("x", q, g) == ([1, 2], [3])


def test_records_missing_is_a_clear_error():
    with pytest.raises(ValueError, match="fetch_test_loaders"):
        _engine(_DM())._test_records("x", [], [])


def test_visrank_refused_when_sharded(monkeypatch):
    from ieee_amd import dist as ddp
    monkeypatch.setattr(ddp, "world_size", lambda: 2)
    with pytest.raises(RuntimeError, match="one GPU"):
        _engine(_DM())._evaluate(dataset_name="x", visrank=True)
