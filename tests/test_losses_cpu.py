"""CPU: the errors the reference's losses raise for labels they cannot use, raised here on the host before any launch --
a label outside [0, num_classes) (its cross entropy scatters the one-hot on the host, cross_entropy_loss.py:45-46) and
fewer `chunk` pieces than identities (its 3M loop indexes past the tuple, multi_modal_margin_loss_new.py:24-33).
Every path is checked with the device entry point replaced by a tripwire: the point is that no kernel ever sees the batch."""
import pytest
import torch

from ieee_amd import _lib, engine as eng_mod
from ieee_amd.losses import (CrossEntropyLoss, chunks_short_of_identities, multiModalMarginLossNew,
                             target_out_of_range)


class _Launched(Exception):
    pass


@pytest.fixture
def no_launch(monkeypatch):
    def trip(*a, **k):
        raise _Launched("a kernel launch was reached")
    monkeypatch.setattr(_lib, "require_gpu", trip)


def _torch_scatter_error(targets, C):
    """the reference's own failure: torch's scatter_ on the host"""
    with pytest.raises(RuntimeError) as e:
        torch.zeros(len(targets), C).scatter_(1, targets.unsqueeze(1), 1)
    return str(e.value)


@pytest.mark.parametrize("targets", [[0, 171, 3, 4], [5, -1, 0, 2], [200, 0, 0, 170], [0, 1, 2, 1000000]])
def test_cross_entropy_rejects_out_of_range_targets_before_launch(no_launch, targets):
    C = 171
    t = torch.tensor(targets)
    with pytest.raises(RuntimeError) as e:
        CrossEntropyLoss(C)(torch.zeros(len(targets), C), t)
    msg = str(e.value)
    assert "out of bounds for dimension 1 with size 171" in msg
    bad = next(v for v in targets if not 0 <= v < C)
    assert msg.startswith("index %d " % bad)
    assert msg == _torch_scatter_error(t, C)        # the same words as the reference's failure


@pytest.mark.parametrize("targets", [[0], [170], [0, 170, 5, 169]])
def test_cross_entropy_in_range_targets_reach_the_launch(no_launch, targets):
    with pytest.raises(_Launched):
        CrossEntropyLoss(171)(torch.zeros(len(targets), 171), torch.tensor(targets))


def test_target_out_of_range_edges():
    assert target_out_of_range(torch.tensor([0, 1, 2]), 3) is None
    assert target_out_of_range(torch.tensor([], dtype=torch.long), 3) is None
    assert target_out_of_range(torch.tensor([0]), 1) is None
    e = target_out_of_range(torch.tensor([0, 3]), 3)
    assert isinstance(e, RuntimeError) and str(e) == "index 3 is out of bounds for dimension 1 with size 3"
    e = target_out_of_range(torch.tensor([[2, -4], [7, 0]]), 3)          # any shape; the first bad label in order
    assert str(e) == "index -4 is out of bounds for dimension 1 with size 3"


@pytest.mark.parametrize("rows,pids,short", [
    (10, [0, 0, 1, 1, 2, 2, 3, 3, 4, 5], True),       # 6 identities, chunk(6) of 10 rows: 5 pieces of 2
    (10, [0, 0, 0, 1, 1, 1, 2, 2, 2, 3], False),      # 4 identities: chunk(4) -> 4 pieces (3, 3, 3, 1)
    (7, [0, 1, 2, 3, 4, 5, 5], True),                 # 6 identities: pieces of 2 -> 4
    (16, list(range(16)), False),
    (64, [i // 4 for i in range(64)], False),
    (5, [0, 1, 2, 3, 3], True),                       # 4 identities: pieces of 2 -> 3
])
def test_chunks_short_of_identities_matches_torch_chunk(rows, pids, short):
    p = torch.tensor(pids)
    n = len(p.unique())
    want = len(torch.zeros(rows).chunk(n)) < n            # what the reference's loop runs into
    assert chunks_short_of_identities(p) == want == short


def test_margin_loss_short_chunks_raise_index_error_before_launch(no_launch):
    pids = torch.tensor([0, 0, 1, 1, 2, 2, 3, 3, 4, 5])
    f = [torch.zeros(10, 8) for _ in range(3)]
    with pytest.raises(IndexError, match="^tuple index out of range$"):
        multiModalMarginLossNew(margin=1)(f[0], f[1], f[2], pids)
    # the reference fails with the same error
    from oracle import model as om
    with pytest.raises(IndexError, match="tuple index out of range"):
        om.margin3m(f[0], f[1], f[2], pids, 1.0)
    with pytest.raises(_Launched):
        multiModalMarginLossNew(margin=1)(f[0], f[1], f[2], torch.arange(10) // 3)


# ---- the fused engine step: the same checks on the host, before the forward, with the resident-batch shortcut -----------
class _Model(object):
    def __init__(self, C):
        self.num_classes = C


class _DM(object):
    num_train_pids = 9999        # the bound is the classifier's width (the logits the kernel reads), not this


def _guarded(C=171, resident=False):
    e = eng_mod._FusedStepMixin()
    e.model, e.datamanager, e.resident_batch = _Model(C), _DM(), resident
    return e


def test_batch_error_order_and_bound():
    ok = torch.arange(64) // 4
    assert eng_mod.batch_error(ok, 1, 171) is None
    assert eng_mod.batch_error(ok, 0, 16) is None
    assert str(eng_mod.batch_error(ok, 0, 15)) == "index 15 is out of bounds for dimension 1 with size 15"
    short = torch.tensor([0, 0, 1, 1, 2, 2, 3, 3, 4, 5])
    assert isinstance(eng_mod.batch_error(short, 1, 171), IndexError)
    assert eng_mod.batch_error(short, 0, 171) is None        # no 3M loss (weight_m = 0 / the CE-only engine): no chunks
    # both wrong: the reference computes the 3M loss first (margin.py:107-111), so its IndexError wins
    both = torch.tensor([0, 0, 1, 1, 2, 2, 3, 3, 4, 500])
    assert isinstance(eng_mod.batch_error(both, 1, 171), IndexError)
    assert isinstance(eng_mod.batch_error(both, 0, 171), RuntimeError)


def test_guard_batch_uses_the_classifier_width_and_caches_only_resident_batches(monkeypatch):
    bad = torch.tensor([0, 1, 2, 171])
    with pytest.raises(RuntimeError, match="index 171 is out of bounds for dimension 1 with size 171"):
        _guarded(171)._guard_batch(bad, 0)
    _guarded(172)._guard_batch(bad, 0)                          # in range for a wider classifier
    calls = []
    real = eng_mod.batch_error
    monkeypatch.setattr(eng_mod, "batch_error", lambda *a: calls.append(1) or real(*a))
    # a resident batch (bench.py: the same tensor every step) is checked once; its answer is kept, errors included
    e = _guarded(171, resident=True)
    for _ in range(3):
        with pytest.raises(RuntimeError):
            e._guard_batch(bad, 1)
    assert len(calls) == 1
    good = torch.arange(8) // 2
    for _ in range(3):
        e._guard_batch(good, 1)
    assert len(calls) == 2
    # any other batch is checked every time: a DataLoader may hand out the same storage with new labels
    e = _guarded(171)
    for _ in range(2):
        e._guard_batch(good, 1)
    good[6:] = 171
    with pytest.raises(RuntimeError):
        e._guard_batch(good, 1)
    assert len(calls) == 5


@pytest.mark.parametrize("cls,kw,pids,exc", [
    ("Image3MEngine", dict(margin=1), [0, 0, 1, 1, 2, 2, 3, 3, 4, 5], IndexError),
    ("Image3MEngine", dict(margin=1), [0, 0, 1, 1, 2, 2, 3, 3, 171, 171], RuntimeError),
    ("Image3MEngine", dict(margin=1, weight_m=0), [0, 0, 1, 1, 2, 2, 3, 3, 4, 171], RuntimeError),
    ("MultiModalImageSoftmaxEngine", {}, [0, 0, 1, 1, 2, 2, 3, 3, 4, 171], RuntimeError),
    ("MultiModalImageSoftmaxEngine", {}, [0, -2, 1, 1], RuntimeError),
])
def test_engine_step_raises_before_moving_the_batch(no_launch, monkeypatch, cls, kw, pids, exc):
    class DM(object):
        num_train_pids = 171
        train_loader = []
        test_loader = {}
        sources = ["synthetic"]

    class Net(torch.nn.Module):
        num_classes = 171

    def to_device(*a, **k):
        raise _Launched("the batch reached the device")
    E = getattr(eng_mod, cls)
    e = E(DM(), Net(), None, use_gpu=False, **kw)
    monkeypatch.setattr(e, "_to_device", to_device)
    p = torch.tensor(pids)
    data = {"img": [torch.zeros(len(pids), 3, 4, 2)] * 3, "pid": p, "camid": p, "impath": "", "timeid": p}
    with pytest.raises(exc):
        e.forward_backward(data)
    p[:] = torch.arange(len(pids)) // 2 % 4        # a batch it can train on gets as far as the device
    with pytest.raises(_Launched):
        e.forward_backward(data)
