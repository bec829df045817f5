"""CPU: staged learning rates (torchreid/optim/optimizer.py:78-108) over the flat-buffer model -- the reference's two
parameter groups, their launch ranges as a partition of the model's runs, schedulers, checkpoint interop with the
torch.optim / reference-layout optimizers for all four fused classes -- and the float64 restatement of the reference's own
RAdam held to a recording of that class (tests/golden/optim_golden.npz)."""
import os

import numpy as np
import pytest
import torch

from ieee_amd.models import build_model
from ieee_amd.optim import (FusedAdam, FusedRAdam, FusedRMSprop, FusedSGD, build_lr_scheduler, build_optimizer)
from tests.util_optim import RAdamF64, U, radam_schedule, reference_groups

C = 171
HEADS = ["fc_R", "fc_T", "fc_N", "classifier_R", "classifier_N", "classifier_T"]
FUSED = {"sgd": FusedSGD, "adam": FusedAdam, "amsgrad": FusedAdam, "rmsprop": FusedRMSprop, "radam": FusedRAdam}
TORCH = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "amsgrad": torch.optim.Adam, "rmsprop": torch.optim.RMSprop,
         "radam": torch.optim.RAdam}


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return build_model("ieee3modalPart", num_classes=C, loss="margin", pretrained=False, device="cpu",
                       compute_dtype=torch.float32)


def _same(params, want):
    return len(params) == len(want) and all(a is b for a, b in zip(params, want))


def merged(runs):
    out = []
    for a, b in sorted(runs):
        if out and out[-1][1] == a:
            out[-1] = (out[-1][0], b)
        else:
            out.append((a, b))
    return out


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("optim", ["sgd", "adam", "amsgrad", "rmsprop", "radam"])
def test_staged_lr_builds_the_reference_groups(model, optim):
    lr = 0.01
    want = reference_groups(model, HEADS, lr, 0.1)
    assert len(want[1]["params"]) == sum(len(list(getattr(model, n).parameters())) for n in HEADS) > 0
    opt = build_optimizer(model, optim, lr=lr, staged_lr=True, new_layers=HEADS, base_lr_mult=0.1)
    assert type(opt) is FUSED[optim]
    assert len(opt.param_groups) == 2
    assert _same(opt.param_groups[0]["params"], want[0]["params"]) and _same(opt.param_groups[1]["params"], want[1]["params"])
    assert opt.param_groups[0]["lr"] == lr * 0.1 and opt.param_groups[1]["lr"] == lr
    # the unfused object: the same torch.optim type as without staged_lr, over the same two groups
    plain = build_optimizer(model, optim, lr=lr, staged_lr=True, new_layers=HEADS, base_lr_mult=0.1, fused=False)
    assert type(plain) is TORCH[optim] and type(build_optimizer(model, optim, lr=lr, fused=False)) is TORCH[optim]
    assert _same(plain.param_groups[0]["params"], want[0]["params"]) and _same(plain.param_groups[1]["params"], want[1]["params"])
    assert plain.param_groups[0]["lr"] == lr * 0.1 and plain.param_groups[1]["lr"] == lr
    # ungrouped: one group over model.parameters(), as before
    flat = build_optimizer(model, optim, lr=lr)
    assert type(flat) is FUSED[optim] and len(flat.param_groups) == 1
    assert _same(flat.param_groups[0]["params"], list(model.parameters()))


def test_staged_lr_string_dataparallel_and_names_that_select_nothing(model):
    """a str is one name; a DataParallel wrapper is unwrapped; '' (the default) and a name that is no child leave the new
    group EMPTY -- which is what the reference's own call does on this torch: torch.optim accepts an empty group
    (checked here with torch.optim.SGD over the reference's groups) and everything trains at lr * base_lr_mult"""
    opt = build_optimizer(model, "sgd", lr=0.01, staged_lr=True, new_layers="fc_R")
    assert _same(opt.param_groups[1]["params"], list(model.fc_R.parameters()))
    wrapped = torch.nn.DataParallel(model)
    assert _same(build_optimizer(wrapped, "adam", lr=0.01, staged_lr=True, new_layers=HEADS).param_groups[1]["params"],
                 reference_groups(model, HEADS, 0.01, 0.1)[1]["params"])
    for names in ("", ["no_such_child"]):
        groups = reference_groups(model, names, 0.01, 0.1)
        ref = torch.optim.SGD(groups, lr=0.01, momentum=0.9, weight_decay=5e-4, dampening=0, nesterov=True)
        assert [len(g["params"]) for g in ref.param_groups] == [len(list(model.parameters())), 0]
        opt = build_optimizer(model, "sgd", lr=0.01, staged_lr=True, new_layers=names)
        assert [len(g["params"]) for g in opt.param_groups] == [len(g["params"]) for g in ref.param_groups]
        assert _same(opt.param_groups[0]["params"], ref.param_groups[0]["params"])
        assert opt.param_groups[0]["lr"] == ref.param_groups[0]["lr"] == 0.01 * 0.1
        assert all(gi == 0 for gi, _, _ in opt.launch_ranges())
        assert merged((a, b) for _, a, b in opt.launch_ranges()) == merged(model.trainable_runs())
        assert len(opt.state_dict()["param_groups"][1]["params"]) == 0
    # every child new: the base group is the empty one
    every = [n for n, _ in model.named_children()]
    opt = build_optimizer(model, "sgd", lr=0.01, staged_lr=True, new_layers=every)
    assert [len(g["params"]) for g in opt.param_groups] == [0, len(list(model.parameters()))]
    assert all(gi == 1 for gi, _, _ in opt.launch_ranges())


# ---------------------------------------------------------------------------------------------------------------- 2
def test_children_are_contiguous_spans_of_the_flat_buffer(model):
    opt = build_optimizer(model, "sgd", lr=0.01, staged_lr=True, new_layers=HEADS)
    first = {}
    for name, p in model._param_items:
        first.setdefault(name.split(".")[0], model._offsets[name])
    assert first["backbone"] == 0 and first["convOne"] == 70524096
    assert [n for n, _ in model.named_children()][-6:] == HEADS
    assert model._flat_params.numel() == 109499337
    spans = opt.group_spans()
    assert spans[1] == [(first["fc_R"], 109499337)] and spans[0] == [(0, first["fc_R"])]


def _check_partition(model, opt):
    spans = opt.group_spans()

    def inside_one_group(gi, a, b):
        return any(c <= a and b <= d for c, d in spans[gi])
    whole = opt.launch_ranges()
    assert merged((a, b) for _, a, b in whole) == merged(model.trainable_runs())
    assert sum(b - a for _, a, b in whole) == sum(b - a for a, b in model.trainable_runs())          # pairwise disjoint
    assert all(a < b and inside_one_group(gi, a, b) for gi, a, b in whole)
    for (g0, _, b0), (g1, a1, _) in zip(whole, whole[1:]):
        assert not (g0 == g1 and b0 == a1), "adjacent ranges of one group are one launch"
    parts = model.part_runs()
    seen = []
    for p in range(len(parts)):
        mine = opt.launch_ranges(p)
        assert merged((a, b) for _, a, b in mine) == merged(parts[p])
        assert sum(b - a for _, a, b in mine) == sum(b - a for a, b in parts[p])
        assert all(a < b and inside_one_group(gi, a, b) for gi, a, b in mine)
        seen += [(a, b) for _, a, b in mine]
    assert merged(seen) == merged(model.trainable_runs())
    # the group of every element, by either route, is the group its parameter is in
    owner = torch.full((model._flat_params.numel(),), -1, dtype=torch.int8)
    for gi, a, b in whole:
        owner[a:b] = gi
    by_part = torch.full_like(owner, -1)
    for p in range(len(parts)):
        for gi, a, b in opt.launch_ranges(p):
            assert bool((by_part[a:b] == -1).all())
            by_part[a:b] = gi
    assert torch.equal(owner, by_part)
    where = {id(p): model._offsets[n] for n, p in model._param_items}
    trainable = torch.zeros_like(owner, dtype=torch.bool)
    for a, b in model.trainable_runs():
        trainable[a:b] = True
    for gi, g in enumerate(opt.param_groups):
        for p in g["params"]:
            sl = slice(where[id(p)], where[id(p)] + p.numel())
            assert bool((owner[sl][trainable[sl]] == gi).all())


@pytest.mark.parametrize("new_layers", [HEADS, ["backbone"], ["convOne", "REM", "classifier_N"], "reduce_layer",
                                        ["CA", "fc_T", "backbone"]])
def test_launch_ranges_partition_the_models_runs(new_layers):
    torch.manual_seed(0)
    m = build_model("ieee3modalPart", num_classes=C, loss="margin", pretrained=False, device="cpu", compute_dtype=torch.float32)
    known = set(n for n, _ in m.named_children())
    assert set([new_layers] if isinstance(new_layers, str) else new_layers) <= known
    opt = build_optimizer(m, "sgd", lr=0.01, staged_lr=True, new_layers=new_layers)
    _check_partition(m, opt)
    # backbone frozen (fixbase / open_layers): the cache follows requires_grad
    for p in m.backbone.parameters():
        p.requires_grad = False
    assert all(a >= 70524096 for _, a, _ in opt.launch_ranges())
    _check_partition(m, opt)
    for p in m.parameters():
        p.requires_grad = True
    _check_partition(m, opt)
    # ablation flags off: whole branches receive no gradient
    for flags in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        m.interaction, m.attention, m.using_REM = flags
        _check_partition(m, opt)


def test_ungrouped_optimizers_launch_exactly_the_models_runs(model):
    for optim in ("sgd", "adam", "rmsprop", "radam"):
        opt = build_optimizer(model, optim, lr=0.01)
        assert opt.launch_ranges() == [(0, a, b) for a, b in model.trainable_runs()]
        for p, runs in enumerate(model.part_runs()):
            assert opt.launch_ranges(p) == [(0, a, b) for a, b in runs]


def test_launch_counts(model):
    """recorded in LABNOTES.md: launches per optimizer step, ungrouped and with the six head children as new layers"""
    flat = build_optimizer(model, "sgd", lr=0.01)
    grouped = build_optimizer(model, "sgd", lr=0.01, staged_lr=True, new_layers=HEADS)
    n_flat, n_grouped = len(flat.launch_ranges()), len(grouped.launch_ranges())
    print("launches per step(): ungrouped %d, grouped %d; by part: ungrouped %s, grouped %s" % (
        n_flat, n_grouped, [len(flat.launch_ranges(p)) for p in range(5)], [len(grouped.launch_ranges(p)) for p in range(5)]))
    # two groups, each one span of the flat buffer: the single boundary between them cuts at most one run in two
    assert n_flat <= n_grouped <= n_flat + 1
    by_part = [sum(len(o.launch_ranges(p)) for p in range(5)) for o in (flat, grouped)]
    assert by_part[0] <= by_part[1] <= by_part[0] + 1


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("optim", ["sgd", "adam", "rmsprop", "radam"])
def test_multi_step_schedule_scales_both_groups(model, optim):
    import warnings
    lr = 0.01
    opt = build_optimizer(model, optim, lr=lr, staged_lr=True, new_layers=HEADS, base_lr_mult=0.1)
    sched = build_lr_scheduler(opt, "multi_step", stepsize=[2, 4], gamma=0.1)
    seen = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (no optimizer.step() before the scheduler's: no GPU here)
        for epoch in range(5):
            seen.append((opt.param_groups[0]["lr"], opt.param_groups[1]["lr"]))
            sched.step()
    want = [(lr * 0.1 * f, lr * f) for f in (1, 1, 0.1, 0.1, 0.01)]
    for got, exp in zip(seen, want):
        assert got == pytest.approx(exp, rel=1e-12)


# ---------------------------------------------------------------------------------------------------------------- 4
def _load_reference_radam():
    """the class the reference builds for optim='radam' when its tree is here; else a stand-in with the same state layout
    (per-parameter step: int, exp_avg, exp_avg_sq; defaults lr / betas / eps / weight_decay) -- state_dict() and
    load_state_dict() are torch.optim.Optimizer's in both"""
    from oracle import ref_import
    if ref_import.available():
        ref_import.import_reference()
        from torchreid.optim.radam import RAdam
        return RAdam

    class RAdamLayout(torch.optim.Optimizer):
        def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
            super(RAdamLayout, self).__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
    return RAdamLayout


def _pattern(lo, hi, k, sign=1.0):
    """a value per flat element that names its position (exact in fp32) and its state key"""
    return ((torch.arange(lo, hi) % 4099).to(torch.float32) * 0.25 + k + 1) * sign


_STATE = {"sgd": ("momentum_buffer",), "adam": ("exp_avg", "exp_avg_sq"), "rmsprop": ("square_avg", "momentum_buffer"),
          "radam": ("exp_avg", "exp_avg_sq")}


def _torch_side(optim, params, lr):
    if optim == "sgd":
        return torch.optim.SGD(params, lr=lr, momentum=0.9, weight_decay=5e-4, dampening=0, nesterov=True)
    if optim == "adam":
        return torch.optim.Adam(params, lr=lr, weight_decay=5e-4, betas=(0.9, 0.99))
    if optim == "rmsprop":
        return torch.optim.RMSprop(params, lr=lr, momentum=0.9, weight_decay=5e-4, alpha=0.99)
    return _load_reference_radam()(params, lr=lr, weight_decay=5e-4, betas=(0.9, 0.99))


@pytest.mark.parametrize("grouped", [False, True], ids=["ungrouped", "grouped"])
@pytest.mark.parametrize("optim", ["sgd", "adam", "rmsprop", "radam"])
def test_checkpoints_interoperate_with_the_torch_layout(model, optim, grouped, tmp_path):
    lr = 0.01
    keys = _STATE[optim]
    has_step = optim != "sgd"
    kw = dict(staged_lr=True, new_layers=HEADS, base_lr_mult=0.1) if grouped else {}

    def torch_params():
        return reference_groups(model, HEADS, lr, 0.1) if grouped else list(model.parameters())
    where = {id(p): (model._offsets[n], p.numel()) for n, p in model._param_items}
    N = model._flat_params.numel()
    # ---- torch / reference layout -> fused
    t = _torch_side(optim, torch_params(), lr)
    for gi, g in enumerate(t.param_groups):
        g["lr"] = 0.5 ** (gi + 3)                         # what a scheduler left there
        for p in g["params"]:
            off, n = where[id(p)]
            for k, key in enumerate(keys):
                t.state[p][key] = _pattern(off, off + n, k).view(p.shape)
            if has_step:
                t.state[p]["step"] = 9 if optim == "radam" else torch.tensor(9.0)
    torch.save({"optimizer": t.state_dict()}, str(tmp_path / "t.pt"))
    f = build_optimizer(model, optim, lr=lr, **kw)
    f.load_state_dict(torch.load(str(tmp_path / "t.pt"), weights_only=False)["optimizer"])
    flats = f.flat_state()
    assert len(flats) == len(keys)
    for k, flat in enumerate(flats):
        assert torch.equal(flat, _pattern(0, N, k)), keys[k]
    assert [g["lr"] for g in f.param_groups] == [0.5 ** (gi + 3) for gi in range(len(f.param_groups))]
    if has_step:
        assert f._step == 9
    # ---- fused -> torch / reference layout (through a file, as resume_from_checkpoint does)
    f2 = build_optimizer(model, optim, lr=lr, **kw)
    flats = f2.flat_state()
    with torch.no_grad():
        for k, flat in enumerate(flats):
            flat.copy_(_pattern(0, N, k, -1.0))
    f2._step = 13
    for gi, g in enumerate(f2.param_groups):
        g["lr"] = 0.25 ** (gi + 1)
    sd = f2.state_dict()
    # torch numbers parameters in group order: base first, then new
    ids = [i for g in sd["param_groups"] for i in g["params"]]
    assert ids == list(range(len(list(model.parameters()))))
    torch.save({"optimizer": sd}, str(tmp_path / "f.pt"))
    t2 = _torch_side(optim, torch_params(), lr)
    t2.load_state_dict(torch.load(str(tmp_path / "f.pt"), weights_only=False)["optimizer"])
    assert [g["lr"] for g in t2.param_groups] == [0.25 ** (gi + 1) for gi in range(len(t2.param_groups))]
    for g in t2.param_groups:
        for p in g["params"]:
            off, n = where[id(p)]
            st = t2.state[p]
            for k, key in enumerate(keys):
                assert torch.equal(st[key].flatten(), _pattern(off, off + n, k, -1.0)), key
            if has_step:
                assert float(st["step"]) == 13
                assert isinstance(st["step"], int) == (optim == "radam")
    # the state the fused object publishes is views of its flat buffers (a file stores each buffer once)
    p = f2.param_groups[-1]["params"][0]
    assert f2.state[p][keys[0]].data_ptr() == flats[0].data_ptr() + 4 * where[id(p)][0]
    # and a fused file loads into a fresh fused object
    f3 = build_optimizer(model, optim, lr=lr, **kw)
    f3.load_state_dict(sd)
    assert all(torch.equal(a, b) for a, b in zip(f3.flat_state(), flats))
    assert [g["lr"] for g in f3.param_groups] == [g["lr"] for g in f2.param_groups]
    if has_step:
        assert f3._step == 13


def test_a_grouped_file_does_not_load_into_an_ungrouped_optimizer(model):
    """torch's own rule (Optimizer.load_state_dict): the group structure of the file must match"""
    sd = build_optimizer(model, "rmsprop", lr=0.01, staged_lr=True, new_layers=HEADS).state_dict()
    with pytest.raises(ValueError):
        build_optimizer(model, "rmsprop", lr=0.01).load_state_dict(sd)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_radam_schedule_changes_branch_between_steps_5_and_6():
    n5, s5 = radam_schedule(5, 0.9, 0.99)
    n6, s6 = radam_schedule(6, 0.9, 0.99)
    assert abs(n5 - 4.96) < 0.01 and abs(n6 - 5.94) < 0.01
    assert s5 == 1.0 / (1 - 0.9 ** 5) and s6 < 0.1          # the rectified step size starts small


def test_radam_restatement_matches_the_recorded_reference(golden_dir):
    """tests/util_optim.RAdamF64 (the float64 reference of the GPU kernel test) against the recording of the reference's own
    RAdam class, which computes in fp32: after EVERY one of the 14 steps (both branches) the parameters agree within twice
    the fp32 forward-error bound the restatement carries, and so do exp_avg / exp_avg_sq at the end"""
    z = np.load(os.path.join(golden_dir, "optim_golden.npz"))
    p0, grads = torch.from_numpy(z["p0"]), torch.from_numpy(z["grads"])
    lr, (b1, b2), eps = float(z["lr"]), [float(v) for v in z["betas"]], float(z["eps"])
    assert grads.shape[0] >= 12 and p0.numel() >= 200 and (b1, b2) == (0.9, 0.99)
    assert sorted(float(v) for v in z["decays"]) == [0.0, 5e-4]
    for k, wd in enumerate(float(v) for v in z["decays"]):
        ref = RAdamF64(p0, lr, b1, b2, eps, wd)
        branches = set()
        for t in range(grads.shape[0]):
            branches.add(ref.step(grads[t]) >= 5)
            got = torch.from_numpy(z["params_%d" % k][t]).double()
            err = (got - ref.w).abs()
            print("wd=%g step %2d: max |err| %.3e, max err/bound %.3f" % (wd, t + 1, float(err.max()), float((err / ref.ew).max())))
            assert bool((err <= 2 * ref.ew).all()), "wd=%g step %d" % (wd, t + 1)
            assert float(ref.ew.max()) < 64 * (t + 1) * U * float(ref.w.abs().max() + 1), "the bound itself stays at rounding level"
        assert branches == {False, True}
        assert int(z["step_%d" % k]) == grads.shape[0]
        assert bool(((torch.from_numpy(z["exp_avg_%d" % k]).double() - ref.m).abs() <= 2 * ref.em).all())
        assert bool(((torch.from_numpy(z["exp_avg_sq_%d" % k]).double() - ref.v).abs() <= 2 * ref.ev).all())
    # weight decay is decoupled and changes the result
    assert not np.array_equal(z["params_0"][-1], z["params_1"][-1])
