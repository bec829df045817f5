"""GPU: ieee_rmsprop_step and ieee_radam_step through the C ABI against float64 references, the grouped FusedSGD's step() against
its five step_part() calls, and one engine step per optimizer with staged learning rates against the reference-grouped
float64 optimizer applied to the same gradients.

Tolerances are the fp32 forward-error bounds of tests/util_optim.py (u = 2^-24 per rounding, carried through square root and
division and through the recursion over the steps), asserted with that file's slack factor 2.  The float64 references run on
the device (torch float64 arithmetic, no kernel of this package).  Gradients of the kernel tests keep |g| >= 0.5 * scale, so
sqrt(v) + eps is well conditioned; the engine tests take one step, where a vanishing gradient meets eps = 1e-8 instead.

Status: written and rehearsed without a device (the file's own logic against a numpy stand-in of the C functions); it has
not yet run on an MI355X, so there are no figures to report here (LABNOTES.md R10.1)."""
import numpy as np
import pytest
import torch

from tests.test_head_kernels_gpu import addr
from tests.util_optim import AdamF64, RAdamF64, RMSpropF64, SGDF64, U, reference_groups

pytestmark = pytest.mark.gpu

DEV = "cuda"
HEADS = ["fc_R", "fc_T", "fc_N", "classifier_R", "classifier_N", "classifier_T"]
N_TURN = 2048 * 256 * 4 + 12347          # > 2048 blocks * 256 lanes * 4 floats: the grid-stride loop turns on both paths
PAD = 8


def f32(v):
    return float(np.float32(v))


def _lib():
    from ieee_amd import _lib as L
    return L, L.require_gpu()


def within(got, ref, tol, what):
    """|got - ref| <= tol elementwise in float64, on the device, with the worst offender in the message"""
    got, ref = got.double(), ref.double()
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % what
    excess = (got - ref).abs() - tol
    if bool((excess > 0).any()):
        i = int(torch.argmax(excess))
        raise AssertionError("%s: %d elements out of bound; worst at %d: got %r want %r |err| %.3e > tol %.3e" % (
            what, int((excess > 0).sum()), i, float(got[i]), float(ref[i]), float((got[i] - ref[i]).abs()), float(tol[i])))


def bits_equal(a, b):
    view = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def _grads(gen, steps, n):
    """|g| >= 0.5 * scale with a scale that varies over the steps"""
    out = []
    for t in range(steps):
        r = torch.randn(n, generator=gen, device=DEV)
        out.append(torch.sign(r) * (0.5 + r.abs()) * (0.1 + 0.4 * (t % 7)))
    return out


def _padded(x, off, fill):
    """x placed `off` floats into a buffer of PAD more elements; the rest is `fill` (what must still be there afterwards)"""
    buf = fill.clone()
    buf[off:off + x.numel()] = x
    return buf


def _outside_untouched(buf, off, n, fill):
    return bits_equal(buf[:off], fill[:off]) and bits_equal(buf[off + n:], fill[off + n:])


# ---------------------------------------------------------------------------------------------------------------- 6
def test_rmsprop_step_fifty_steps_vector_and_scalar_paths():
    """ieee_rmsprop_step over 50 steps against torch.optim.RMSprop in float64 (hyper-parameters rounded to fp32, as the kernel
    receives them): momentum 0 with a NULL buffer and 0.9, weight decay 0 and 5e-4, slices at float offsets 0 (16-byte path)
    and 1..3 (scalar path) of n > 2048*256*4 elements; nothing outside the slice changes"""
    L, lib = _lib()
    gen = torch.Generator(device=DEV).manual_seed(810)
    n, steps = N_TURN, 50
    lr, alpha, eps = f32(1e-3), f32(0.99), f32(1e-8)
    p0 = torch.randn(n, generator=gen, device=DEV)
    grads = _grads(gen, steps, n)
    fill = torch.randn(n + PAD, generator=gen, device=DEV)
    for mom in (0.0, f32(0.9)):
        for wd in (0.0, f32(5e-4)):
            w = torch.nn.Parameter(p0.double().clone())
            opt = torch.optim.RMSprop([w], lr=lr, alpha=alpha, eps=eps, weight_decay=wd, momentum=mom, centered=False)
            ref = RMSpropF64(p0, lr, alpha, eps, wd, mom)
            for g in grads:
                w.grad = g.double()
                opt.step()
                ref.step(g)
            st = opt.state[w]
            # the restatement that carries the bound IS torch's optimizer (float64 against float64)
            assert float((ref.w - w.detach()).abs().max()) <= 1e-12 * float(w.detach().abs().max())
            assert float((ref.s - st["square_avg"]).abs().max()) <= 1e-12 * float(st["square_avg"].abs().max())
            print("rmsprop mom=%g wd=%g: bound on params max %.3e (|w| max %.3f), square_avg rel %.3e" % (
                mom, wd, float(ref.ew.max()), float(ref.w.abs().max()), float((ref.es / ref.s).max())))
            for off in range(4):
                what = "rmsprop off=%d mom=%g wd=%g" % (off, mom, wd)
                pd, sq = _padded(p0, off, fill), _padded(torch.zeros_like(p0), off, fill)
                buf = _padded(torch.zeros_like(p0), off, fill) if mom else None
                for g in grads:
                    gd = _padded(g, off, fill)
                    L.check(lib.ieee_rmsprop_step(addr(pd, off), addr(gd, off), addr(sq, off), addr(buf, off) if mom else None,
                                                  n, lr, alpha, eps, wd, mom, L.stream()))
                torch.cuda.synchronize()
                within(pd[off:off + n], w.detach(), 2 * ref.ew, what + " params")
                within(sq[off:off + n], st["square_avg"], 2 * ref.es, what + " square_avg")
                if mom:
                    within(buf[off:off + n], st["momentum_buffer"], 2 * ref.eb, what + " momentum_buffer")
                    assert _outside_untouched(buf, off, n, fill), what + ": momentum written outside the slice"
                assert _outside_untouched(pd, off, n, fill) and _outside_untouched(sq, off, n, fill), what + ": wrote outside the slice"


def test_rmsprop_and_radam_reject_bad_arguments():
    L, lib = _lib()
    t = torch.zeros(16, device=DEV)
    ok = lambda s: s == 0
    assert lib.ieee_rmsprop_step(None, L.ptr(t), L.ptr(t), None, 16, 1e-3, 0.99, 1e-8, 0.0, 0.0, L.stream()) < 0
    assert lib.ieee_rmsprop_step(L.ptr(t), L.ptr(t), L.ptr(t), None, 16, 1e-3, 0.99, 1e-8, 0.0, 0.9, L.stream()) < 0   # momentum without a buffer
    assert lib.ieee_rmsprop_step(L.ptr(t), L.ptr(t), L.ptr(t), None, -1, 1e-3, 0.99, 1e-8, 0.0, 0.0, L.stream()) < 0
    assert ok(lib.ieee_rmsprop_step(L.ptr(t), L.ptr(t), L.ptr(t), None, 0, 1e-3, 0.99, 1e-8, 0.0, 0.0, L.stream()))
    assert lib.ieee_radam_step(L.ptr(t), L.ptr(t), None, L.ptr(t), 16, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1, L.stream()) < 0
    assert lib.ieee_radam_step(L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), 16, 1e-3, 0.9, 0.99, 1e-8, 0.0, 0, L.stream()) < 0
    assert lib.ieee_radam_step(L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), -4, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1, L.stream()) < 0
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0


# ---------------------------------------------------------------------------------------------------------------- 7
def test_radam_step_across_both_branches_vector_and_scalar_paths():
    """ieee_radam_step over 14 steps (1-5: the SGD-like branch, 6-14: the rectified one, beta2 = 0.99) against the float64
    restatement that tests/test_optim_groups_cpu.py holds to the reference's own class; weight decay 0 and 5e-4, offsets 0..3,
    n > 2048*256*4; exp_avg and exp_avg_sq are checked too"""
    L, lib = _lib()
    gen = torch.Generator(device=DEV).manual_seed(820)
    n, steps = N_TURN, 14
    lr, b1, b2, eps = f32(1e-2), f32(0.9), f32(0.99), f32(1e-8)
    p0 = torch.randn(n, generator=gen, device=DEV)
    grads = _grads(gen, steps, n)
    fill = torch.randn(n + PAD, generator=gen, device=DEV)
    for wd in (0.0, f32(5e-4)):
        ref = RAdamF64(p0, lr, b1, b2, eps, wd)
        branches = [ref.step(g) >= 5 for g in grads]
        assert branches == [False] * 5 + [True] * 9
        print("radam wd=%g: bound on params max %.3e (|w| max %.3f)" % (wd, float(ref.ew.max()), float(ref.w.abs().max())))
        for off in range(4):
            what = "radam off=%d wd=%g" % (off, wd)
            pd = _padded(p0, off, fill)
            m, v = _padded(torch.zeros_like(p0), off, fill), _padded(torch.zeros_like(p0), off, fill)
            for t, g in enumerate(grads):
                gd = _padded(g, off, fill)
                L.check(lib.ieee_radam_step(addr(pd, off), addr(gd, off), addr(m, off), addr(v, off), n, lr, b1, b2, eps, wd, t + 1,
                                            L.stream()))
            torch.cuda.synchronize()
            within(pd[off:off + n], ref.w, 2 * ref.ew, what + " params")
            within(m[off:off + n], ref.m, 2 * ref.em, what + " exp_avg")
            within(v[off:off + n], ref.v, 2 * ref.ev, what + " exp_avg_sq")
            assert all(_outside_untouched(b, off, n, fill) for b in (pd, m, v)), what + ": wrote outside the slice"


# ---------------------------------------------------------------------------------------------------------------- 8
def test_grouped_sgd_step_equals_its_five_parts_bitwise():
    """a grouped FusedSGD over seeded random gradients: step() and step_part(0..4) leave bit-identical parameters, momentum
    and bf16 shadow, every shadow element is bf16(parameter), and the two groups moved by their own learning rates"""
    from ieee_amd.models import build_model
    from ieee_amd.optim import FusedSGD, build_optimizer
    m = build_model("ieee3modalPart", num_classes=171, loss="margin", pretrained=False, compute_dtype=torch.bfloat16)
    opt = build_optimizer(m, "sgd", lr=0.05, momentum=0.9, weight_decay=5e-4, staged_lr=True, new_layers=HEADS, base_lr_mult=0.1)
    assert isinstance(opt, FusedSGD) and m._shadow_enabled is True and len(opt.param_groups) == 2
    gen = torch.Generator(device=DEV).manual_seed(830)
    with torch.no_grad():
        m._flat_grads.copy_(torch.randn(m._flat_grads.numel(), generator=gen, device=DEV))
        opt.momentum_buffer().copy_(torch.randn(m._flat_grads.numel(), generator=gen, device=DEV) * 0.1)
    m.fresh_shadow()
    start = (m._flat_params.clone(), opt.momentum_buffer().clone(), m._flat_shadow.clone())
    opt.step()
    torch.cuda.synchronize()
    whole = (m._flat_params.clone(), opt.momentum_buffer().clone(), m._flat_shadow.clone())
    with torch.no_grad():
        m._flat_params.copy_(start[0]); opt.momentum_buffer().copy_(start[1]); m._flat_shadow.copy_(start[2])
    for part in range(5):
        opt.step_part(part)
    torch.cuda.synchronize()
    parts = (m._flat_params, opt.momentum_buffer(), m._flat_shadow)
    for a, b, what in zip(whole, parts, ("parameters", "momentum", "shadow")):
        assert bits_equal(a, b), what
    assert bits_equal(m._flat_shadow, m._flat_params.to(torch.bfloat16))
    # the groups: with these gradients the update is lr_group * (d + 0.9 b'), b' = 0.9 b + d, d = g + wd w -- in float64
    spans = opt.group_spans()
    touched = torch.zeros(m._flat_params.numel(), dtype=torch.bool, device=DEV)
    for gi, a, b in opt.launch_ranges():
        touched[a:b] = True
        lr = opt.param_groups[gi]["lr"]
        ref = SGDF64(start[0][a:b], f32(lr), f32(0.9), f32(5e-4))
        ref.b = start[1][a:b].double()
        ref.step(m._flat_grads[a:b])
        within(m._flat_params[a:b], ref.w, 2 * ref.ew, "group %d range [%d, %d)" % (gi, a, b))
    assert opt.param_groups[0]["lr"] == 0.05 * 0.1 and opt.param_groups[1]["lr"] == 0.05
    assert bits_equal(m._flat_params[~touched], start[0][~touched]) and int((~touched).sum()) > 0
    assert sorted(s for sp in spans for s in sp) == [(0, spans[1][0][0]), (spans[1][0][0], m._flat_params.numel())]


# ---------------------------------------------------------------------------------------------------------------- 9
class _DM(object):
    num_train_pids = 171
    sources = ["synthetic"]
    train_loader = []
    test_loader = {}


def _reference_step(optim, before, grads, mask, lr, wd):
    """the float64 optimizer the reference builds for `optim` (torch.optim, or the restatement of its RAdam) over the
    elements `mask` of one group, first step; returns (parameters, bound)"""
    w0, g = before[mask], grads[mask]
    lr, wd = f32(lr), f32(wd)
    if optim == "sgd":
        ref, topt = SGDF64(w0, lr, f32(0.9), wd), lambda p: torch.optim.SGD([p], lr=lr, momentum=f32(0.9), weight_decay=wd, dampening=0, nesterov=True)
    elif optim == "adam":
        ref, topt = AdamF64(w0, lr, f32(0.9), f32(0.99), f32(1e-8), wd), lambda p: torch.optim.Adam([p], lr=lr, betas=(f32(0.9), f32(0.99)), eps=f32(1e-8), weight_decay=wd)
    elif optim == "rmsprop":
        ref, topt = RMSpropF64(w0, lr, f32(0.99), f32(1e-8), wd, f32(0.9)), lambda p: torch.optim.RMSprop([p], lr=lr, alpha=f32(0.99), eps=f32(1e-8), weight_decay=wd, momentum=f32(0.9))
    else:
        ref, topt = RAdamF64(w0, lr, f32(0.9), f32(0.99), f32(1e-8), wd), None
    ref.step(g)
    want = ref.w
    if topt is not None:
        p = torch.nn.Parameter(w0.double().clone())
        p.grad = g.double()
        topt(p).step()
        want = p.detach()
        assert float((want - ref.w).abs().max()) <= 1e-12 * float(1 + want.abs().max()), "the restatement is not torch's " + optim
    return want, ref.ew


@pytest.mark.parametrize("optim", ["sgd", "adam", "rmsprop", "radam"])
def test_engine_step_with_staged_lr_matches_the_grouped_reference(optim):
    """one Image3MEngine.forward_backward with build_optimizer(..., staged_lr=True): the parameters before the step and the
    gradients it left in the flat buffer, fed to the reference-grouped float64 optimizer, give the parameters after it within
    the one-step fp32 bound, per group; parameters without a gradient do not move; with the backbone frozen its span stays"""
    from ieee_amd.engine import Image3MEngine
    from ieee_amd.models import build_model
    from ieee_amd.optim import FUSED_OPTIMIZERS, build_optimizer
    from tests.util_model import generated_state, images
    lr, wd, mult = 3e-4, 5e-4, 0.1
    m = build_model("ieee3modalPart", num_classes=171, loss="margin", pretrained=False, compute_dtype=torch.float32)
    m.load_state_dict(generated_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, 5))
    opt = build_optimizer(m, optim=optim, lr=lr, weight_decay=wd, momentum=0.9, staged_lr=True, new_layers=HEADS, base_lr_mult=mult)
    assert isinstance(opt, FUSED_OPTIMIZERS)
    eng = Image3MEngine(_DM(), m, opt, margin=1, use_gpu=True)
    assert eng._fused_ok()
    assert Image3MEngine(_DM(), m, build_optimizer(m, optim), margin=1, use_gpu=True)._fused_ok()          # ungrouped too
    m.train()
    B = 8
    pids = torch.arange(B) // 4
    batch = lambda seed: {"img": images(B, seed), "pid": pids, "camid": pids * 0, "impath": "", "timeid": pids * 0}
    before = m._flat_params.clone()
    eng.forward_backward(batch(5))
    torch.cuda.synchronize()
    grads, after = m._flat_grads.clone(), m._flat_params.clone()
    N = before.numel()
    trainable = torch.zeros(N, dtype=torch.bool, device=DEV)
    for a, b in m.trainable_runs():
        trainable[a:b] = True
    where = {id(p): (m._offsets[n], p.numel()) for n, p in m._param_items}
    groups = reference_groups(m, HEADS, lr, mult)
    covered = torch.zeros_like(trainable)
    for gi, g in enumerate(groups):
        mask = torch.zeros_like(trainable)
        for p in g["params"]:
            off, n = where[id(p)]
            mask[off:off + n] = True
        assert not bool((mask & covered).any())
        covered |= mask
        mask &= trainable
        assert opt.param_groups[gi]["lr"] == g.get("lr", lr)
        want, bound = _reference_step(optim, before, grads, mask, g.get("lr", lr), wd)
        err = (after[mask].double() - want).abs()
        print("%s group %d: %d elements, max |err| %.3e, max err/bound %.3f" % (optim, gi, int(mask.sum()), float(err.max()),
                                                                                  float((err / bound).max())))
        within(after[mask], want, 2 * bound, "%s group %d" % (optim, gi))
        assert not bits_equal(after[mask], before[mask])
    assert bool(covered.all())
    # REM.*.conv_value receives no gradient: bitwise unchanged
    assert int((~trainable).sum()) > 0 and bits_equal(after[~trainable], before[~trainable])
    for name, p in m._param_items:
        if ".conv_value." in name:
            off = m._offsets[name]
            assert not bool(trainable[off:off + p.numel()].any())
    # backbone frozen: its span does not move, the rest does
    for p in m.backbone.parameters():
        p.requires_grad = False
    end = where[id(list(m.backbone.parameters())[-1])]
    end = end[0] + end[1]
    assert end == 70524096
    eng.forward_backward(batch(6))
    torch.cuda.synchronize()
    assert bits_equal(m._flat_params[:end], after[:end])
    rest = trainable.clone()
    rest[:end] = False
    assert not bits_equal(m._flat_params[rest], after[rest])
    assert bits_equal(m._flat_params[~trainable], before[~trainable])
