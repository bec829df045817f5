"""Float64 restatements of the optimizers behind ieee_rmsprop_step / ieee_radam_step (and of SGD-nesterov / Adam for the
grouped engine tests), each with the fp32 forward-error bound of the kernel's arithmetic carried through the recursion, and
the reference's staged-lr grouping restated for tests (torchreid/optim/optimizer.py:78-108).

Error model (as tests/test_head_kernels_gpu.py): u = 2^-24 relative per fp32 rounding -- a product, a sum, a correctly
rounded quotient or square root, the conversion of a double scalar to fp32 -- and the errors the inputs already carry are
pushed through each operation to first order.  Every `k * U * (...)` below counts k roundings on the terms in the
parentheses; callers assert against TWICE the bound (the slack constant of that file: second-order terms, fused
multiply-adds that round once where two are counted).  The gradients of the tests are bounded away from zero, so
sqrt(v) + eps is well conditioned and the first-order term e_v / (2 sqrt(v)) of the square root holds."""
import math

import torch

U = 2.0 ** -24


def reference_groups(model, new_layers, lr, base_lr_mult):
    """optimizer.py:78-108, restated: named_children() order, base group first with lr * base_lr_mult"""
    if isinstance(new_layers, str):
        new_layers = [new_layers]
    if isinstance(model, torch.nn.DataParallel):
        model = model.module
    base, new = [], []
    for name, module in model.named_children():
        (new if name in new_layers else base).extend(module.parameters())
    return [{'params': base, 'lr': lr * base_lr_mult}, {'params': new}]


def radam_schedule(step, beta1, beta2):
    """radam.py:94-110 (degenerated_to_sgd=True) in Python floats: (N_sma, step_size)"""
    beta2_t = beta2 ** step
    n_sma_max = 2 / (1 - beta2) - 1
    n_sma = n_sma_max - 2 * step * beta2_t / (1 - beta2_t)
    if n_sma >= 5:
        step_size = math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_sma_max - 4) * (n_sma - 2) / n_sma * n_sma_max / (n_sma_max - 2)) / (
            1 - beta1 ** step)
    else:
        step_size = 1.0 / (1 - beta1 ** step)
    return n_sma, step_size


class RAdamF64(object):
    """radam.py:51-130 over one float64 tensor, with the error bounds (ew, em, ev) of an fp32 evaluation of the same steps"""

    def __init__(self, p, lr, beta1, beta2, eps, wd):
        self.w = p.double().clone()
        self.m, self.v = torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.ew, self.em, self.ev = torch.zeros_like(self.w), torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.lr, self.b1, self.b2, self.eps, self.wd = lr, beta1, beta2, eps, wd
        self.t = 0

    def step(self, grad):
        g = grad.double()
        b1, b2, lr = self.b1, self.b2, self.lr
        self.t += 1
        # v = b2 v + (1 - b2) g g: the scalar, two products and the sum on the new term, product and sum on the old one
        self.v = b2 * self.v + (1 - b2) * g * g
        self.ev = b2 * self.ev + 4 * U * self.v
        self.em = b1 * self.em + 4 * U * (b1 * self.m.abs() + (1 - b1) * g.abs())
        self.m = b1 * self.m + (1 - b1) * g
        n_sma, step_size = radam_schedule(self.t, b1, b2)
        x, ex = self.w, self.ew
        if self.wd != 0:
            # x = w - (wd lr) w: scalar, product, sum
            x = self.w - self.wd * lr * self.w
            ex = self.ew + 4 * U * self.w.abs()
        step_lr = step_size * lr
        if n_sma >= 5:
            root = self.v.sqrt()
            den = root + self.eps
            eden = self.ev / (2 * root.clamp_min(1e-30)) + 2 * U * den          # sqrt and the sum, one rounding each
            q = self.m / den
            upd = step_lr * q
            eupd = step_lr * (self.em / den + self.m.abs() * eden / den ** 2)
        else:
            upd = step_lr * self.m
            eupd = step_lr * self.em
        # quotient, scalar, product on the update; the final sum on both
        self.ew = ex + eupd + 4 * U * (upd.abs() + x.abs())
        self.w = x - upd
        return n_sma


class RMSpropF64(object):
    """torch.optim.RMSprop(centered=False) (torch/optim/rmsprop.py::_single_tensor_rmsprop) over one float64 tensor -- held
    to torch's own float64 optimizer by the tests that use it -- with the fp32 error bounds (ew, es, eb)"""

    def __init__(self, p, lr, alpha, eps, wd, momentum):
        self.w = p.double().clone()
        self.s, self.b = torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.ew, self.es, self.eb = torch.zeros_like(self.w), torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.lr, self.alpha, self.eps, self.wd, self.mom = lr, alpha, eps, wd, momentum

    def step(self, grad):
        g = grad.double()
        lr, al, mom = self.lr, self.alpha, self.mom
        d = g + self.wd * self.w
        ed = self.wd * self.ew + 2 * U * (g.abs() + self.wd * self.w.abs())
        self.s = al * self.s + (1 - al) * d * d
        self.es = al * self.es + (1 - al) * 2 * d.abs() * ed + 4 * U * self.s
        root = self.s.sqrt()
        den = root + self.eps
        eden = self.es / (2 * root.clamp_min(1e-30)) + 2 * U * den
        q = d / den
        eq = ed / den + d.abs() * eden / den ** 2 + U * q.abs()
        if mom != 0:
            self.eb = mom * self.eb + eq + 2 * U * (mom * self.b.abs() + q.abs())
            self.b = mom * self.b + q
            upd, eupd = self.b, self.eb
        else:
            upd, eupd = q, eq
        self.ew = self.ew + lr * eupd + 2 * U * (self.w.abs() + lr * upd.abs())
        self.w = self.w - lr * upd


class SGDF64(object):
    """torch.optim.SGD(momentum, weight_decay, dampening=0, nesterov) over one float64 tensor with the fp32 error bounds of
    sgd_one (ieee_amd/csrc/head.hip), the recursion of tests/test_head_kernels_gpu.py::_sgd_ref_and_bound"""

    def __init__(self, p, lr, momentum, wd, nesterov=True):
        self.w = p.double().clone()
        self.b = torch.zeros_like(self.w)
        self.ew, self.eb = torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.lr, self.mom, self.wd, self.nesterov = lr, momentum, wd, nesterov

    def step(self, grad):
        g = grad.double()
        lr, mom, wd = self.lr, self.mom, self.wd
        d = g + wd * self.w
        ed = wd * self.ew + 2 * U * (g.abs() + wd * self.w.abs())
        if mom:
            nb = mom * self.b + d
            self.eb = mom * self.eb + ed + 2 * U * (mom * self.b.abs() + d.abs())
            self.b = nb
            if self.nesterov:
                ed = ed + mom * self.eb + 2 * U * (d.abs() + mom * nb.abs())
                d = d + mom * nb
            else:
                ed, d = self.eb.clone(), nb
        self.ew = self.ew + lr * ed + 2 * U * (self.w.abs() + lr * d.abs())
        self.w = self.w - lr * d


class AdamF64(object):
    """torch.optim.Adam (L2 decay, bias correction, no amsgrad) over one float64 tensor with the fp32 error bounds of
    adam_kernel, the recursion of tests/test_head_kernels_gpu.py::test_adam_fifty_steps_with_weight_decay"""

    def __init__(self, p, lr, beta1, beta2, eps, wd):
        self.w = p.double().clone()
        self.m, self.v = torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.ew, self.em, self.ev = torch.zeros_like(self.w), torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.lr, self.b1, self.b2, self.eps, self.wd = lr, beta1, beta2, eps, wd
        self.t = 0

    def step(self, grad):
        g = grad.double()
        lr, b1, b2 = self.lr, self.b1, self.b2
        self.t += 1
        d = g + self.wd * self.w
        ed = self.wd * self.ew + 2 * U * (g.abs() + self.wd * self.w.abs())
        self.m = b1 * self.m + (1 - b1) * d
        self.v = b2 * self.v + (1 - b2) * d * d
        bc1, bc2s = 1 - b1 ** self.t, (1 - b2 ** self.t) ** 0.5
        self.em = b1 * self.em + (1 - b1) * ed + 4 * U * (self.m.abs() + d.abs())
        self.ev = b2 * self.ev + (1 - b2) * 2 * d.abs() * ed + 4 * U * (self.v + (1 - b2) * d * d)
        root = self.v.sqrt()
        denom = root / bc2s + self.eps
        edn = self.ev / (2 * root.clamp_min(1e-30)) / bc2s + 4 * U * denom
        upd = lr / bc1 * self.m / denom
        self.ew = self.ew + lr / bc1 * (self.em / denom + self.m.abs() * edn / denom ** 2) + 4 * U * (upd.abs() + self.w.abs())
        self.w = self.w - upd
