"""Mirror of torchreid.optim (reference torchreid/optim/optimizer.py:11-157, lr_scheduler.py:7-68): the five optimizers of
`build_optimizer`, staged learning rates included, with a MultiStepLR / StepLR / cosine schedule.  On a native model every
optimizer is a fused one: FusedSGD, FusedAdam, FusedRMSprop and FusedRAdam run one element-wise kernel over the model's flat
parameter / gradient buffers (one launch per contiguous trainable run of a parameter group) and are torch.optim.Optimizers,
so schedulers, state_dict() and the reference's checkpoint code keep working.

Parameter groups (staged_lr).  The reference puts the children named in `new_layers` in one group and every other child
in a base group that trains at lr * base_lr_mult (optimizer.py:78-108).  Every parameter is a view of the flat buffer, so
a group IS a set of element spans of it; what a fused optimizer launches over is the model's trainable runs (or the runs
of one staged-backward part) cut at the group boundaries, each piece with its own group's hyper-parameters, read from
`param_groups` at every step (that is where schedulers write them)."""
import torch

from . import _lib

AVAI_OPTIMS = ['adam', 'amsgrad', 'sgd', 'rmsprop', 'radam']
AVAI_SCH = ['single_step', 'multi_step', 'cosine']


def staged_param_groups(model, new_layers, lr, base_lr_mult):
    """the reference's two groups (optimizer.py:78-108): [{'params': base, 'lr': lr * base_lr_mult}, {'params': new}], children
    in named_children() order.  A name that is no child (the default '' among them) selects nothing: the new group is then
    empty, which torch.optim accepts, and everything trains at the base rate -- as the reference's own call does."""
    if isinstance(new_layers, str):
        new_layers = [new_layers]
    if isinstance(model, torch.nn.DataParallel):
        model = model.module
    base_params, new_params = [], []
    for name, module in model.named_children():
        if name in new_layers:
            new_params += [p for p in module.parameters()]
        else:
            base_params += [p for p in module.parameters()]
    return [{'params': base_params, 'lr': lr * base_lr_mult}, {'params': new_params}]


class _FlatOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share: parameter groups as spans of the model's flat buffer, the launch ranges cut from
    the model's runs, and checkpoint interop -- state_dict() carries the state as per-parameter entries under the keys
    of the torch / reference optimizer (`_KEYS`, views of the flat state buffers, so a file stores them once, numbered
    in group order as torch numbers them) and load_state_dict() scatters such entries, from either implementation, back
    into the flat buffers."""
    _KEYS = ()
    _HAS_STEP = False

    def __init__(self, model, defaults, param_groups=None):
        self.model = model
        self._ungrouped = param_groups is None
        super(_FlatOptimizer, self).__init__(list(model.parameters()) if param_groups is None else param_groups, defaults)
        self._step = 0
        self._ranges_key = None

    # ---- groups over the flat buffer ------------------------------------------------------------------------------
    def _where(self):
        """id(parameter) -> (offset, numel) in the flat buffers"""
        m = self.model
        if getattr(self, "_where_for", None) is not m._param_items:
            self._where_map = {id(p): (m._offsets[name], p.numel()) for name, p in m._param_items}
            self._where_for = m._param_items
        return self._where_map

    def group_spans(self):
        """per parameter group, the merged [start, end) element spans of the flat buffer its parameters occupy"""
        where = self._where()
        out = []
        for g in self.param_groups:
            spans = []
            for off, n in sorted(where[id(p)] for p in g['params']):
                if spans and spans[-1][1] == off:
                    spans[-1][1] = off + n
                else:
                    spans.append([off, off + n])
            out.append([tuple(s) for s in spans])
        return out

    @staticmethod
    def _cut(runs, spans):
        """runs ∩ the groups' spans as (group, start, end), in address order within a run; adjacent pieces of one group merge"""
        cut = []
        for a, b in runs:
            pieces = sorted((max(a, c), min(b, d), gi) for gi, sp in enumerate(spans) for c, d in sp if max(a, c) < min(b, d))
            for lo, hi, gi in pieces:
                if cut and cut[-1][0] == gi and cut[-1][2] == lo:
                    cut[-1] = (gi, cut[-1][1], hi)
                else:
                    cut.append((gi, lo, hi))
        return cut

    def launch_ranges(self, part=None, parts=None):
        """[(group index, start, end)]: one kernel launch each.  part=None: the whole step (model.trainable_runs());
        part=p: what is final after staged-backward part p (model.part_runs()[p]).  Built over model.parameters() (no
        explicit groups) these are exactly the model's runs; otherwise the runs are cut at the group boundaries, cached on
        what part_runs() is cached on plus the grouping.  (parts: model.part_runs(), when the caller already holds it.)"""
        m = self.model
        if self._ungrouped and len(self.param_groups) == 1:
            return [(0, a, b) for a, b in (m.trainable_runs() if part is None else (parts or m.part_runs())[part])]
        key = (m.interaction, m.attention, m.using_REM, tuple(p.requires_grad for _, p in m._param_items),
               tuple(len(g['params']) for g in self.param_groups), id(m._param_items))
        if self._ranges_key != key:
            spans = self.group_spans()
            ranges = {None: self._cut(m.trainable_runs(), spans)}
            for i, runs in enumerate(m.part_runs()):
                ranges[i] = self._cut(runs, spans)
            self._ranges, self._ranges_key = ranges, key
        return self._ranges[part]

    def zero_grad(self, set_to_none=True):
        for p in self.model.parameters():
            p.grad = None

    # ---- state --------------------------------------------------------------------------------------------------
    def _flats(self):
        """the flat state tensors, one per entry of _KEYS (None: this configuration keeps no such state)"""
        raise NotImplementedError

    def flat_state(self):
        """the flat state tensors (data-parallel replica synchronisation)"""
        return [t for t in self._flats() if t is not None]

    def _step_entry(self):
        return torch.tensor(float(self._step))

    def _fused_note(self):
        return {'layout': 'per-parameter views of flat buffers', 'step': self._step}

    def _load_legacy(self, fused, flats):
        return False

    def _publish_views(self):
        flats, where = self._flats(), self._where()
        for g in self.param_groups:
            for p in g['params']:
                off, n = where[id(p)]
                st = self.state[p]
                if self._HAS_STEP:
                    st['step'] = self._step_entry()
                for key, flat in zip(self._KEYS, flats):
                    if flat is not None:
                        st[key] = flat[off:off + n].view(p.shape)

    def state_dict(self):
        self._publish_views()
        d = super(_FlatOptimizer, self).state_dict()
        d['fused'] = self._fused_note()
        return d

    def load_state_dict(self, state_dict):
        fused = state_dict.get('fused')
        super(_FlatOptimizer, self).load_state_dict({k: v for k, v in state_dict.items() if k != 'fused'})
        flats, where = self._flats(), self._where()
        if not self._load_legacy(fused, flats):
            steps = []
            for flat in flats:
                if flat is not None:
                    flat.zero_()
            for g in self.param_groups:
                for p in g['params']:
                    st = self.state.get(p, {})
                    off, n = where[id(p)]
                    if 'step' in st:
                        steps.append(int(float(st['step'])))
                    for key, flat in zip(self._KEYS, flats):
                        if flat is not None and st.get(key) is not None:
                            flat[off:off + n].copy_(st[key].reshape(-1))
            self._step = max(steps) if steps else (int(fused['step']) if fused and 'step' in fused else 0)
        self._publish_views()


class FusedSGD(_FlatOptimizer):
    """torch.optim.SGD(momentum, weight_decay, dampening=0, nesterov) (reference optim/optimizer.py:130-138): state key
    `momentum_buffer`, exactly where torch.optim.SGD keeps its own."""
    _KEYS = ('momentum_buffer',)

    def __init__(self, model, lr=1e-3, momentum=0.9, weight_decay=5e-4, nesterov=True, param_groups=None):
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov, dampening=0)
        super(FusedSGD, self).__init__(model, defaults, param_groups)
        self._buf = None
        # the update also writes the bf16 image of the new parameters (ieee_sgd_nesterov_step_shadow): the bf16 training forward
        # then reads the 1x1 convolutions' GEMM operands from that shadow instead of packing them (IEEE_SGD_SHADOW=0: off)
        import os
        model._shadow_enabled = os.environ.get("IEEE_SGD_SHADOW", "1") != "0" and getattr(model, "compute_dtype", None) == torch.bfloat16
        self._parts_done = set()

    def momentum_buffer(self):
        if self._buf is None or self._buf.device != self.model._flat_params.device:
            self._buf = torch.zeros_like(self.model._flat_params)
        return self._buf

    def _flats(self):
        return (self.momentum_buffer(),)

    def _update(self, ranges):
        lib = _lib.require_gpu()
        m = self.model
        buf = self.momentum_buffer()
        m._native_epoch += 1                      # parameters change behind torch's version counters
        self._opt_called = True                   # what torch's schedulers look at to order step() calls (step_part too)
        shadow = m.shadow_buffer() if getattr(m, "_shadow_enabled", False) else None
        # skip_flags (set by the engine for the duration of a fused step): the executor's range-guard words -- a step whose
        # BatchNorm sums were clamped leaves parameters, momentum and shadow untouched (include/ieee_amd.h)
        skip = getattr(self, "skip_flags", None)
        for gi, a, b in ranges:
            g = self.param_groups[gi]
            _lib.check(lib.ieee_sgd_nesterov_step_ex(_lib.ptr(m._flat_params[a:b]), _lib.ptr(m._flat_grads[a:b]),
                                                     _lib.ptr(buf[a:b]), b - a, float(g['lr']), float(g['momentum']),
                                                     float(g['weight_decay']), 1 if g['nesterov'] else 0,
                                                     _lib.ptr(shadow[a:b]) if shadow is not None else None,
                                                     _lib.ptr(skip) if skip is not None else None, _lib.stream()))

    @torch.no_grad()
    def step(self, closure=None):
        """uses the gradients the native backward left in the model's flat gradient buffer"""
        self._update(self.launch_ranges())
        self.model.shadow_is_current()

    @torch.no_grad()
    def step_part(self, part):
        """the same update restricted to the parameters whose gradients are final after staged-backward part `part`
        (model.part_runs()); the five parts together are exactly step().  Runs on the current stream."""
        parts = self.model.part_runs()
        self._update(self.launch_ranges(part, parts))
        if part == 0:
            self._parts_done = set()
        self._parts_done.add(part)
        if len(self._parts_done) == len(parts):   # every trainable parameter (and its shadow element) has been written
            self._parts_done = set()
            self.model.shadow_is_current()

    def _fused_note(self):
        return {'layout': 'per-parameter views of one flat buffer'}

    def _load_legacy(self, fused, flats):
        if fused is not None and fused.get('momentum_buffer') is not None:        # files written by round-1 builds
            flats[0].copy_(fused['momentum_buffer'])
            return True
        return False


class FusedAdam(_FlatOptimizer):
    """torch.optim.Adam(lr, betas, eps=1e-8, weight_decay[, amsgrad]) over the model's flat buffers in one launch per
    contiguous trainable run (reference optim/optimizer.py:113-128 builds exactly these two variants); state keys step,
    exp_avg, exp_avg_sq, max_exp_avg_sq as torch.optim.Adam's."""
    _KEYS = ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')
    _HAS_STEP = True

    def __init__(self, model, lr=0.0003, betas=(0.9, 0.99), eps=1e-8, weight_decay=5e-4, amsgrad=False, param_groups=None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        super(FusedAdam, self).__init__(model, defaults, param_groups)
        model._shadow_enabled = False              # (the bf16 parameter shadow is FusedSGD's: every operand is packed here)
        self._m = self._v = self._vmax = None

    def _buffers(self):
        ref = self.model._flat_params
        if self._m is None or self._m.device != ref.device:
            self._m, self._v = torch.zeros_like(ref), torch.zeros_like(ref)
            self._vmax = torch.zeros_like(ref) if any(g['amsgrad'] for g in self.param_groups) else None
        return self._m, self._v, self._vmax

    _flats = _buffers

    @torch.no_grad()
    def step(self, closure=None):
        lib = _lib.require_gpu()
        mdl = self.model
        m, v, vmax = self._buffers()
        self._step += 1
        mdl._native_epoch += 1                    # parameters change behind torch's version counters
        for gi, a, b in self.launch_ranges():
            g = self.param_groups[gi]
            _lib.check(lib.ieee_adam_step(_lib.ptr(mdl._flat_params[a:b]), _lib.ptr(mdl._flat_grads[a:b]), _lib.ptr(m[a:b]),
                                          _lib.ptr(v[a:b]), _lib.ptr(vmax[a:b]) if g['amsgrad'] else None, b - a,
                                          float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']),
                                          float(g['weight_decay']), self._step, _lib.stream()))

    def _load_legacy(self, fused, flats):
        if fused is not None and fused.get('exp_avg') is not None:                  # files written by round-1 builds
            self._step = int(fused['step'])
            flats[0].copy_(fused['exp_avg']); flats[1].copy_(fused['exp_avg_sq'])
            if flats[2] is not None and fused.get('max_exp_avg_sq') is not None:
                flats[2].copy_(fused['max_exp_avg_sq'])
            return True
        return False


class FusedRMSprop(_FlatOptimizer):
    """torch.optim.RMSprop(lr, alpha, eps=1e-8, weight_decay, momentum, centered=False) as the reference builds it
    (optim/optimizer.py:140-147) in one ieee_rmsprop_step launch per range; state keys step, square_avg and (momentum > 0)
    momentum_buffer as torch.optim.RMSprop's."""
    _KEYS = ('square_avg', 'momentum_buffer')
    _HAS_STEP = True

    def __init__(self, model, lr=0.0003, alpha=0.99, eps=1e-8, weight_decay=5e-4, momentum=0.9, param_groups=None):
        defaults = dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=False, weight_decay=weight_decay)
        super(FusedRMSprop, self).__init__(model, defaults, param_groups)
        if any(g['centered'] for g in self.param_groups):
            raise ValueError("FusedRMSprop implements centered=False, what the reference builds")
        model._shadow_enabled = False              # (the bf16 parameter shadow is FusedSGD's)
        self._sq = self._buf = None

    def _flats(self):
        ref = self.model._flat_params
        if self._sq is None or self._sq.device != ref.device:
            self._sq = torch.zeros_like(ref)
            self._buf = torch.zeros_like(ref) if any(g['momentum'] != 0 for g in self.param_groups) else None
        return self._sq, self._buf

    @torch.no_grad()
    def step(self, closure=None):
        lib = _lib.require_gpu()
        mdl = self.model
        sq, buf = self._flats()
        self._step += 1
        mdl._native_epoch += 1                    # parameters change behind torch's version counters
        for gi, a, b in self.launch_ranges():
            g = self.param_groups[gi]
            _lib.check(lib.ieee_rmsprop_step(_lib.ptr(mdl._flat_params[a:b]), _lib.ptr(mdl._flat_grads[a:b]), _lib.ptr(sq[a:b]),
                                             _lib.ptr(buf[a:b]) if g['momentum'] != 0 else None, b - a, float(g['lr']),
                                             float(g['alpha']), float(g['eps']), float(g['weight_decay']),
                                             float(g['momentum']), _lib.stream()))


class FusedRAdam(_FlatOptimizer):
    """The reference's vendored RAdam (optim/radam.py:19-130, degenerated_to_sgd=True; built at optim/optimizer.py:149-155),
    which is not torch.optim.RAdam: decoupled weight decay, rectified branch from N_sma >= 5, sqrt(v)+eps without bias
    correction.  One ieee_radam_step launch per range; state keys step (a Python int, as the reference keeps it), exp_avg,
    exp_avg_sq."""
    _KEYS = ('exp_avg', 'exp_avg_sq')
    _HAS_STEP = True

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, param_groups=None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super(FusedRAdam, self).__init__(model, defaults, param_groups)
        model._shadow_enabled = False              # (the bf16 parameter shadow is FusedSGD's)
        self._m = self._v = None

    def _flats(self):
        ref = self.model._flat_params
        if self._m is None or self._m.device != ref.device:
            self._m, self._v = torch.zeros_like(ref), torch.zeros_like(ref)
        return self._m, self._v

    def _step_entry(self):
        return int(self._step)

    @torch.no_grad()
    def step(self, closure=None):
        lib = _lib.require_gpu()
        mdl = self.model
        m, v = self._flats()
        self._step += 1
        mdl._native_epoch += 1                    # parameters change behind torch's version counters
        for gi, a, b in self.launch_ranges():
            g = self.param_groups[gi]
            _lib.check(lib.ieee_radam_step(_lib.ptr(mdl._flat_params[a:b]), _lib.ptr(mdl._flat_grads[a:b]), _lib.ptr(m[a:b]),
                                           _lib.ptr(v[a:b]), b - a, float(g['lr']), float(g['betas'][0]), float(g['betas'][1]),
                                           float(g['eps']), float(g['weight_decay']), self._step, _lib.stream()))


FUSED_OPTIMIZERS = (FusedSGD, FusedAdam, FusedRMSprop, FusedRAdam)


def build_optimizer(model, optim='adam', lr=0.0003, weight_decay=5e-04, momentum=0.9, sgd_dampening=0,
                    sgd_nesterov=False, rmsprop_alpha=0.99, adam_beta1=0.9, adam_beta2=0.99, staged_lr=False,
                    new_layers='', base_lr_mult=0.1, fused=True):
    """reference optim/optimizer.py:11-157.  Note the reference's SGD branch hard-codes nesterov=True
    (:137) whatever `sgd_nesterov` says; kept.  `fused=True` on a native model returns the fused class for every `optim`
    (FusedSGD, FusedAdam for 'adam' / 'amsgrad', FusedRMSprop, FusedRAdam); `staged_lr` builds the reference's two
    parameter groups (staged_param_groups) for the fused and the torch.optim objects alike.
    `fused=False`, or a model without flat buffers, returns torch.optim objects; for 'radam' that is torch.optim.RAdam,
    which is NOT the algorithm of the reference's own RAdam class (radam.py:19-130: decoupled decay, threshold N_sma >= 5,
    no bias correction in the denominator) -- FusedRAdam is."""
    if optim not in AVAI_OPTIMS:
        raise ValueError('Unsupported optim: {}. Must be one of {}'.format(optim, AVAI_OPTIMS))
    if not isinstance(model, torch.nn.Module):
        raise TypeError('model given to build_optimizer must be an instance of nn.Module')
    if isinstance(model, torch.nn.DataParallel):
        model = model.module
    groups = staged_param_groups(model, new_layers, lr, base_lr_mult) if staged_lr else None
    if fused and hasattr(model, "trainable_runs"):
        if optim == 'sgd':
            return FusedSGD(model, lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=True, param_groups=groups)
        if optim in ('adam', 'amsgrad'):
            return FusedAdam(model, lr=lr, betas=(adam_beta1, adam_beta2), weight_decay=weight_decay,
                             amsgrad=(optim == 'amsgrad'), param_groups=groups)
        if optim == 'rmsprop':
            return FusedRMSprop(model, lr=lr, momentum=momentum, weight_decay=weight_decay, alpha=rmsprop_alpha,
                                param_groups=groups)
        return FusedRAdam(model, lr=lr, weight_decay=weight_decay, betas=(adam_beta1, adam_beta2), param_groups=groups)
    params = groups if staged_lr else model.parameters()
    if optim == 'sgd':
        return torch.optim.SGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay,
                               dampening=sgd_dampening, nesterov=True)
    if optim == 'adam':
        return torch.optim.Adam(params, lr=lr, weight_decay=weight_decay, betas=(adam_beta1, adam_beta2))
    if optim == 'amsgrad':
        return torch.optim.Adam(params, lr=lr, weight_decay=weight_decay, betas=(adam_beta1, adam_beta2),
                                amsgrad=True)
    if optim == 'rmsprop':
        return torch.optim.RMSprop(params, lr=lr, momentum=momentum, weight_decay=weight_decay, alpha=rmsprop_alpha)
    return torch.optim.RAdam(params, lr=lr, weight_decay=weight_decay, betas=(adam_beta1, adam_beta2))


def build_lr_scheduler(optimizer, lr_scheduler='single_step', stepsize=1, gamma=0.1, max_epoch=1):
    """reference optim/lr_scheduler.py:7-68"""
    if lr_scheduler not in AVAI_SCH:
        raise ValueError('Unsupported scheduler: {}. Must be one of {}'.format(lr_scheduler, AVAI_SCH))
    if lr_scheduler == 'single_step':
        if isinstance(stepsize, list):
            stepsize = stepsize[-1]
        if not isinstance(stepsize, int):
            raise TypeError('For single_step lr_scheduler, stepsize must be an integer, but got {}'.format(
                type(stepsize)))
        return torch.optim.lr_scheduler.StepLR(optimizer, step_size=stepsize, gamma=gamma)
    if lr_scheduler == 'multi_step':
        if not isinstance(stepsize, list):
            raise TypeError('For multi_step lr_scheduler, stepsize must be a list, but got {}'.format(type(stepsize)))
        return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=stepsize, gamma=gamma)
    return torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, float(max_epoch))
