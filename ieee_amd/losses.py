"""Mirror of torchreid.losses.  Same classes / call signatures as the reference (torchreid/losses/cross_entropy_loss.py:6-50,
multi_modal_margin_loss_new.py:7-40, hard_mine_triplet_loss.py:6-48, hcloss.py:6-39, losses/__init__.py:9-44); forward AND
backward run in ieee_ce_ls_fwd_bwd / ieee_margin3m_fwd_bwd (the two criteria of the margin config) and in
ieee_triplet_hard_fwd_bwd / ieee_center_pairs_fwd_bwd (csrc/metric_loss.hip).  `time_loss` has no counterpart: it measures
dist(center, center) and returns the python int 0 without a graph."""
import torch
from torch import nn

from . import _lib


def chunks_short_of_identities(pids):
    """True when `feat.chunk(n)` yields fewer than n = len(unique(pids)) pieces, i.e. when the reference's 3M loss dies
    with `IndexError: tuple index out of range` in its first loop (multi_modal_margin_loss_new.py:24-33) BEFORE any
    gradient exists.  Evaluated on the host so that the same error can be raised before anything is launched."""
    rows = int(pids.numel())
    n = int(torch.unique(pids).numel())
    per = -(-rows // n)
    return -(-rows // per) < n


def target_out_of_range(targets, num_classes):
    """The RuntimeError the reference's cross entropy raises for a label outside [0, num_classes) -- its one-hot is a
    host-side `scatter_` (cross_entropy_loss.py:45-46) -- or None.  ce_rows_kernel reads logits[target] unchecked, so
    this runs on the host before the launch."""
    t = targets.detach().reshape(-1)
    bad = (t < 0) | (t >= num_classes)
    if not bool(bad.any()):
        return None
    v = int(t[bad][0])
    return RuntimeError("index %d is out of bounds for dimension 1 with size %d" % (v, num_classes))


class _CEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, eps):
        lib = _lib.require_gpu()
        x = logits.to(torch.float32).contiguous()
        squeeze = x.dim() == 2
        if squeeze:
            x = x.unsqueeze(0)
        heads, B, C = x.shape
        t = targets.to(device=x.device, dtype=torch.int64).contiguous()
        dl = torch.empty_like(x)
        head_loss = torch.empty(heads, dtype=torch.float32, device=x.device)
        head_acc = torch.empty(heads, dtype=torch.float32, device=x.device)
        work = torch.empty(heads * B * 2, dtype=torch.float32, device=x.device)
        _lib.check(lib.ieee_ce_ls_fwd_bwd(_lib.ptr(x), _lib.ptr(t), _lib.ptr(dl), _lib.ptr(head_loss),
                                          _lib.ptr(head_acc), _lib.ptr(work), heads, B, C, float(eps), 1.0,
                                          _lib.stream()))
        ctx.save_for_backward(dl)
        ctx.squeeze = squeeze
        return head_loss[0] if squeeze else head_loss


    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        if ctx.squeeze:
            return dl[0] * g, None, None
        return dl * g.view(-1, 1, 1), None, None


class CrossEntropyLoss(nn.Module):
    r"""Cross entropy loss with label smoothing regularizer (reference cross_entropy_loss.py:6-50):
    ``(-t * log_softmax(x)).mean(0).sum()`` with ``t = (1-eps)*onehot + eps/K``.  The reference builds
    the one-hot on the host (`targets.cpu()`, :46); here nothing leaves the device."""

    def __init__(self, num_classes, eps=0.1, use_gpu=True, label_smooth=True):
        super(CrossEntropyLoss, self).__init__()
        self.num_classes = num_classes
        self.eps = eps if label_smooth else 0
        self.use_gpu = use_gpu

    def forward(self, inputs, targets):
        assert inputs.dim() == 2 and inputs.size(1) == self.num_classes
        err = target_out_of_range(targets.cpu(), self.num_classes)   # the reference moves the targets to the host too
        if err is not None:
            raise err
        return _CEFunction.apply(inputs, targets, self.eps)


class _MarginFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f1, f2, f3, pids, margin):
        lib = _lib.require_gpu()
        feats = torch.stack([f1, f2, f3]).to(torch.float32).contiguous()
        _, B, D = feats.shape
        p = pids.to(device=feats.device, dtype=torch.int64).contiguous()
        df = torch.empty_like(feats)
        out3 = torch.empty(3, dtype=torch.float32, device=feats.device)
        work = torch.empty(B + 3, dtype=torch.float32, device=feats.device)
        _lib.check(lib.ieee_margin3m_fwd_bwd(_lib.ptr(feats), _lib.ptr(p), _lib.ptr(df), _lib.ptr(out3), _lib.ptr(work), B, D,
                                             float(margin), 1.0, _lib.stream()))
        ctx.save_for_backward(df)
        ctx.out3 = out3
        return out3[0]

    @staticmethod
    def backward(ctx, g):
        (df,) = ctx.saved_tensors
        return df[0] * g, df[1] * g, df[2] * g, None, None


DIST_TYPES = {'l2': 0, 'l1': 1, 'cos': 2}          # IEEE_DIST_* of include/ieee_amd.h
CENTER_HETERO, CENTER_MARGIN3M = 0, 1             # IEEE_CENTER_*


class _CenterPairsFunction(torch.autograd.Function):
    """ieee_center_pairs_fwd_bwd over M = len(feats) modalities: the loss and its gradient in one call"""

    @staticmethod
    def forward(ctx, pids, dist_type, mode, margin, *fs):
        lib = _lib.require_gpu()
        feats = torch.stack(fs).to(torch.float32).contiguous()
        M, B, D = feats.shape
        p = pids.to(device=feats.device, dtype=torch.int64).contiguous()
        df = torch.empty_like(feats)
        out3 = torch.empty(3, dtype=torch.float32, device=feats.device)
        work = torch.empty(B + 3, dtype=torch.float32, device=feats.device)
        _lib.check(lib.ieee_center_pairs_fwd_bwd(_lib.ptr(feats), M, _lib.ptr(p), _lib.ptr(df), _lib.ptr(out3), _lib.ptr(work),
                                                 B, D, DIST_TYPES[dist_type], mode, float(margin), 1.0, 0, _lib.stream()))
        ctx.save_for_backward(df)
        return out3[0]

    @staticmethod
    def backward(ctx, g):
        (df,) = ctx.saved_tensors
        return (None, None, None, None) + tuple(df[m] * g for m in range(df.shape[0]))


class multiModalMarginLossNew(nn.Module):
    """3M loss, reference multi_modal_margin_loss_new.py:7-40 (dist_type 'l2' is the one the engine uses:
    margin.py:80-91 constructs it with the default).  Per identity chunk: centers per modality,
    max(|m-d(1,2)|, |m-d(2,3)|, |m-d(1,3)|), summed over chunks, with d = squared L2 ('l2', ieee_margin3m_fwd_bwd) or
    the mean of absolute differences ('l1' = nn.L1Loss, ieee_center_pairs_fwd_bwd)."""

    def __init__(self, margin=3, dist_type='l2'):
        super(multiModalMarginLossNew, self).__init__()
        if dist_type == 'cos':
            raise NotImplementedError("dist_type='cos': the reference's forward raises UnboundLocalError for it -- its loop "
                                      "handles 'l2' and 'l1' only and never assigns `dist` "
                                      "(multi_modal_margin_loss_new.py:32-40) -- so there is nothing to reproduce")
        if dist_type not in ('l2', 'l1'):
            raise NotImplementedError("dist_type must be 'l2' or 'l1', not %r" % (dist_type,))
        self.dist_type = dist_type
        self.margin = margin

    def forward(self, feat1, feat2, feat3, label1):
        if chunks_short_of_identities(label1.cpu()):
            raise IndexError('tuple index out of range')     # the reference's loop over the chunks (:24-33)
        if self.dist_type == 'l2':
            return _MarginFunction.apply(feat1, feat2, feat3, label1, self.margin)
        return _CenterPairsFunction.apply(label1, self.dist_type, CENTER_MARGIN3M, self.margin, feat1, feat2, feat3)


class hetero_loss(nn.Module):
    """Hetero-center loss, reference hcloss.py:6-39: per identity chunk (torch.chunk over the unique labels) the distance
    of the two modality centres, summed over the chunks -- 'l2' |sum (c1-c2)^2|, 'l1' |mean |c1-c2||, 'cos'
    max(0, 1 - cos(c1, c2)).  `margin` is stored and, as in the reference, not used."""

    def __init__(self, margin=0.1, dist_type='l2'):
        super(hetero_loss, self).__init__()
        if dist_type not in DIST_TYPES:
            raise NotImplementedError("dist_type must be 'l2', 'l1' or 'cos', not %r" % (dist_type,))
        self.margin = margin
        self.dist_type = dist_type

    def forward(self, feat1, feat2, label1):
        if chunks_short_of_identities(label1.cpu()):
            raise IndexError('tuple index out of range')     # feat1[i] past the chunks (hcloss.py:25-27)
        return _CenterPairsFunction.apply(label1, self.dist_type, CENTER_HETERO, self.margin, feat1, feat2)


def single_identity(pids):
    """True when every row carries the same label: batch-hard mining has no negative to pick"""
    p = pids.detach().reshape(-1)
    return p.numel() > 0 and bool((p == p[0]).all())


def single_identity_error():
    """the reference's TripletLoss dies in `.min()` of an empty tensor (hard_mine_triplet_loss.py:42) with a RuntimeError"""
    return RuntimeError("TripletLoss: every row of the batch has the same identity, so no anchor has a negative to mine "
                        "(the reference fails in min() of an empty tensor); sample at least two identities per batch")


def triplet_work_floats(B):
    """workspace of ieee_triplet_hard_fwd_bwd: the B x B squared distances and 5 numbers per anchor"""
    return B * B + 5 * B


class _TripletFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inputs, targets, margin):
        lib = _lib.require_gpu()
        x = inputs.to(torch.float32).contiguous()
        B, D = x.shape
        t = targets.to(device=x.device, dtype=torch.int64).contiguous()
        dx = torch.empty_like(x)
        out = torch.empty(4, dtype=torch.float32, device=x.device)
        work = torch.empty(triplet_work_floats(B), dtype=torch.float32, device=x.device)
        _lib.check(lib.ieee_triplet_hard_fwd_bwd(_lib.ptr(x), 1, _lib.ptr(t), _lib.ptr(dx), _lib.ptr(out), _lib.ptr(work),
                                                 B, D, float(margin), 1.0, 0, _lib.stream()))
        ctx.save_for_backward(dx)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return dx * g, None, None


class TripletLoss(nn.Module):
    """Triplet loss with batch-hard mining (Hermans et al., arXiv:1703.07737), reference hard_mine_triplet_loss.py:6-48:
    mean over anchors of max(0, margin + d(anchor, hardest positive) - d(anchor, hardest negative)).  Distances are formed
    from differences (exactly 0 for equal rows), not from the reference's fp32 Gram expansion; see csrc/metric_loss.hip."""

    def __init__(self, margin=0.3):
        super(TripletLoss, self).__init__()
        self.margin = margin

    def forward(self, inputs, targets):
        assert inputs.dim() == 2 and targets.numel() == inputs.size(0)
        if single_identity(targets.cpu()):
            raise single_identity_error()
        return _TripletFunction.apply(inputs, targets, self.margin)


def DeepSupervision(criterion, xs, y):
    """reference losses/__init__.py:9-44: sum of the criterion over a list of outputs.  When the list is the
    native model's 6 part-logits (views of one [18,B,C] tensor) this is still 6 small launches; the fused
    engine path batches all 18 heads in one."""
    loss = 0.
    for x in xs:
        loss += criterion(x, y)
    return loss
