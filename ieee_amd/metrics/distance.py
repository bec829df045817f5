"""Distance matrices on MI355X.  Same names, arguments and error behaviour as the
reference's torchreid/metrics/distance.py:6-80; the arithmetic runs in
ieee_sqeuclid_distmat (tiled MFMA GEMM with the norm epilogue fused).

`precision` (keyword, or IEEE_DISTMAT_PRECISION; not in the reference) picks the matrix pipe for fp32 inputs:
"fp32" (default) = fp32 MFMA; "bf16x3" = the fp32 rows as three exact bf16 pieces and six piece products on the bf16
matrix cores (fp32-grade accuracy); "f16x2" = two fp16 pieces of the power-of-two-scaled rows and three products
(2^-22 relative, the fastest fp32-grade path); "bf16x2" = two bf16 pieces (~2^-16); "bf16" = round the inputs to bf16."""
import os

import torch

from .. import _lib


def _as_device(x, dtype):
    dev = x.device
    if dev.type != "cuda":
        x = x.cuda(non_blocking=False)
    return x.to(dtype).contiguous(), dev


PRECISIONS = ("fp32", "bf16x3", "f16x2", "bf16x2", "bf16")
_SPLIT_SCHEME = {"bf16x3": 6, "bf16x2": 3, "f16x2": 2}     # IEEE_SPLIT_* in include/ieee_amd.h


def _resolve(precision, input_dtype, compute_dtype=None):
    """-> (precision, compute_dtype): the environment's default, the known values, bf16 for bf16 inputs"""
    if precision is None:
        precision = os.environ.get("IEEE_DISTMAT_PRECISION", "fp32")
    if precision not in PRECISIONS:
        raise ValueError("Unknown distmat precision: {}. Choose one of {}".format(precision, PRECISIONS))
    if compute_dtype is None:
        compute_dtype = torch.bfloat16 if (input_dtype == torch.bfloat16 or precision == "bf16") else torch.float32
    return precision, compute_dtype


def _pad8(x):
    """kernels move 16-byte chunks: pad the feature axis with zeros (changes nothing)"""
    d = x.shape[1]
    return x if d % 8 == 0 else torch.nn.functional.pad(x, (0, 8 - d % 8))


def _workspace_bytes(lib, m, n, d, compute_dtype, precision):
    if compute_dtype == torch.float32 and precision in _SPLIT_SCHEME:
        return lib.ieee_sqeuclid_distmat_split_workspace_bytes(m, n, d, _SPLIT_SCHEME[precision])
    return (m + n) * 4


def _launch(lib, a, b, metric_id, compute_dtype, precision, out, ldo, work):
    """a [m, d], b [n, d]: contiguous device rows of compute_dtype, d % 8 == 0; out: fp32, row stride ldo >= n;
    work: a device buffer of at least _workspace_bytes(...) bytes"""
    (m, d), n = a.shape, b.shape[0]
    if compute_dtype == torch.float32 and precision in _SPLIT_SCHEME:
        _lib.check(lib.ieee_sqeuclid_distmat_split(_lib.ptr(a), _lib.ptr(b), m, n, d, _SPLIT_SCHEME[precision], metric_id,
                                                   _lib.ptr(out), ldo, _lib.ptr(work), work.numel() * work.element_size(),
                                                   _lib.stream()))
        return
    dt = _lib.IEEE_BF16 if compute_dtype == torch.bfloat16 else _lib.IEEE_F32
    _lib.check(lib.ieee_sqeuclid_distmat(_lib.ptr(a), _lib.ptr(b), m, n, d, dt, metric_id, _lib.ptr(out), ldo,
                                         _lib.ptr(work), _lib.stream()))


def _distmat(input1, input2, metric_id, compute_dtype=None, precision=None):
    lib = _lib.require_gpu()
    precision, compute_dtype = _resolve(precision, input1.dtype, compute_dtype)
    a, dev = _as_device(input1, compute_dtype)
    b, _ = _as_device(input2, compute_dtype)
    m, n = a.shape[0], b.shape[0]
    out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    if m == 0 or n == 0:
        return out.to(dev)
    a, b = _pad8(a), _pad8(b)
    work = torch.empty(_workspace_bytes(lib, m, n, a.shape[1], compute_dtype, precision), dtype=torch.uint8, device=a.device)
    _launch(lib, a, b, metric_id, compute_dtype, precision, out, n, work)
    return out if dev.type == "cuda" else out.to(dev)


def compute_distance_matrix(input1, input2, metric='euclidean', precision=None):
    """Reference torchreid/metrics/distance.py:6-46.  CPU inputs are staged through the GPU and the
    result is returned on the inputs' device (the reference's caller, Engine._evaluate, passes CPU
    tensors, engine/engine.py:368-399); CUDA inputs stay on the device."""
    assert isinstance(input1, torch.Tensor)
    assert isinstance(input2, torch.Tensor)
    assert input1.dim() == 2, 'Expected 2-D tensor, but got {}-D'.format(input1.dim())
    assert input2.dim() == 2, 'Expected 2-D tensor, but got {}-D'.format(input2.dim())
    assert input1.size(1) == input2.size(1)

    if metric == 'euclidean':
        distmat = euclidean_squared_distance(input1, input2, precision)
    elif metric == 'cosine':
        distmat = cosine_distance(input1, input2, precision)
    else:
        raise ValueError(
            'Unknown distance metric: {}. '
            'Please choose either "euclidean" or "cosine"'.format(metric)
        )
    return distmat


def _pair_index(idx, rows, name):
    """-> int64 host or device tensor, 1-D, every entry in [0, rows): checked where the indices are"""
    idx = torch.as_tensor(idx)
    if idx.dim() != 1 or idx.dtype.is_floating_point or idx.dtype == torch.bool:
        raise ValueError("pair_distances: {} must be a 1-D integer array, got {} {}".format(name, idx.dtype, tuple(idx.shape)))
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= rows):
        raise ValueError("pair_distances: {} has entries outside [0, {})".format(name, rows))
    return idx


def pair_distances(input1, input2, idx1, idx2, metric='euclidean'):
    """compute_distance_matrix(input1, input2, metric)[idx1, idx2] in fp32 without the matrix: a 1-D fp32 tensor on
    input1's device, entry p the distance of input1[idx1[p]] and input2[idx2[p]] with the bits the matrix has there
    (ieee_distmat_pairs: the pairs go through the matrix GEMM's own MFMA sequence, norms and epilogue).  idx1, idx2:
    1-D integer tensors or arrays of one length, on the host or the device."""
    from ._stream import check_metric
    metric_id = check_metric(metric)
    assert isinstance(input1, torch.Tensor) and isinstance(input2, torch.Tensor)
    if input1.dim() != 2 or input2.dim() != 2 or input1.size(1) != input2.size(1) or not input1.size(0) or not input2.size(0):
        raise ValueError("pair_distances: expected input1 [m, d] and input2 [n, d] with m, n >= 1, got {} and {}".format(
            tuple(input1.shape), tuple(input2.shape)))
    idx1, idx2 = _pair_index(idx1, input1.size(0), "idx1"), _pair_index(idx2, input2.size(0), "idx2")
    if idx1.numel() != idx2.numel():
        raise ValueError("pair_distances: {} row indices for {} column indices".format(idx1.numel(), idx2.numel()))
    lib = _lib.require_gpu()
    a, dev = _as_device(input1, torch.float32)
    b, _ = _as_device(input2, torch.float32)
    a, b = _pad8(a), _pad8(b)
    i1, i2 = idx1.to(a.device, torch.int32).contiguous(), idx2.to(a.device, torch.int32).contiguous()
    out = torch.empty(i1.numel(), dtype=torch.float32, device=a.device)
    work = torch.empty((a.shape[0] + b.shape[0]) * 4, dtype=torch.uint8, device=a.device)
    _lib.check(lib.ieee_distmat_pairs(_lib.ptr(a), _lib.ptr(b), a.shape[0], b.shape[0], a.shape[1], _lib.ptr(i1),
                                      _lib.ptr(i2), i1.numel(), metric_id, _lib.ptr(out), _lib.ptr(work), _lib.stream()))
    return out if dev.type == "cuda" else out.to(dev)


def euclidean_squared_distance(input1, input2, precision=None):
    """distance.py:49-64 — |a|^2 + |b|^2 - 2 a.b (squared, no sqrt)."""
    return _distmat(input1, input2, 0, precision=precision)


def cosine_distance(input1, input2, precision=None):
    """distance.py:67-80 — 1 - a^.b^ with F.normalize's eps of 1e-12."""
    return _distmat(input1, input2, 1, precision=precision)
