"""GPU: the head, loss and optimizer kernels of ieee_amd/csrc/head.hip called through the C ABI the way the executor
(net.hip) calls them -- pointer tables of 3 / 6 / 18 groups, row strides that differ from the channel count, frozen and
eval modes, accumulate flags, unaligned optimizer slices -- against float64 CPU references of the same operation.

Tolerances come from an fp32 forward-error model, written next to each assert: with u = 2^-24, a sum of M terms is off
by at most ~M*u*sum|terms|, a product or quotient adds ~u relative per rounding, and hardware exp / log / sqrt add a few
ulp.  A constant c = 2..4 covers the slack.  Where the kernel's arithmetic is exact (copies, zeroing, bf16 rounding,
skipped updates, accumulate = old + new) the assert is bit equality."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24              # fp32 unit roundoff
MAXG = 18                   # IEEE_MAX_GROUPS
DEV = "cuda"


def _lib():
    from ieee_amd import _lib as L
    return L, L.require_gpu()


def tab(ts):
    """a pointer table (host array of device addresses); ints are raw addresses, None is NULL"""
    return (ctypes.c_void_p * len(ts))(*[0 if t is None else (t if isinstance(t, int) else t.data_ptr()) for t in ts])


def addr(t, floats):
    """the address `floats` fp32 elements past the start of t"""
    return t.data_ptr() + 4 * int(floats)


def within(got, ref, tol, what):
    """|got - ref| <= tol elementwise (float64), with the worst offender in the message"""
    got, ref, tol = got.double().cpu(), ref.double().cpu(), torch.as_tensor(tol, dtype=torch.float64).expand_as(ref)
    assert torch.isfinite(got).all(), "%s: non-finite output" % what
    err = (got - ref).abs()
    bad = err > tol
    if bool(bad.any()):
        i = int(torch.argmax((err - tol).flatten()))
        raise AssertionError("%s: %d elements out of bound; worst at %d: got %r want %r |err| %.3e > tol %.3e" % (
            what, int(bad.sum()), i, float(got.flatten()[i]), float(ref.flatten()[i]), float(err.flatten()[i]),
            float(tol.flatten()[i])))


def bits_equal(a, b):
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    if a.dtype == torch.bfloat16:
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def sentinel_like(shape, device=DEV):
    """a fill no kernel writes: a NaN with a payload (so a stray write of any number shows)"""
    return torch.full(shape, -1, dtype=torch.int32, device=device).view(torch.float32)


# ============================================================================ cross entropy
def _ce_ref(x, y, eps, C):
    """per-row loss, softmax, lse of the label-smoothed CE in float64 (oracle.model.cross_entropy_ls, row-wise)"""
    xd = x.double()
    lse = torch.logsumexp(xd, dim=-1)
    logp = xd - lse[..., None]
    t = torch.full_like(logp, eps / C)
    t.scatter_add_(-1, y.expand(*xd.shape[:-1]).unsqueeze(-1), torch.full(xd.shape[:-1] + (1,), 1.0 - eps, dtype=torch.float64))
    return -(t * logp).sum(-1), logp.exp(), t, lse


def _ce_bounds(x, y, eps, C, lse, rowloss):
    """fp32 error model of ce_rows_kernel:
    lse = mx + log(sum_c exp(x_c - mx)): the C-term sum of exps in (0, 1] is off by (C+4)u relative (exp: ~2 ulp); the
    rounding of x_c - mx moves each exponent by u|x_c - mx| <= 2u max|x|; log and the final add cost u|lse| each.
    rowloss = -(1-eps)(x_y - lse) - (eps/C)(sum_c x_c - C lse): the C-term sum of x adds C u sum|x| / C = u sum|x| after the
    eps/C weight, the rest is a handful of roundings of |lse|, |x_y|, |rowloss|."""
    xd = x.double()
    mxa = xd.abs().amax(-1)
    lse_err = 2 * U * (C + 8 + 2 * mxa + 2 * lse.abs())
    xy = xd.gather(-1, y.expand(*xd.shape[:-1]).unsqueeze(-1)).squeeze(-1)
    row_tol = 2 * (lse_err + eps * U * xd.abs().sum(-1) + 4 * U * (lse.abs() + xy.abs() + rowloss.abs()))
    return lse_err, row_tol


def _ce_run(L, lib, x, y, eps, gs, with_grad=True):
    heads, B, C = x.shape
    xd, yd = x.to(DEV, copy=True), y.to(DEV, copy=True)
    dl = sentinel_like((heads, B, C)) if with_grad else None
    hl, ha = sentinel_like((heads,)), sentinel_like((heads,))
    work = torch.empty(heads * B * 2, device=DEV)
    L.check(lib.ieee_ce_ls_fwd_bwd(L.ptr(xd), L.ptr(yd), L.ptr(dl), L.ptr(hl), L.ptr(ha), L.ptr(work), heads, B, C, eps, gs,
                                   L.stream()))
    torch.cuda.synchronize()
    return hl.cpu(), ha.cpu(), (dl.cpu() if with_grad else None)


def _ce_check(L, lib, x, y, eps, gs, what):
    heads, B, C = x.shape
    hl, ha, dl = _ce_run(L, lib, x, y, eps, gs)
    rowloss, p, t, lse = _ce_ref(x, y, eps, C)
    lse_err, row_tol = _ce_bounds(x, y, eps, C, lse, rowloss)
    # head loss = mean of B row losses: the row bounds, plus a B-term sum (B u sum|row|) and the division
    want = rowloss.mean(-1)
    within(hl, want, row_tol.mean(-1) + (B + 2) * U * rowloss.abs().mean(-1), what + " head_loss")
    # accuracy: 100 * k / B in fp32 (100k is exact), k from torch.argmax (first index among equal maxima)
    k = (x.argmax(-1) == y).sum(-1).numpy().astype(np.float32)
    assert np.array_equal(ha.numpy(), np.float32(100.0) * k / np.float32(B)), what + " head_acc"
    # dlogits = (exp(x - lse) - t) * gs / B: exp of an argument off by lse_err -> p * (lse_err + 3u) absolute, plus the
    # rounding of t (eps/C), the difference and the two scalings
    sc = gs / B
    want_d = (p - t) * sc
    tol_d = abs(sc) * (2 * p * (lse_err[..., None] + 3 * U) + 4 * U * (p + t)) + 4 * U * want_d.abs()
    within(dl, want_d, tol_d, what + " dlogits")
    return hl, ha


def test_ce_ls_shapes_eps_and_grad_scale():
    L, lib = _lib()
    g = torch.Generator().manual_seed(101)
    for heads in (1, 18):
        for B in (1, 64):
            for C in (1, 63, 64, 65, 171, 750, 1000):
                x = torch.randn(heads, B, C, generator=g) * 3
                y = torch.randint(0, C, (B,), generator=g)
                if C > 1 and B > 1:        # some rows predicted right, so head_acc is not trivially 0
                    x[:, : B // 2].scatter_(-1, y[: B // 2].expand(heads, -1).unsqueeze(-1), 12.0)
                for eps in (0.0, 0.1):
                    for gs in (1.0, 0.37):
                        _ce_check(L, lib, x, y, eps, gs, "heads=%d B=%d C=%d eps=%g gs=%g" % (heads, B, C, eps, gs))


def test_ce_ls_large_logit_offset_and_no_grad_buffer():
    """x + 1e4: softmax is unchanged, so only the max subtraction keeps exp() finite; the bound scales with max|x|
    (the 2u max|x| term of _ce_bounds).  dlogits = NULL gives the same loss and accuracy bits."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(102)
    for C in (65, 171, 1000):
        x = torch.randn(18, 64, C, generator=g) * 2
        y = torch.randint(0, C, (64,), generator=g)
        hl0, _ = _ce_check(L, lib, x, y, 0.1, 1.0, "C=%d" % C)
        hl1, ha1 = _ce_check(L, lib, x + 1e4, y, 0.1, 1.0, "C=%d shifted" % C)
        # the shifted loss is the unshifted one (the reference's own values agree to fp64 rounding)
        within(hl1, hl0, 2 * U * (C + 8 + 4e4) * 2 + 1e-6, "C=%d shift invariance" % C)
        hl2, ha2, _ = _ce_run(L, lib, x + 1e4, y, 0.1, 1.0, with_grad=False)
        assert bits_equal(hl2, hl1) and bits_equal(ha2, ha1)


def test_ce_ls_argmax_ties_go_to_the_first_index():
    """exact ties of the row maximum at positions in different lanes (c, c+1, c+37) and in the same lane (c, c+64): the
    kernel's wave arg-max must pick the smallest index, as torch.argmax; half the rows have their label on the later copy"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(103)
    for C in (65, 171, 750):
        B, heads = 64, 18
        x = torch.randn(heads, B, C, generator=g)
        y = torch.empty(B, dtype=torch.long)
        for b in range(B):
            c = int(torch.randint(0, C - 64, (1,), generator=g))
            copies = [c, c + (1, 37, 64)[b % 3]]
            x[:, b, copies] = 9.0
            y[b] = copies[b % 2]
        # small-integer logits: ties among many entries of a row
        xi = torch.randint(-3, 4, (heads, B, C), generator=g).float()
        for xx in (x, xi):
            _, ha = _ce_check(L, lib, xx, y, 0.1, 1.0, "ties C=%d" % C)
            assert float(ha.max()) > 0 or xx is xi


# ============================================================================ 3M margin loss
def _margin_ref(f, pids, margin):
    """float64 reference over the chunks torch.chunk yields (oracle.model.margin3m when there are enough of them; the
    same loop over the existing chunks otherwise -- what the kernel reports next to the reference's IndexError)"""
    from oracle import model as om
    fd = [t.double().clone().requires_grad_(True) for t in f]
    n = len(pids.unique())
    chunks = fd[0].chunk(n, 0)
    if len(chunks) >= n:
        loss = om.margin3m(fd[0], fd[1], fd[2], pids, margin)
    else:
        c1, c2, c3 = fd[0].chunk(n, 0), fd[1].chunk(n, 0), fd[2].chunk(n, 0)
        loss = 0
        for i in range(len(c1)):
            a, b, c = c1[i].mean(0), c2[i].mean(0), c3[i].mean(0)
            d = lambda u_, v_: ((u_ - v_) ** 2).sum()
            loss = loss + max(abs(margin - d(a, b)), abs(margin - d(b, c)), abs(margin - d(a, c)))
    loss.backward()
    return float(loss.detach()), [t.grad if t.grad is not None else torch.zeros_like(t) for t in fd], n, len(chunks)


def _margin_run(L, lib, f, pids, margin, gs):
    B, D = f[0].shape
    feats = torch.stack(f).to(DEV, copy=True).contiguous()
    df = sentinel_like((3, B, D))
    out3 = sentinel_like((3,))
    work = torch.empty(B + 3, device=DEV)
    pd_ = pids.to(DEV, copy=True)
    L.check(lib.ieee_margin3m_fwd_bwd(L.ptr(feats), L.ptr(pd_), L.ptr(df), L.ptr(out3), L.ptr(work), B, D, margin, gs,
                                      L.stream()))
    torch.cuda.synchronize()
    return out3.cpu(), df.cpu()


def _margin_bounds(f, pids, margin):
    """fp32 error model of margin3m_kernel, per chunk of `rows` rows: a center is a rows-term sum / rows (err (rows+2)u
    mean|f|); a distance is a D-term sum of squared differences (err (D+2 rows+8)u sum_k (|c_a|+|c_b|)^2); the loss adds
    nchunks terms.  The gradient of a row is 2 gs (c_a - c_b) / rows: err (rows+4)u (|c_a|+|c_b|) / rows relative to it."""
    B, D = f[0].shape
    n = len(pids.unique())
    fd = [t.double() for t in f]
    loss_tol, grad_tol, gaps = 0.0, [torch.zeros(B, D, dtype=torch.float64) for _ in range(3)], []
    per = -(-B // n)
    for r0 in range(0, B, per):
        rows = min(B, r0 + per) - r0
        c = [t[r0:r0 + rows].mean(0) for t in fd]
        ca = [t[r0:r0 + rows].abs().mean(0) for t in fd]
        pairs = ((0, 1), (1, 2), (0, 2))
        dt = [float(((ca[a] + ca[b]) ** 2).sum()) * 2 * (D + 2 * rows + 8) * U for a, b in pairs]
        dv = [float(((c[a] - c[b]) ** 2).sum()) for a, b in pairs]
        loss_tol += max(dt) + 4 * U * max(abs(margin - d) for d in dv)
        s = sorted(abs(margin - d) for d in dv)
        t_ = max(dt)
        gaps.append((r0, rows, s[2] - s[1] > 4 * t_ and s[2] > 4 * t_))      # the pair, and the sign of its m - d
        for m in range(3):
            for a, b in pairs:
                if m in (a, b):
                    grad_tol[m][r0:r0 + rows] = torch.maximum(grad_tol[m][r0:r0 + rows], 4 * (rows + 4) * U * (ca[a] + ca[b]) / rows)
    return loss_tol * 2, grad_tol, gaps


def _margin_feats(B, D, pids, g):
    """per chunk, the three modality centers sit at 0, 1 and 3 half-units along a random direction (permuted per chunk, so
    every pair gets selected) plus small noise: the distances are ~0.25, 1 and 2.25 -- far apart against the fp32 bound,
    so the selected pair and the sign of m - d are decided by the data, not by rounding"""
    n = len(pids.unique())
    per = -(-B // n)
    v = (torch.randint(0, 2, (D,), generator=g).double() * 2 - 1) / D ** 0.5
    f = [torch.empty(B, D) for _ in range(3)]
    for r0 in range(0, B, per):
        rows = min(B, r0 + per) - r0
        perm = torch.randperm(3, generator=g)
        for m in range(3):
            off = (0.0, 1.0, 3.0)[int(perm[m])] * 0.5
            f[m][r0:r0 + rows] = (off * v + torch.randn(rows, D, generator=g, dtype=torch.float64) * 0.02 / D ** 0.5).float()
    return f


@pytest.mark.parametrize("D", [1, 100, 255, 256, 257, 768, 2048])
def test_margin3m_dims_batches_and_identity_layouts(D):
    """ragged D against the 256-thread k stride; identities sorted, interleaved ([0,1,0,1,...]: the reference chunks by
    POSITION, not by identity) and non-contiguous values; grad_scale 1 and 0.37"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(200 + D)
    for B in (1, 4, 10, 32, 64):
        layouts = {"sorted": torch.arange(B) // 4, "interleaved": torch.arange(B) % 2,
                   "sparse": (torch.arange(B) // 4) * 7919 + 3}
        for name, pids in layouts.items():
            f = _margin_feats(B, D, pids, g)
            for margin, gs in ((1.0, 1.0), (3.0, 0.37)):    # m - d < 0 for the selected pair, then > 0
                what = "D=%d B=%d %s margin=%g gs=%g" % (D, B, name, margin, gs)
                out3, df = _margin_run(L, lib, f, pids, margin, gs)
                loss, grads, n, nch = _margin_ref(f, pids, margin)
                loss_tol, grad_tol, gaps = _margin_bounds(f, pids, margin)
                assert out3[1] == n and out3[2] == nch, what
                within(out3[0:1], torch.tensor([loss]), loss_tol, what + " loss")
                # the gradient of a chunk is compared where the selected pair and the sign of m - d are decided well
                # outside the error bound (random data: almost every chunk)
                rows_ok = torch.zeros(B, dtype=torch.bool)
                for r0, rows, ok in gaps:
                    rows_ok[r0:r0 + rows] = ok
                assert bool(rows_ok.all()), what + ": near-ties in the data"
                assert not bool(df.isnan().any()), what + ": dfeats not written"
                for m in range(3):
                    within(df[m][rows_ok], grads[m][rows_ok] * gs, (grad_tol[m] * gs + 4 * U * (grads[m] * gs).abs())[rows_ok],
                           what + " dfeats[%d]" % m)


def test_margin3m_short_chunks_report_and_cover_every_row():
    """10 rows of 6 identities: torch.chunk(6) yields 5 pieces of 2 and the reference raises IndexError.  The kernel
    reports label_num = 6 and 5 chunks in out3[1..2], sums the 5 terms, and writes every row of dfeats (the buffer is
    pre-filled with a NaN sentinel).  Since ceil(B / ceil(B / n)) <= n, torch.chunk never yields MORE pieces than the
    kernel uses, so there are no rows beyond the used chunks: all 10 get the reference's gradient."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(210)
    for B, pids in ((10, torch.tensor([0, 0, 1, 1, 2, 2, 3, 3, 4, 5])), (7, torch.tensor([9, 8, 7, 6, 5, 4, 4])),
                    (64, torch.arange(64) // 2 % 23)):
        D = 257
        f = _margin_feats(B, D, pids, g)
        out3, df = _margin_run(L, lib, f, pids, 1.0, 1.0)
        loss, grads, n, nch = _margin_ref(f, pids, 1.0)
        assert nch < n and float(out3[1]) == n and float(out3[2]) == nch
        loss_tol, grad_tol, _ = _margin_bounds(f, pids, 1.0)
        within(out3[0:1], torch.tensor([loss]), loss_tol, "short chunks B=%d loss" % B)
        for m in range(3):
            within(df[m], grads[m], grad_tol[m] + 4 * U * grads[m].abs(), "short chunks B=%d dfeats[%d]" % (B, m))


def test_margin3m_tie_keeps_the_first_pair():
    """f3 := f1 bitwise: d(1,2) and d(2,3) are computed from the same bits in the same order, so |m - d(1,2)| equals
    |m - d(2,3)| exactly, and with d > 2m both beat |m - d(1,3)| = m.  Python's max keeps the first: pair (1,2) -- the
    gradient goes to modalities 1 and 2, modality 3 gets exact zeros."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(220)
    for B, D in ((8, 768), (64, 257), (10, 100)):
        pids = torch.arange(B) // 2
        f1 = torch.randn(B, D, generator=g)
        f2 = torch.randn(B, D, generator=g) + 1.0
        out3, df = _margin_run(L, lib, [f1, f2, f1.clone()], pids, 1.0, 0.5)
        loss, grads, _, _ = _margin_ref([f1, f2, f1.clone()], pids, 1.0)
        assert float(df[2].abs().max()) == 0.0 and float(grads[2].abs().max()) == 0.0
        assert float(df[0].abs().min()) > 0 and float(df[1].abs().min()) > 0
        assert torch.equal(df[0], -df[1])
        loss_tol, grad_tol, _ = _margin_bounds([f1, f2, f1], pids, 1.0)
        within(out3[0:1], torch.tensor([loss]), loss_tol, "tie loss")
        for m in range(2):
            within(df[m], grads[m] * 0.5, grad_tol[m] * 0.5 + 4 * U * grads[m].abs(), "tie dfeats[%d]" % m)


# ============================================================================ row-wise BatchNorm
def _bn_stats_tol(x, R):
    """fp32 error model of the statistics (two passes over R rows, 16 lanes then a 16-term sum): mean off by (R+4)u
    mean|x|; the centered variance off by 2(R+8)u relative (the mean's error enters only at second order); invstd by
    half of that plus 2 roundings"""
    mean_err = (R + 4) * U * x.abs().mean(0)
    var_rel = 2 * (R + 8) * U
    return mean_err, var_rel


def _rowbn_case(L, lib, groups, R, C, ldx, ldo, relu, training, g, what, frozen_bwd=False, place=None):
    """one forward + backward of `groups` problems laid out like the executor's: x rows ldx apart; out (and dout) rows ldo
    apart in a buffer of `nblk` blocks of R rows, problem i at (block, column) = place[i] (default: a block each, column 0),
    against F.batch_norm + relu autograd in float64.  Every output element outside the problems keeps its sentinel bits."""
    place = place or [(i, 0) for i in range(groups)]
    nblk = 1 + max(b for b, _ in place)
    assert ldx >= C and all(c + C <= ldo for _, c in place)
    xs = [torch.randn(R, ldx, generator=g) * 1.5 + torch.randn(1, ldx, generator=g) for _ in range(groups)]
    gam = [torch.rand(C, generator=g) + 0.5 for _ in range(groups)]
    bet = [torch.randn(C, generator=g) * 0.3 for _ in range(groups)]
    rm0 = [torch.randn(C, generator=g) * 0.2 for _ in range(groups)]
    rv0 = [torch.rand(C, generator=g) + 0.5 for _ in range(groups)]
    xd = [t.to(DEV, copy=True) for t in xs]
    ga_d, be_d = [t.to(DEV, copy=True) for t in gam], [t.to(DEV, copy=True) for t in bet]
    rm_d, rv_d = [t.to(DEV, copy=True) for t in rm0], [t.to(DEV, copy=True) for t in rv0]
    sv = [torch.empty(2, C, device=DEV) for _ in range(groups)]
    obuf = sentinel_like((nblk, R, ldo))
    optr = [addr(obuf, b * R * ldo + c) for b, c in place]
    covered = torch.zeros(nblk, R, ldo, dtype=torch.bool)
    for b, c in place:
        covered[b, :, c:c + C] = True
    L.check(lib.ieee_rowbn_fwd(groups, tab(xd), tab(optr), tab(ga_d), tab(be_d), tab(rm_d), tab(rv_d), tab(sv), R, C, ldx, ldo,
                               0.1, 1e-5, training, 1 if relu else 0, L.stream()))
    torch.cuda.synchronize()
    ob = obuf.cpu()
    out = [ob[b, :, c:c + C] for b, c in place]
    # gaps between strided rows keep their bits
    gap = ob[~covered]
    assert bits_equal(gap, sentinel_like(gap.shape, "cpu")), what + ": write outside the output rows"
    dbuf_rows = []
    for i in range(groups):
        x = xs[i][:, :C].double().requires_grad_(True)
        ga, be = gam[i].double().requires_grad_(True), bet[i].double().requires_grad_(True)
        rm, rv = rm0[i].double().clone(), rv0[i].double().clone()
        pre = F.batch_norm(x, rm, rv, ga, be, bool(training), 0.1, 1e-5)
        ref = F.relu(pre) if relu else pre
        xc = xs[i][:, :C].double()
        if training:
            mu, var = xc.mean(0), xc.var(0, unbiased=False)
        else:
            mu, var = rm0[i].double(), rv0[i].double()
        invstd = (var + 1e-5).rsqrt()
        xh = (xc - mu) * invstd
        mean_err, var_rel = _bn_stats_tol(xc, R) if training else (0.0 * mu, 0.0)
        # out = (x - mean) invstd gamma + beta: the statistics' error through |gamma| invstd, plus 4 roundings
        tol = ga.detach().abs() * invstd * (mean_err + 2 * U * (xc - mu).abs()) + \
            (ga.detach() * xh).abs() * (var_rel / 2 + 3 * U) + 4 * U * (ref.detach().abs() + be.detach().abs())
        within(out[i], ref.detach(), 2 * tol, "%s fwd group %d" % (what, i))
        if training:
            # running stats: (1-m) r + m stat with the unbiased variance R/(R-1) var
            within(rm_d[i], rm, 2 * (0.1 * mean_err + 3 * U * (rm.abs() + 0.1 * mu.abs())), "%s running_mean %d" % (what, i))
            within(rv_d[i], rv, 2 * (0.1 * var_rel * var * R / (R - 1) + 4 * U * rv.abs()), "%s running_var %d" % (what, i))
        else:
            assert bits_equal(rm_d[i], rm0[i]) and bits_equal(rv_d[i], rv0[i])
        # backward: dout zero where the pre-activation is within 0.02 of the ReLU kink (both sides then mask alike)
        dout = torch.randn(R, C, generator=g)
        if relu:
            dout = dout * (pre.detach().abs() > 0.02)
        ref.backward(dout.double())
        dbuf_rows.append((x.grad, ga.grad, be.grad, dout, xh, invstd, mean_err, var_rel, ga.detach()))
    # device backward: dout rows ldo apart in a buffer laid out like the output, dx rows ldx apart
    dob = torch.zeros_like(obuf)
    for i, (b, c) in enumerate(place):
        dob[b, :, c:c + C] = dbuf_rows[i][3].to(DEV, copy=True)
    dptr = [addr(dob, b * R * ldo + c) for b, c in place]
    dxb = [sentinel_like((R, ldx)) for _ in range(groups)]
    dg0 = [torch.randn(C, generator=g).to(DEV, copy=True) for _ in range(groups)]
    db0 = [torch.randn(C, generator=g).to(DEV, copy=True) for _ in range(groups)]
    dg, db = [t.clone() for t in dg0], [t.clone() for t in db0]
    relu_flag = (3 if frozen_bwd else 1) if relu else (2 if frozen_bwd else 0)
    L.check(lib.ieee_rowbn_bwd(groups, tab(dptr), tab(optr), tab(xd), tab(ga_d), tab(sv), tab(dxb), tab(dg), tab(db), R, C, ldo,
                               ldo, ldx, ldx, relu_flag, 0, L.stream()))
    torch.cuda.synchronize()
    for i in range(groups):
        dx_ref, dga_ref, dbe_ref, dout, xh, invstd, mean_err, var_rel, ga = dbuf_rows[i]
        dxc = dxb[i].cpu()
        assert bits_equal(dxc[:, C:], sentinel_like((R, ldx - C), "cpu")), what + ": dx written outside its rows"
        gq = dout.double()
        m1, m2 = gq.abs().mean(0), (gq * xh).abs().mean(0)
        dxh = mean_err * invstd + xh.abs() * var_rel / 2          # error of the kernel's xhat
        if frozen_bwd:
            # dx = gamma invstd g: invstd = 1/sqrt(rv + eps) (3 roundings) and the two products
            tol = 6 * U * dx_ref.abs()
            assert bits_equal(dg[i], dg0[i]) and bits_equal(db[i], db0[i]), what + ": frozen BN wrote dgamma/dbeta"
        else:
            # dx = gamma invstd (g - s1/R - xhat s2/R): s1, s2 are R-term sums, xhat carries dxh
            tol = ga * invstd * (4 * U * gq.abs() + (R + 8) * U * (m1 + xh.abs() * m2) + dxh * m2 + xh.abs() * (gq.abs() * dxh).mean(0)) + \
                dx_ref.abs() * (var_rel + 4 * U)
            within(dg[i], dga_ref, 2 * ((R + 8) * U * (gq * xh).abs().sum(0) + (gq.abs() * dxh).sum(0)), "%s dgamma %d" % (what, i))
            within(db[i], dbe_ref, 2 * (R + 8) * U * gq.abs().sum(0), "%s dbeta %d" % (what, i))
        within(dxc[:, :C], dx_ref, 2 * tol, "%s dx %d" % (what, i))


def test_rowbn_executor_layouts():
    L, lib = _lib()
    g = torch.Generator().manual_seed(300)
    D, R = 128, 768
    featcat = [(m, i * D) for m in range(3) for i in range(6)]             # [3][B][R], head (m, i) at column i*D
    fc_all = [(0, (R, 2 * R, 0)[m] + i * D) for m in range(3) for i in range(6)]   # eval: cat([T, R, N]) rows of 3R
    # the 18 fc heads, training: x [B][D] each, out into featcat rows of R = 768 (6 heads per modality)
    _rowbn_case(L, lib, 18, 64, D, D, R, True, 1, g, "18 heads train", place=featcat)
    # eval: statistics from the running buffers, out into fc_all rows of 3R; the backward the executor runs after a
    # forward on running statistics is the frozen one (relu = 3: a fixed affine map, dgamma / dbeta not written)
    _rowbn_case(L, lib, 18, 64, D, D, 3 * R, True, 0, g, "18 heads eval", frozen_bwd=True, place=fc_all)
    # one modality frozen (6 groups, eval statistics in the training forward)
    _rowbn_case(L, lib, 6, 64, D, D, R, True, 0, g, "6 heads frozen", frozen_bwd=True, place=featcat[6:12])
    # the reduce layer over the parts: 3 groups of 384 rows x 768
    _rowbn_case(L, lib, 3, 384, R, R, R, True, 1, g, "reduce parts")
    # a ragged channel count with strides > C on both sides, no ReLU, and gaps between rows that must keep their bits
    _rowbn_case(L, lib, 3, 64, D, 3 * 64, 200, True, 1, g, "C=128 ldx=3R")
    _rowbn_case(L, lib, 3, 64, 200, 208, 256, False, 1, g, "ragged C=200")
    _rowbn_case(L, lib, 6, 384, 200, 256, 208, False, 0, g, "ragged C=200 eval", frozen_bwd=True)


def test_rowbn_reduce_layer_pair_shares_gamma_and_running_stats():
    """net.hip's reduce layer: BatchNorm1d(768)+ReLU applied to the parts [6B rows] and then to the global vector [B rows]
    with ONE gamma / beta / running buffer pair.  Forward: the running statistics take both updates in order.  Backward:
    parts first (dgamma / dbeta overwritten, accumulate = 0), then the global vector (accumulate = 1).  Against one
    float64 nn.BatchNorm1d module applied twice."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(310)
    B, R, G = 64, 768, 3
    PB = 6 * B
    xp = torch.randn(G, PB, R, generator=g) * 2 + 0.3
    xg = torch.randn(G, B, R, generator=g) * 0.5 - 0.2
    gam, bet = torch.rand(G, R, generator=g) + 0.5, torch.randn(G, R, generator=g) * 0.2
    rm0, rv0 = torch.randn(G, R, generator=g) * 0.1, torch.rand(G, R, generator=g) + 0.5
    dop = torch.randn(G, PB, R, generator=g)
    dog = torch.randn(G, B, R, generator=g)
    refs = []
    for m in range(G):
        bn = torch.nn.BatchNorm1d(R, eps=1e-5, momentum=0.1).double()
        with torch.no_grad():
            bn.weight.copy_(gam[m]); bn.bias.copy_(bet[m]); bn.running_mean.copy_(rm0[m]); bn.running_var.copy_(rv0[m])
        a = xp[m].double().requires_grad_(True)
        b = xg[m].double().requires_grad_(True)
        pa, pb = bn(a), bn(b)
        oa, ob = F.relu(pa), F.relu(pb)
        ka, kb = (pa.detach().abs() > 0.02), (pb.detach().abs() > 0.02)
        dop[m] *= ka
        dog[m] *= kb
        # the parts' backward alone (what the first, overwriting call must leave), then both
        ga1, gb1 = torch.autograd.grad(oa, (bn.weight, bn.bias), dop[m].double(), retain_graph=True)
        (oa * dop[m].double()).sum().add((ob * dog[m].double()).sum()).backward()
        refs.append(dict(oa=oa.detach(), ob=ob.detach(), rm=bn.running_mean.clone(), rv=bn.running_var.clone(),
                         dxa=a.grad, dxb=b.grad, dg=bn.weight.grad.clone(), dbe=bn.bias.grad.clone(), dg1=ga1, db1=gb1))
    d = lambda t: [x.to(DEV, copy=True).contiguous() for x in t]
    xpd, xgd, gad, bed, rmd, rvd = d(xp), d(xg), d(gam), d(bet), d(rm0), d(rv0)
    op, og = [torch.empty(PB, R, device=DEV) for _ in range(G)], [torch.empty(B, R, device=DEV) for _ in range(G)]
    s1, s2 = [torch.empty(2, R, device=DEV) for _ in range(G)], [torch.empty(2, R, device=DEV) for _ in range(G)]
    L.check(lib.ieee_rowbn_fwd(G, tab(xpd), tab(op), tab(gad), tab(bed), tab(rmd), tab(rvd), tab(s1), PB, R, R, R, 0.1, 1e-5, 1, 1,
                               L.stream()))
    L.check(lib.ieee_rowbn_fwd(G, tab(xgd), tab(og), tab(gad), tab(bed), tab(rmd), tab(rvd), tab(s2), B, R, R, R, 0.1, 1e-5, 1, 1,
                               L.stream()))
    dxa, dxb = [torch.empty(PB, R, device=DEV) for _ in range(G)], [torch.empty(B, R, device=DEV) for _ in range(G)]
    dg, db = [torch.full((R,), 7.0, device=DEV) for _ in range(G)], [torch.full((R,), 7.0, device=DEV) for _ in range(G)]
    dopd, dogd = d(dop), d(dog)
    L.check(lib.ieee_rowbn_bwd(G, tab(dopd), tab(op), tab(xpd), tab(gad), tab(s1), tab(dxa), tab(dg), tab(db), PB, R, R, R, R, R,
                               1, 0, L.stream()))
    torch.cuda.synchronize()
    dg1, db1 = [t.clone() for t in dg], [t.clone() for t in db]
    L.check(lib.ieee_rowbn_bwd(G, tab(dogd), tab(og), tab(xgd), tab(gad), tab(s2), tab(dxb), tab(dg), tab(db), B, R, R, R, R, R,
                               1, 1, L.stream()))
    torch.cuda.synchronize()
    for m in range(G):
        r = refs[m]
        xa, xb = xp[m].double(), xg[m].double()
        ea, va = _bn_stats_tol(xa, PB)
        eb, vb = _bn_stats_tol(xb, B)
        mua, mub = xa.mean(0), xb.mean(0)
        vara, varb = xa.var(0, unbiased=False), xb.var(0, unbiased=False)
        # running stats after two updates: the second scales the first's error by 0.9
        rm_tol = 2 * (0.09 * ea + 0.1 * eb + 6 * U * (r["rm"].abs() + 0.1 * mua.abs() + 0.1 * mub.abs()))
        rv_tol = 2 * (0.09 * va * vara * PB / (PB - 1) + 0.1 * vb * varb * B / (B - 1) + 6 * U * r["rv"].abs())
        within(rmd[m], r["rm"], rm_tol, "running_mean %d" % m)
        within(rvd[m], r["rv"], rv_tol, "running_var %d" % m)
        for got, want, x, e, v, rows in ((op[m], r["oa"], xa, ea, va, PB), (og[m], r["ob"], xb, eb, vb, B)):
            mu, var = x.mean(0), x.var(0, unbiased=False)
            invstd = (var + 1e-5).rsqrt()
            tol = gam[m].double() * invstd * (e + 2 * U * (x - mu).abs()) + (gam[m].double() * (x - mu) * invstd).abs() * (v / 2 + 3 * U) + \
                4 * U * (want.abs() + bet[m].double().abs())
            within(got, want, 2 * tol, "reduce fwd %d rows=%d" % (m, rows))
        # the first call overwrote the 7.0 fill; the second added its sums to that
        ga_, gb_ = dop[m].double(), dog[m].double()
        xha, xhb = (xa - mua) * (vara + 1e-5).rsqrt(), (xb - mub) * (varb + 1e-5).rsqrt()
        dxha, dxhb = ea * (vara + 1e-5).rsqrt() + xha.abs() * va / 2, eb * (varb + 1e-5).rsqrt() + xhb.abs() * vb / 2
        tga = (PB + 8) * U * (ga_ * xha).abs().sum(0) + (ga_.abs() * dxha).sum(0)
        tgb = (B + 8) * U * (gb_ * xhb).abs().sum(0) + (gb_.abs() * dxhb).sum(0)
        within(dg1[m], r["dg1"], 2 * tga, "dgamma after the overwriting call %d" % m)
        within(db1[m], r["db1"], 2 * (PB + 8) * U * ga_.abs().sum(0), "dbeta after the overwriting call %d" % m)
        within(dg[m], r["dg"], 2 * (tga + tgb + U * r["dg"].abs()), "dgamma accumulated %d" % m)
        within(db[m], r["dbe"], 2 * ((PB + 8) * U * ga_.abs().sum(0) + (B + 8) * U * gb_.abs().sum(0) + U * r["dbe"].abs()),
               "dbeta accumulated %d" % m)
        for got, want, gq, xh, dxh, var, rows in ((dxa[m], r["dxa"], ga_, xha, dxha, vara, PB), (dxb[m], r["dxb"], gb_, xhb, dxhb, varb, B)):
            invstd = (var + 1e-5).rsqrt()
            m1, m2 = gq.abs().mean(0), (gq * xh).abs().mean(0)
            v = 2 * (rows + 8) * U
            tol = gam[m].double() * invstd * (4 * U * gq.abs() + (rows + 8) * U * (m1 + xh.abs() * m2) + dxh * m2 +
                                              xh.abs() * (gq.abs() * dxh).mean(0)) + want.abs() * (v + 4 * U)
            within(got, want, 2 * tol, "reduce dx %d rows=%d" % (m, rows))


# ============================================================================ column sums, span zeroing
def test_colsum_grouped_strided_and_accumulate():
    L, lib = _lib()
    g = torch.Generator().manual_seed(400)
    for groups, M, N, ldx in ((3, 64, 768, 768 + 5), (18, 64, 171, 200), (18, 64, 128, 768), (3, 1, 1, 3), (7, 33, 129, 130)):
        X = [torch.randn(M, ldx, generator=g) for _ in range(groups)]
        Xd = [t.to(DEV, copy=True) for t in X]
        for acc in (0, 1):
            base = [torch.randn(N + 3, generator=g) for _ in range(groups)]
            out = [t.to(DEV, copy=True) for t in base]
            L.check(lib.ieee_colsum_grouped(groups, tab(Xd), tab(out), M, N, ldx, acc, L.stream()))
            torch.cuda.synchronize()
            for i in range(groups):
                o = out[i].cpu()
                want = X[i][:, :N].double().sum(0) + (base[i][:N].double() if acc else 0)
                # an M-term serial sum (+ one add of the old value): (M+2) u sum|terms|
                tol = (M + 2) * U * (X[i][:, :N].double().abs().sum(0) + (base[i][:N].double().abs() if acc else 0))
                within(o[:N], want, 2 * tol, "colsum G=%d M=%d N=%d ldx=%d acc=%d" % (groups, M, N, ldx, acc))
                assert bits_equal(o[N:], base[i][N:]), "colsum wrote past N"


def test_zero_spans_odd_lengths_and_offsets():
    L, lib = _lib()
    g = torch.Generator().manual_seed(410)
    for count in (1, 6, MAXG):
        lens = [int(v) | 1 for v in torch.randint(1, 3000, (count,), generator=g)]
        if count == 6:
            lens[2] = 2048 * 256 * 2 + 1            # more than the grid cap: the grid-stride loop turns
        offs = [int(v) | 1 for v in torch.randint(1, 64, (count,), generator=g)]
        total = sum(o + n for o, n in zip(offs, lens)) + 7
        host = torch.randn(total, generator=g)
        buf = host.to(DEV, copy=True)
        ptrs, pos, spans = [], 0, []
        for o, n in zip(offs, lens):
            pos += o
            ptrs.append(addr(buf, pos))
            spans.append((pos, n))
            pos += n
        nn_ = (ctypes.c_int64 * count)(*lens)
        L.check(lib.ieee_zero_spans(count, tab(ptrs), nn_, L.stream()))
        torch.cuda.synchronize()
        want = host.clone()
        for p, n in spans:
            want[p:p + n] = 0.0
        got = buf.cpu()
        assert bits_equal(got, want), "zero_spans count=%d" % count


# ============================================================================ REM, CA mix, sigmoid
def test_rem_fwd_bwd_strided_param():
    L, lib = _lib()
    g = torch.Generator().manual_seed(500)
    B, parts, D, pgs, ggs = 64, 6, 768, 5, 3
    part = torch.randn(3, B, parts, D, generator=g)
    r = torch.randn(3, B, D, generator=g)
    pbuf = torch.randn(3 * pgs, generator=g)
    param = pbuf[::pgs].clone()
    pd_, rd, pbd = part.to(DEV, copy=True), r.to(DEV, copy=True), pbuf.to(DEV, copy=True)
    out = torch.empty_like(pd_)
    L.check(lib.ieee_rem_fwd(L.ptr(pd_), L.ptr(rd), L.ptr(pbd), pgs, L.ptr(out), B, parts, D, L.stream()))
    ref = part.double() + 2 * param.double().view(3, 1, 1, 1) * r.double().unsqueeze(2)
    # part + (2 p) r: 2p is exact, then one product and one sum rounding
    within(out, ref, U * (ref.abs() + (2 * param.double().view(3, 1, 1, 1) * r.double().unsqueeze(2)).abs()), "rem fwd")
    do = torch.randn(3, B, parts, D, generator=g)
    dr, work = torch.empty_like(rd), torch.empty(3 * B, device=DEV)
    gbuf = torch.randn(3 * ggs, generator=g)
    for acc in (0, 1):
        gd = gbuf.to(DEV, copy=True)
        dod = do.to(DEV, copy=True)
        L.check(lib.ieee_rem_bwd(L.ptr(dod), L.ptr(rd), L.ptr(pbd), pgs, L.ptr(dr), L.ptr(gd), ggs, L.ptr(work), B, parts, D,
                                 acc, L.stream()))
        torch.cuda.synchronize()
        S = do.double().sum(2)                                    # [3][B][D]
        # dr = 2p * (a parts-term sum): (parts+2) u |2p| sum|dout|
        within(dr, 2 * param.double().view(3, 1, 1) * S, (parts + 2) * U * 2 * param.double().abs().view(3, 1, 1) * do.double().abs().sum(2),
               "rem dr")
        # dparam = 2 sum_b sum_k r * sum_i dout: parts + D/256 + 8 + B levels of summation over |terms|
        terms = (do.double().abs().sum(2) * r.double().abs()).sum((1, 2))
        dp = 2 * (S * r.double()).sum((1, 2))
        gcpu = gd.cpu()
        within(gcpu[::ggs], dp + (gbuf[::ggs].double() if acc else 0), 2 * (parts + D // 256 + 8 + B + 2) * U * 2 * terms, "rem dparam acc=%d" % acc)
        if acc:
            assert bits_equal(gcpu[::ggs], gbuf[::ggs] + first), "accumulate = old + the non-accumulating result"
        else:
            first = gcpu[::ggs].clone()
        mask = torch.ones(3 * ggs, dtype=torch.bool)
        mask[::ggs] = False
        assert bits_equal(gcpu[mask], gbuf[mask]), "rem dparam wrote between the strided slots"


def test_ca_mix_and_sigmoid_at_kinks_and_saturation():
    L, lib = _lib()
    g = torch.Generator().manual_seed(510)
    B, hid = 64, 96
    h = torch.randn(3, 2 * B, hid, generator=g)
    h[:, ::3, ::4] = 0.0                     # the ReLU kink exactly
    h[:, 1::5, 1::4] = -0.0
    h[:, 2::7] = torch.tensor([2e-38, -2e-38, 100.0, -100.0]).repeat(hid // 4)
    hd = h.to(DEV, copy=True)
    hs = torch.empty(3, B, hid, device=DEV)
    L.check(lib.ieee_ca_mix_fwd(L.ptr(hd), L.ptr(hs), B, hid, L.stream()))
    assert bits_equal(hs, h[:, :B] + h[:, B:]), "ca_mix_fwd: one fp32 add"
    dhs = torch.randn(3, B, hid, generator=g)
    dh = sentinel_like((3, 2 * B, hid))
    dhsd = dhs.to(DEV, copy=True)
    L.check(lib.ieee_ca_mix_bwd(L.ptr(dhsd), L.ptr(hd), L.ptr(dh), B, hid, L.stream()))
    want = torch.where(h > 0, torch.cat([dhs, dhs], 1), torch.zeros(()))
    assert bits_equal(dh, want), "ca_mix_bwd: dh = dhs * [h > 0] (0 and -0 are not > 0)"
    # sigmoid: saturated inputs, zero, and ordinary values
    z = torch.cat([torch.tensor([100.0, -100.0, 88.0, -88.0, 0.0, -0.0, 20.0, -20.0]), torch.randn(100003, generator=g) * 6])
    zd = z.to(DEV, copy=True)
    L.check(lib.ieee_sigmoid_fwd(L.ptr(zd), z.numel(), L.stream()))
    att = torch.sigmoid(z.double())
    # 1 / (1 + exp(-z)): exp ~2 ulp, the add and the division 1 ulp each; results below FLT_MIN may flush to 0
    fmin = float(np.finfo(np.float32).tiny)
    within(zd, att, 6 * U * att + fmin, "sigmoid fwd")
    datt = torch.randn(z.numel(), generator=g)
    a32 = zd.clone()
    dz = torch.empty_like(zd)
    dattd = datt.to(DEV, copy=True)
    L.check(lib.ieee_sigmoid_bwd(L.ptr(dattd), L.ptr(a32), L.ptr(dz), z.numel(), L.stream()))
    a = a32.cpu().double()
    want = datt.double() * a * (1 - a)
    # datt * att * (1 - att) from the kernel's own att: 3 roundings (1 - att is exact for att >= 0.5, one rounding otherwise)
    within(dz, want, 4 * U * want.abs() + fmin, "sigmoid bwd")
    assert float(dz.cpu()[0]) == 0.0 and float(dz.cpu()[1]) == 0.0       # saturated: att * (1 - att) = 0 exactly


# ============================================================================ L2 normalisation
def test_l2norm_fwd_bwd_ragged_zero_and_tiny_rows():
    L, lib = _lib()
    g = torch.Generator().manual_seed(600)
    for rows in (1, 7, 192):
        for D in (1, 100, 768):
            x = torch.randn(rows, D, generator=g) * 2
            x[0 if rows == 1 else 1] = 0.0
            if rows > 1:
                x[2::5] = torch.randn(len(range(2, rows, 5)), D, generator=g) * (1e-14 / max(1.0, D ** 0.5))   # norm < 1e-12
            xr = x.double().requires_grad_(True)
            y_ref = F.normalize(xr, p=2, dim=1)
            dy = torch.randn(rows, D, generator=g)
            y_ref.backward(dy.double())
            xd = x.to(DEV, copy=True)
            y, nrm = torch.empty_like(xd), torch.empty(rows, device=DEV)
            L.check(lib.ieee_l2norm_fwd(L.ptr(xd), L.ptr(y), L.ptr(nrm), rows, D, L.stream()))
            what = "rows=%d D=%d" % (rows, D)
            # y = x / max(sqrt(sum x^2), eps): a D-term sum of squares ((D+4)u relative), sqrt and the division
            within(y, y_ref.detach(), (D + 8) * U * y_ref.detach().abs(), what + " y")
            nref = x.double().norm(dim=1).clamp_min(1e-12)
            within(nrm, nref, (D + 8) * U * nref, what + " norm")
            dyd = dy.to(DEV, copy=True)
            dx = sentinel_like((rows, D))
            L.check(lib.ieee_l2norm_bwd(L.ptr(dyd), L.ptr(y), L.ptr(nrm), L.ptr(dx), rows, D, 0, L.stream()))
            yy, nn_ = y_ref.detach(), nref[:, None]
            dot = (dy.double() * yy).sum(1, keepdim=True)
            clamped = (x.double().norm(dim=1) <= 1e-12)[:, None]
            # dx = (dy - y (y.dy)) / norm (y.dy: a D-term sum); clamped rows: dy / eps (autograd of clamp_min)
            tol = (4 * U * dy.double().abs() + yy.abs() * ((D + 4) * U * (dy.double() * yy).abs().sum(1, keepdim=True) +
                                                           2 * U * dot.abs() + (D + 8) * U * dot.abs())) / nn_
            tol = torch.where(clamped, 2 * U * dy.double().abs() / nn_, tol) + (D + 8) * U * xr.grad.abs()
            within(dx, xr.grad, 2 * tol, what + " dx")
            # accumulate: dx + (the same value) -- one exact doubling
            first = dx.clone()
            L.check(lib.ieee_l2norm_bwd(L.ptr(dyd), L.ptr(y), L.ptr(nrm), L.ptr(dx), rows, D, 1, L.stream()))
            assert bits_equal(dx, 2 * first), what + " accumulate"


# ============================================================================ optimizers
def _sgd_ref_and_bound(p, grads, lr, mom, wd, nesterov):
    """torch.optim.SGD in float64 and the fp32 forward-error bound of sgd_one over the steps:
    d = g + wd w (2 roundings of |g| + |wd w|), b = m buf + d (2 of |m buf| + |d|), d' = d + m b (2 of |d| + |m b|),
    w' = w - lr d' (2 of |w| + |lr d'|); the bound carries the previous step's w / buf errors through the same map."""
    w = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.SGD([w], lr=lr, momentum=mom, weight_decay=wd, dampening=0, nesterov=bool(nesterov))
    ew = torch.zeros_like(w.detach())
    eb = torch.zeros_like(ew)
    buf = torch.zeros_like(ew)
    for gr in grads:
        wv = w.detach().clone()
        d = gr.double() + wd * wv
        ed = wd * ew + 2 * U * (gr.double().abs() + wd * wv.abs())
        if mom:
            nb = mom * buf + d
            eb = mom * eb + ed + 2 * U * (mom * buf.abs() + d.abs())
            buf = nb
            if nesterov:
                ed = ed + mom * eb + 2 * U * (d.abs() + mom * nb.abs())
                d = d + mom * nb
            else:
                ed, d = eb.clone(), nb
        ew = ew + lr * ed + 2 * U * (wv.abs() + lr * d.abs())
        w.grad = gr.double().clone()
        opt.step()
    return w.detach(), (opt.state[w]["momentum_buffer"] if mom else None), 2 * ew, 2 * eb


def test_sgd_vector_and_scalar_paths_shadow_and_skip():
    """slices at float offsets 0..3 (offset 0: the 16-byte path; 1..3: the scalar path) of n > 2048*256*4 elements (the
    grid-stride loop turns on both paths); momentum 0 with a NULL buffer, nesterov 0 / 1, weight decay 0 / 5e-4"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(700)
    n = 2048 * 256 * 4 + 12347
    p0 = torch.randn(n + 8, generator=g)
    grads = [torch.randn(n + 8, generator=g) for _ in range(2)]
    gds = [t.to(DEV, copy=True) for t in grads]
    lr = 0.05
    cases = [(off, 0.9, nest, wd) for off in range(4) for nest in (0, 1) for wd in (0.0, 5e-4)]
    cases += [(off, 0.0, 0, wd) for off in (0, 1) for wd in (0.0, 5e-4)]
    for off, mom, nest, wd in cases:
        what = "off=%d mom=%g nesterov=%d wd=%g" % (off, mom, nest, wd)
        pd = p0.to(DEV, copy=True)
        buf = torch.zeros(n + 8, device=DEV) if mom else None
        shadow = torch.zeros(n + 8, dtype=torch.bfloat16, device=DEV)
        for gd in gds:
            L.check(lib.ieee_sgd_nesterov_step_ex(addr(pd, off), addr(gd, off), addr(buf, off) if mom else None, n, lr, mom, wd,
                                                  nest, shadow.data_ptr() + 2 * off, None, L.stream()))
        torch.cuda.synchronize()
        pc = pd.cpu()
        w_ref, b_ref, ew, eb = _sgd_ref_and_bound(p0[off:off + n], [t[off:off + n] for t in grads], lr, mom, wd, nest)
        within(pc[off:off + n], w_ref, ew, what + " params")
        if mom:
            within(buf[off:off + n], b_ref, eb, what + " momentum")
        # the shadow is the bf16 image of the updated parameters, element for element (round to nearest even)
        sc = shadow.cpu()
        assert bits_equal(sc[off:off + n], pc[off:off + n].to(torch.bfloat16)), what + " shadow"
        assert bits_equal(pc[:off], p0[:off]) and bits_equal(pc[off + n:], p0[off + n:]), what + ": wrote outside the slice"
        assert float(sc[:off].float().abs().sum()) == 0 and float(sc[off + n:].float().abs().sum()) == 0, what + ": shadow outside"
    # skip words: any set word leaves parameters, momentum and shadow bit-identical (both paths)
    for off in (0, 3):
        for words in ((1, 0), (0, 1), (1, 1)):
            pd, buf = p0.to(DEV, copy=True), torch.randn(n + 8, generator=g).to(DEV, copy=True)
            shadow = p0.to(torch.bfloat16).to(DEV, copy=True)
            snap = (pd.clone(), buf.clone(), shadow.clone())
            skip = torch.tensor(words, dtype=torch.int32, device=DEV)
            L.check(lib.ieee_sgd_nesterov_step_ex(addr(pd, off), addr(gds[0], off), addr(buf, off), n, lr, 0.9, 5e-4, 1,
                                                  shadow.data_ptr() + 2 * off, L.ptr(skip), L.stream()))
            torch.cuda.synchronize()
            assert bits_equal(pd, snap[0]) and bits_equal(buf, snap[1]) and bits_equal(shadow, snap[2]), \
                "skip %r off=%d: state changed" % (words, off)
        skip = torch.zeros(2, dtype=torch.int32, device=DEV)          # (0, 0): the update runs
        pd = p0.to(DEV, copy=True)
        L.check(lib.ieee_sgd_nesterov_step_ex(addr(pd, off), addr(gds[0], off), None, n, lr, 0.0, 0.0, 0, None, L.ptr(skip),
                                              L.stream()))
        assert not bits_equal(pd, p0.to(DEV, copy=True))


def test_adam_fifty_steps_with_weight_decay():
    """ieee_adam_step over 50 steps (bias correction far from its first-step values) against torch.optim.Adam in float64
    with the hyper-parameters rounded to fp32, as the kernel receives them.  Bound: the fp32 error of every quantity is
    carried through the update recursively (m, v, the denominator, the step), 4u per rounding step."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(710)
    n = 40961
    f32 = lambda v: float(np.float32(v))
    lr, b1, b2, eps, wd = f32(3e-3), f32(0.9), f32(0.999), f32(1e-8), f32(5e-4)
    p0 = torch.randn(n, generator=g)
    w = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([w], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    pd = p0.to(DEV, copy=True)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    em, ev, ew = (torch.zeros(n, dtype=torch.float64) for _ in range(3))
    for t in range(1, 51):
        gr = torch.randn(n, generator=g) * (0.1 + (t % 7))
        wv = w.detach().clone()
        d = gr.double() + wd * wv
        ed = wd * ew + 2 * U * d.abs()
        w.grad = gr.double().clone()
        opt.step()
        st = opt.state[w]
        mm, vv = st["exp_avg"], st["exp_avg_sq"]
        bc1, bc2s = 1 - b1 ** t, (1 - b2 ** t) ** 0.5
        em = b1 * em + (1 - b1) * ed + 4 * U * (mm.abs() + d.abs())
        ev = b2 * ev + (1 - b2) * 2 * d.abs() * ed + 4 * U * (vv + (1 - b2) * d * d)
        denom = vv.sqrt() / bc2s + eps
        edn = ev / (2 * vv.sqrt().clamp_min(1e-30)) / bc2s + 4 * U * denom
        upd = lr / bc1 * mm / denom
        ew = ew + lr / bc1 * (em / denom + mm.abs() * edn / denom ** 2) + 4 * U * (upd.abs() + wv.abs())
        grd = gr.to(DEV, copy=True)
        L.check(lib.ieee_adam_step(L.ptr(pd), L.ptr(grd), L.ptr(m), L.ptr(v), None, n, lr, b1, b2, eps, wd, t, L.stream()))
    within(pd, w.detach(), 2 * ew, "adam params after 50 steps")
    within(m, st["exp_avg"], 2 * em, "adam exp_avg")
    within(v, st["exp_avg_sq"], 2 * ev, "adam exp_avg_sq")


def test_guard_buffers_restore_and_backup_bitwise():
    L, lib = _lib()
    g = torch.Generator().manual_seed(720)
    n = 2048 * 256 + 4097               # the grid-stride loop turns
    a = torch.randn(n, generator=g)
    b = torch.randn(n, generator=g)
    a[:6] = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 1e-40, float("nan")])
    for flag in (1, 0, 7):
        bufs, backup = a.to(DEV, copy=True), b.to(DEV, copy=True)
        flags = torch.tensor([flag, 0], dtype=torch.int32, device=DEV)
        L.check(lib.ieee_guard_buffers(L.ptr(flags), L.ptr(bufs), L.ptr(backup), n, L.stream()))
        torch.cuda.synchronize()
        if flag:       # restore: buffers <- backup, backup untouched
            assert bits_equal(bufs, b) and bits_equal(backup, b), "guard restore flag=%d" % flag
        else:          # keep: backup <- buffers, buffers untouched
            assert bits_equal(bufs, a) and bits_equal(backup, a), "guard backup"
