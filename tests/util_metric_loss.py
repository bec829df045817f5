"""float64 restatements of the three metric criteria of ieee_amd.losses -- the batch-hard triplet loss
(hard_mine_triplet_loss.py:23-48), the hetero-center loss (hcloss.py:18-39) and the 3M loss with either distance
(multi_modal_margin_loss_new.py:19-40) -- as the kernels of csrc/metric_loss.hip are meant to compute them: loss AND every
gradient element.  tests/test_metric_loss_cpu.py pins them against the reference's classes and against torch autograd, and
shows that the `variant`s (deliberately wrong restatements) leave the bounds the GPU tests use.

The triplet gradient is written out (numpy, no autograd): exactly equal maxima / minima share their anchor's gradient
evenly, a pair with d^2 < 1e-12 gets none, an anchor whose hinge is <= 0 contributes none.  d^2 is formed from differences
(exactly 0 for equal rows), which is what the kernel does; the reference's Gram expansion agrees with it to rounding."""
import numpy as np
import torch

CLAMP = 1e-12


def sq_dists(x):
    """[B][B] sum_k (x_i - x_j)^2, row by row (no B*B*D temporary)"""
    x = np.asarray(x, np.float64)
    return np.stack([((x[i] - x) ** 2).sum(1) for i in range(x.shape[0])])


def triplet_ref(x, pids, margin, variant=None):
    """x [B][E] (any float dtype; computed in float64), pids [B].  -> dict(loss, grad [B][E], ap, an, hinge, active,
    gap_p, gap_n, ties): gap_* = relative distance of every anchor's best candidate to the best one that is not exactly
    equal to it (inf when there is none), ties = the largest number of exactly equal best candidates.
    variant: None | 'one_tie' (the whole gradient to the first of equal entries) | 'clamp_grad' (clamped pairs get the
    gradient of sqrt at the clamp value)"""
    x = np.asarray(x, np.float64)
    pids = np.asarray(pids)
    B = x.shape[0]
    d2 = sq_dists(x)
    d = np.sqrt(np.maximum(d2, CLAMP))
    same = pids[:, None] == pids[None, :]
    W = np.zeros((B, B))
    ap, an, gap_p, gap_n = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)
    ties = 1
    for i in range(B):
        pos, neg = d[i][same[i]], d[i][~same[i]]
        ap[i], an[i] = pos.max(), neg.min()
        rest_p, rest_n = pos[pos != ap[i]], neg[neg != an[i]]
        gap_p[i] = (ap[i] - rest_p.max()) / ap[i] if rest_p.size else np.inf
        gap_n[i] = (rest_n.min() - an[i]) / an[i] if rest_n.size else np.inf
        tp = np.flatnonzero(same[i] & (d[i] == ap[i]))
        tn = np.flatnonzero(~same[i] & (d[i] == an[i]))
        ties = max(ties, tp.size, tn.size)
        if margin + ap[i] - an[i] > 0:
            if variant == "one_tie":
                tp, tn = tp[:1], tn[:1]
            W[i, tp] += 1.0 / (B * tp.size)
            W[i, tn] -= 1.0 / (B * tn.size)
    hinge = np.maximum(margin + ap - an, 0.0)
    keep = np.ones_like(d2, bool) if variant == "clamp_grad" else d2 >= CLAMP
    Wd = np.where(keep, W / d, 0.0)
    Ws = Wd + Wd.T                      # i as anchor of j, and j as anchor of i: d d_ij / d x_i = (x_i - x_j) / d_ij
    grad = Ws.sum(1)[:, None] * x - Ws @ x
    absw = np.abs(Wd) + np.abs(Wd).T
    return dict(loss=hinge.mean(), grad=grad, ap=ap, an=an, hinge=margin + ap - an, active=int((hinge > 0).sum()),
                gap_p=gap_p, gap_n=gap_n, ties=ties, absw=absw)


U = 2.0 ** -24           # unit roundoff of fp32
STABLE = 2.0 ** -10      # selection stability: best and second-best candidate differ by at least this, relative


def triplet_bounds(ref, x, D, parts, margin, gscale=1.0):
    """fp32 error model of ieee_triplet_hard_fwd_bwd against triplet_ref `ref` of the SAME fp32 inputs x [B][parts*D]
    (exact in float64), valid when the selection is stable (asserted by the tests: gaps >= STABLE >> e_d, |hinge| >> e_d):
      d2   a lane sums L = ceil(D/64) * parts non-negative terms (x_i - x_j)^2, each with one rounding in the difference (2u
           on the square) and one in the FMA, then 6 butterfly adds: relative error e2 = (L + 8) u;
      d    sqrt is correctly rounded: e_d = e2 / 2 + u (relative; the same for d_ap, d_an, the selection being stable);
      loss hinge_i off by e_d (ap + an) + 2u (|m| + ap + an); the mean is ceil(B/256) strided adds, an 8-level tree and a
           division over non-negative terms -> (e_d + (ceil(B/256) + 12) u) (|m| + mean(ap + an));
      dx   row i sums n_i terms w_ij (x_i - x_j), n_i = the pairs with a weight (<= 4 + ties for random data):
           w = (1/(B np) +- 1/(B nn)) / d carries 4 roundings and e_d, the difference 1, the FMA chain n_i, gscale 1:
           |err_ik| <= (e_d + (n_i + 8) u) gscale sum_j |w_ij| |x_ik - x_jk|   (<= the triangle bound used here).
    -> loss_tol, grad_tol [B][E], mean_tol (for out[1], out[2])"""
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    L = -(-D // 64) * parts
    e_d = (L + 8) * U / 2 + U
    assert e_d < STABLE / 8
    span = abs(margin) + float((ref["ap"] + ref["an"]).mean())
    loss_tol = (e_d + (-(-B // 256) + 12) * U) * span
    A = ref["absw"]
    n_i = (A != 0).sum(1)
    ax = np.abs(x)
    grad_tol = (e_d + (n_i[:, None] + 8) * U) * gscale * (A.sum(1)[:, None] * ax + A @ ax)
    return loss_tol, grad_tol, (e_d + (-(-B // 256) + 12) * U) * float(max(ref["ap"].mean(), ref["an"].mean()))


def assert_stable(ref, tie_case=False):
    """the condition under which fp32 and float64 mine the same pairs and hinge the same anchors"""
    assert float(ref["gap_p"].min()) >= STABLE and float(ref["gap_n"].min()) >= STABLE, (ref["gap_p"].min(), ref["gap_n"].min())
    assert float(np.abs(ref["hinge"]).min()) >= STABLE * float((ref["ap"] + ref["an"]).max()), np.abs(ref["hinge"]).min()
    assert tie_case == (ref["ties"] > 1), ref["ties"]


def center_bounds(feats, pids, dist_type, mode, margin=0.0, gscale=1.0):
    """fp32 error model of center_pairs_kernel per chunk of `rows` rows (the l2 part is tests/test_head_kernels_gpu.py's
    model of margin3m_kernel), with a = mean_r |f|:
      centre  rows-term sum / rows: abs err (rows + 2) u a;
      l2      S = sum_k (c_a - c_b)^2, a thread's ceil(D/256)-chain and an 8-level tree: err 2 (D + 2 rows + 8) u sum_k (a_a + a_b)^2;
              gradient 2 gs (c_a - c_b) / rows: err 4 (rows + 4) u (a_a + a_b) gs / rows + 4u |g|;
      l1      S = sum_k |c_a - c_b| / D: err (rows + ceil(D/256) + 13) u mean_k (a_a + a_b); gradient +- gs / (D rows), exact up
              to 4u once the SIGN of every difference is decided: |c_a - c_b|_k > 2 (rows + 3) u (a_a + a_b)_k or exactly 0;
      cos     dot, |c1|^2, |c2|^2 with E = 2 (rows + 2) + ceil(D/256) + 9 roundings each: cos off by
              tc = (E + 6) u (P / (n1 n2) + |cos| (Q1 / n1^2 + Q2 / n2^2)), P = sum a_1 a_2, Q = sum a^2; gradient
              gs / rows ((E + 10) u (a_2 / (n1 n2) + |cos| a_1 / n1^2) + tc a_1 / n1^2) and 1 <-> 2.
    3M: the loss term is |m - S_sel|; the selected pair and the sign of m - S are compared only where they are decided
    outside 4x the distance bound (`decided`; the tests assert that this is every chunk, except where they build a tie).
    -> loss_tol, [grad_tol per modality], decided (list of bool per chunk), signs_ok (l1)"""
    fd = [np.asarray(f, np.float64) for f in feats]
    M = len(fd)
    B, D = fd[0].shape
    n = len(np.unique(np.asarray(pids)))
    per = -(-B // n)
    pairs = ((0, 1),) if M == 2 else ((0, 1), (1, 2), (0, 2))
    chain = -(-D // 256)
    loss_tol, grad_tol, decided, signs_ok, total = 0.0, [np.zeros((B, D)) for _ in range(M)], [], True, 0.0
    for r0 in list(range(0, B, per))[:n]:
        rows = min(B, r0 + per) - r0
        c = [f[r0:r0 + rows].mean(0) for f in fd]
        a = [np.abs(f[r0:r0 + rows]).mean(0) for f in fd]
        dts, dvs = [], []
        for p, q in pairs:
            if dist_type == "l2":
                dts.append(float(((a[p] + a[q]) ** 2).sum()) * 2 * (D + 2 * rows + 8) * U)
                dvs.append(float(((c[p] - c[q]) ** 2).sum()))
                g = 4 * (rows + 4) * U * (a[p] + a[q]) / rows * gscale
            elif dist_type == "l1":
                dts.append(float((a[p] + a[q]).mean()) * (rows + chain + 13) * U)
                dvs.append(float(np.abs(c[p] - c[q]).mean()))
                diff = np.abs(c[p] - c[q])
                signs_ok = signs_ok and bool(((diff > 2 * (rows + 3) * U * (a[p] + a[q])) | (diff == 0)).all())
                g = np.full(D, 4 * U * gscale / (D * rows))
            else:
                E = 2 * (rows + 2) + chain + 9
                n1, n2 = np.sqrt((c[p] ** 2).sum()), np.sqrt((c[q] ** 2).sum())
                cs = float((c[p] * c[q]).sum() / (n1 * n2))
                tc = (E + 6) * U * (float((a[p] * a[q]).sum()) / (n1 * n2)
                                    + abs(cs) * (float((a[p] ** 2).sum()) / n1 ** 2 + float((a[q] ** 2).sum()) / n2 ** 2))
                dts.append(tc)
                dvs.append(1 - cs)
                g = None
                for me, other, nme in ((p, q, n1), (q, p, n2)):
                    gt = gscale / rows * ((E + 10) * U * (a[other] / (n1 * n2) + abs(cs) * a[me] / nme ** 2) + tc * a[me] / nme ** 2)
                    grad_tol[me][r0:r0 + rows] = np.maximum(grad_tol[me][r0:r0 + rows], gt)
            if g is not None:
                for m in (p, q):
                    grad_tol[m][r0:r0 + rows] = np.maximum(grad_tol[m][r0:r0 + rows], g)
        t_ = max(dts)
        if mode == "margin3m":
            s = sorted(abs(margin - d) for d in dvs)
            loss_tol += t_ + 4 * U * s[2]
            total += s[2]
            decided.append(s[2] - s[1] > 4 * t_ and s[2] > 4 * t_)
        else:
            loss_tol += t_ + 4 * U * abs(dvs[0])
            total += abs(dvs[0])
            # (max(0, 1 - cos) needs no decision: its gradient goes to 0 continuously where 1 - cos does)
            decided.append(dist_type == "cos" or abs(dvs[0]) > 4 * t_)
    return 2 * loss_tol + n * U * total, grad_tol, decided, signs_ok          # (+ the chunk-order sum of the terms)


def triplet_autograd(x, pids, margin):
    """the same criterion through torch autograd in float64 (difference form, Tensor.max() / .min() per anchor as the
    reference writes them): loss, grad"""
    x = torch.as_tensor(np.asarray(x, np.float64)).clone().requires_grad_(True)
    pids = torch.as_tensor(np.asarray(pids))
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(2).clamp(min=CLAMP).sqrt()
    mask = pids[:, None] == pids[None, :]
    ap = torch.stack([d[i][mask[i]].max() for i in range(len(pids))])
    an = torch.stack([d[i][~mask[i]].min() for i in range(len(pids))])
    loss = torch.nn.functional.margin_ranking_loss(an, ap, torch.ones_like(an), margin=margin)
    loss.backward()
    return loss.item(), x.grad.numpy()


def center_ref(feats, pids, dist_type, mode, margin=0.0, variant=None):
    """feats: M arrays [B][D]; mode 'hetero' (M = 2) | 'margin3m' (M = 3); dist_type 'l2' | 'l1' | 'cos'.
    -> loss (float), grads (M arrays), label_num, chunks.  The formulas are restated with torch float64 ops and
    differentiated by autograd (|.| has sign(0) = 0 there); which argument of the 3M max is kept is decided here.
    variant: None | 'max_last' (the LAST of equal maxima) | 'l1_sum' (L1 as a sum, not nn.L1Loss's mean)"""
    fs = [torch.as_tensor(np.asarray(f, np.float64)).clone().requires_grad_(True) for f in feats]
    pids = torch.as_tensor(np.asarray(pids))
    n = int(torch.unique(pids).numel())
    chunks = [f.chunk(n, 0) for f in fs]
    if len(chunks[0]) < n:
        raise IndexError("tuple index out of range")

    def dist(a, b):
        if dist_type == "l2":
            return ((a - b) ** 2).sum()
        if dist_type == "l1":
            return (a - b).abs().sum() if variant == "l1_sum" else (a - b).abs().mean()
        na, nb = a.norm().clamp(min=1e-8), b.norm().clamp(min=1e-8)        # nn.CosineSimilarity(dim=0, eps=1e-8)
        return (a * b).sum() / (na * nb)

    total = torch.zeros((), dtype=torch.float64)
    for i in range(n):
        c = [ch[i].mean(0) for ch in chunks]
        if mode == "hetero":
            v = 1 - dist(c[0], c[1]) if dist_type == "cos" else dist(c[0], c[1]).abs()
            if v.item() > 0:                       # python's max(0, v): the int 0 unless v > 0
                total = total + v
        else:
            if dist_type == "cos":
                raise NotImplementedError("the reference's 3M loss never assigns `dist` for 'cos'")
            args = [(margin - dist(c[0], c[1])).abs(), (margin - dist(c[1], c[2])).abs(), (margin - dist(c[0], c[2])).abs()]
            vals = [a.item() for a in args]
            best = max(vals)
            order = [k for k in range(3) if vals[k] == best]
            total = total + args[order[-1] if variant == "max_last" else order[0]]
    if total.requires_grad:
        total.backward()
    grads = [f.grad.numpy() if f.grad is not None else np.zeros(tuple(f.shape)) for f in fs]
    return float(total.item()), grads, n, len(chunks[0])


def seeded(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


def unit_rows(x):
    """rows scaled to unit L2 norm (float32 in, float32 out): what the model's 'margin' mode returns per modality"""
    x = np.asarray(x, np.float64)
    return (x / np.sqrt((x * x).sum(-1, keepdims=True))).astype(np.float32)
