"""GPU: the kernels of csrc/metric_loss.hip -- ieee_triplet_hard_fwd_bwd and ieee_center_pairs_fwd_bwd -- and what is built on
them (losses.TripletLoss, hetero_loss, multiModalMarginLossNew(dist_type='l1'), Image3MEngine(weight_t=...)) against the
float64 restatements of tests/util_metric_loss.py (pinned to the reference's classes by tests/test_metric_loss_cpu.py):
the loss and EVERY gradient element, and against the reference's fp32 CPU results in tests/golden/metric_loss_golden.npz.

Bounds are not tuned.  They are the fp32 error models written out in util_metric_loss.triplet_bounds / center_bounds:
with u = 2^-24, the D*parts-term sum of squared differences is a per-lane FMA chain of ceil(D/64)*parts terms plus a 6-step
butterfly (relative, the terms being non-negative), the square root is correctly rounded and halves that, and a gradient
row is a sum of n_i <= 4 + ties weighted differences.  They hold only if fp32 and float64 select the same pairs, which is a
CONDITION on the data, asserted on the float64 side for every anchor (util_metric_loss.assert_stable): best and second
best candidate at least 2^-10 apart relative, every hinge at least that far from 0; in the tie cases the second best is
the best candidate that is not exactly equal.  Seeds are chosen so that it holds; no anchor is skipped.  Where the
kernel's arithmetic is exact (inactive hinges, accumulate = old + new, two calls) the assert is bit equality."""
import os

import numpy as np
import pytest
import torch

from tests import util_metric_loss as um

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = um.U
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metric_loss_golden.npz")


def _lib():
    from ieee_amd import _lib as L
    return L, L.require_gpu()


def sentinel_like(shape):
    """a fill no kernel writes: a NaN with a payload"""
    return torch.full(shape, -1, dtype=torch.int32, device=DEV).view(torch.float32)


def within(got, ref, tol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = np.broadcast_to(np.asarray(tol, np.float64), ref.shape)
    assert np.isfinite(got).all(), "%s: non-finite output" % what
    err = np.abs(got - ref)
    if (err > tol).any():
        i = int(np.argmax((err - tol).ravel()))
        raise AssertionError("%s: %d elements out of bound; worst at %d: got %r want %r |err| %.3e > tol %.3e" % (
            what, int((err > tol).sum()), i, got.ravel()[i], ref.ravel()[i], err.ravel()[i], tol.ravel()[i]))


# ============================================================================ batch-hard triplet
def triplet_data(B, D, parts, ids, seed, unit=False):
    """x [B][parts*D] fp32, pids [B].  Rows live near a 4-dimensional latent (identity centre + noise) embedded in
    parts*D dimensions, so that the distances of an anchor to its candidates are spread out like in a trained embedding
    (in a random high-dimensional cloud they concentrate and no seed separates best from second best by 2^-10);
    scaled so that the median pair distance is 1, or every part of every row to unit norm (`unit`: the engine's features)."""
    rs = np.random.RandomState(seed)
    E = parts * D
    pids = np.asarray(ids)
    q = min(E, 4)
    cent = {p: rs.standard_normal(q) for p in np.unique(pids)}
    z = np.stack([cent[p] for p in pids]) + 0.45 * rs.standard_normal((B, q))
    P = rs.standard_normal((q, E)) / np.sqrt(q)
    x = z @ P + (0.02 * rs.standard_normal((B, E)) if E > q else 0.0)
    if unit:
        x = x.reshape(B, parts, D) + 0.3 * rs.standard_normal((1, parts, D))
        x = (x / np.sqrt((x * x).sum(2, keepdims=True))).reshape(B, E)
    else:
        d = np.sqrt(um.sq_dists(x))
        x = x / np.median(d[np.triu_indices(B, 1)])
    return x.astype(np.float32), pids


def run_triplet(x, pids, parts, margin, gscale=1.0, prev=None, want_dx=True):
    """x [B][parts*D] -> the kernel's layout [parts][B][D]; returns out[4], dx as [B][parts*D]"""
    L, lib = _lib()
    B, E = x.shape
    D = E // parts
    xd = torch.from_numpy(np.ascontiguousarray(x.reshape(B, parts, D).transpose(1, 0, 2))).to(DEV)
    pd = torch.from_numpy(np.asarray(pids, np.int64)).to(DEV)
    if prev is None:
        dx = sentinel_like((parts, B, D))
    else:
        dx = torch.from_numpy(np.ascontiguousarray(prev.reshape(B, parts, D).transpose(1, 0, 2))).to(DEV)
    out = sentinel_like((4,))
    work = torch.empty(B * B + 5 * B, device=DEV)
    L.check(lib.ieee_triplet_hard_fwd_bwd(L.ptr(xd), parts, L.ptr(pd), L.ptr(dx) if want_dx else None, L.ptr(out), L.ptr(work),
                                          B, D, margin, gscale, 0 if prev is None else 1, L.stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), dx.cpu().numpy().transpose(1, 0, 2).reshape(B, E)


def check_triplet(x, pids, parts, margin, what, gscale=1.0, tie_case=False):
    B, E = x.shape
    ref = um.triplet_ref(x, pids, margin)
    um.assert_stable(ref, tie_case)
    loss_tol, grad_tol, mean_tol = um.triplet_bounds(ref, x, E // parts, parts, margin, gscale)
    out, dx = run_triplet(x, pids, parts, margin, gscale)
    print("%s: loss %.9g ref %.9g tol %.3g | max grad err %.3g, max tol %.3g | active %d/%d" % (
        what, out[0], ref["loss"], loss_tol, np.abs(dx - gscale * ref["grad"]).max(), grad_tol.max(), ref["active"], B))
    within(out[0:1], [ref["loss"]], loss_tol, what + " loss")
    within(out[1:3], [ref["ap"].mean(), ref["an"].mean()], mean_tol, what + " mean d_ap, d_an")
    assert out[3] == ref["active"], what
    within(dx, gscale * ref["grad"], grad_tol, what + " dx")
    return ref, out, dx


# (B, D, parts, identities, seed, margin): the smallest shapes that take each path -- two singletons; K = 2; the engine's
# shape; B not a multiple of a wave (65) or of a workgroup (257); D = 1, 3 (below a wave), 2304 / 2305 (a lane chain of 36 / 37,
# the last one ragged); identities in shuffled order
TRIPLET_CASES = {
    "two_singletons": (2, 5, 1, [4, 2], 1, 2.0),
    "B8_K2": (8, 16, 1, list(np.arange(8) // 2), 2, 0.3),
    "engine_shape": (64, 768, 3, list(np.arange(64) // 4), 3, 0.3),
    "B65": (65, 16, 1, list(np.arange(65) % 13), 14, 0.3),
    "B257": (257, 24, 1, list((np.arange(257) * 7) % 33), 25, 0.3),
    "D1": (8, 1, 1, list(np.arange(8) // 2), 6, 0.3),
    "D3": (12, 3, 1, list(np.arange(12) % 4), 7, 0.3),
    "D2304": (8, 2304, 1, list(np.arange(8) // 2), 18, 0.3),
    "D2305_parts2": (9, 2305, 2, [5, 1, 5, 3, 1, 3, 5, 1, 3], 9, 0.3),
    "shuffled": (32, 40, 1, list(np.random.RandomState(0).permutation(np.arange(32) // 4 * 1000003 + 17)), 10, 0.3),
}


def _case(name):
    B, D, parts, ids, seed, margin = TRIPLET_CASES[name]
    x, pids = triplet_data(B, D, parts, ids, seed, unit=(name == "engine_shape"))
    return x, pids, parts, margin


@pytest.mark.parametrize("name", sorted(TRIPLET_CASES))
def test_triplet_kernel_matches_the_float64_restatement(name):
    x, pids, parts, margin = _case(name)
    ref, out, dx = check_triplet(x, pids, parts, margin, name)
    if name == "two_singletons":      # each row's hardest positive is itself (clamped): the gradient is the negative's alone
        assert ref["active"] == 2 and np.abs(dx).min() > 0


def test_triplet_margins_inactive_anchors_scale_accumulate_and_repeat():
    x, pids, parts, _ = _case("B65")
    ref, _, _ = check_triplet(x, pids, parts, -0.35, "some inactive", gscale=0.37)
    assert 0 < ref["active"] < 65
    # every hinge inactive: the loss is 0 and dx is written with exact zeros
    out, dx = run_triplet(x, pids, parts, -100.0)
    assert out[0] == 0.0 and out[3] == 0.0 and not dx.any() and not np.isnan(dx).any()
    # every hinge active
    ref, out, dx = check_triplet(x, pids, parts, 10.0, "all active")
    assert ref["active"] == 65
    # accumulate = 1 adds to what is there: one more rounding of old + new
    prev = um.seeded(x.shape, 77, 0.01)
    _, acc = run_triplet(x, pids, parts, 10.0, prev=prev)
    assert np.array_equal(acc, prev + dx)
    # the same bits on a second call, and without dx only the four numbers
    out2, dx2 = run_triplet(x, pids, parts, 10.0)
    assert np.array_equal(out2.view(np.int32), out.view(np.int32)) and np.array_equal(dx2.view(np.int32), dx.view(np.int32))
    out3, untouched = run_triplet(x, pids, parts, 10.0, want_dx=False)
    assert np.array_equal(out3.view(np.int32), out.view(np.int32)) and np.isnan(untouched).all()


def test_triplet_duplicate_rows_share_the_gradient_and_clamped_pairs_get_none():
    """rows 1 := row 0 (identity 0 has three rows): every anchor that mines row 0 mines row 1 too, exactly tied, and the
    two get identical gradients (the reference's Tensor.max() / .min() split evenly).  In the second set row 1 is row 0
    plus one ulp in one element: 0 < d^2 < 1e-12 is clamped, so the pair (0, 1) -- each the other's hardest positive, tied
    with itself at 1e-6 -- contributes nothing, where the gradient of sqrt at the clamp would be ~1e5 times the ulp."""
    x, pids = triplet_data(12, 20, 1, [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3], 11)
    x[1] = x[0]
    ref, out, dx = check_triplet(x, pids, 1, 10.0, "duplicates", tie_case=True)
    assert np.array_equal(dx[0], dx[1]) and np.abs(dx[0]).max() > 0
    wrong = um.triplet_ref(x, pids, 10.0, "one_tie")["grad"]
    assert (np.abs(wrong - ref["grad"]) > um.triplet_bounds(ref, x, 20, 1, 10.0)[1]).any()
    x, pids = triplet_data(8, 20, 1, [0, 0, 1, 1, 2, 2, 3, 3], 12)
    x[0] += 1.0                          # away from the others: nobody mines row 0 or 1 as a negative (a near-tie otherwise)
    x[1] = x[0]
    x[1, 3] = x[0, 3] + np.spacing(x[0, 3])
    ref, out, dx = check_triplet(x, pids, 1, 10.0, "near duplicate", tie_case=True)
    wrong = um.triplet_ref(x, pids, 10.0, "clamp_grad")["grad"]
    assert (np.abs(wrong - ref["grad"]) > um.triplet_bounds(ref, x, 20, 1, 10.0)[1]).any()


def test_triplet_loss_module_backward_and_single_identity():
    from ieee_amd.losses import TripletLoss
    x, pids, _, margin = _case("B8_K2")
    ref = um.triplet_ref(x, pids, margin)
    loss_tol, grad_tol, _ = um.triplet_bounds(ref, x, x.shape[1], 1, margin, 2.5)
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    loss = TripletLoss(margin=margin)(xt, torch.from_numpy(pids).to(DEV))
    assert loss.dim() == 0
    (2.5 * loss).backward()
    within([loss.item()], [ref["loss"]], loss_tol, "TripletLoss")
    within(xt.grad.cpu().numpy(), 2.5 * ref["grad"], grad_tol + 2 * U * np.abs(2.5 * ref["grad"]), "TripletLoss backward")
    with pytest.raises(RuntimeError, match="same identity"):
        TripletLoss()(xt, torch.zeros(8, dtype=torch.long, device=DEV))


# ============================================================================ centre losses
DIST = {"l2": 0, "l1": 1, "cos": 2}
MODE = {"hetero": 0, "margin3m": 1}


def centre_data(B, D, pids, seed, M=3):
    """per chunk the modality centres sit 0, 1 and 3 half-units along a random +-1 direction (permuted per chunk) plus small
    noise, as tests/test_head_kernels_gpu.py builds them: the three distances are far apart against the fp32 bound.
    M = 2 (hetero): two clouds around their own random centre, so that the cosine is not +-1."""
    rs = np.random.RandomState(seed)
    if M == 2:
        return [(rs.standard_normal((B, D)) * 0.3 + rs.standard_normal(D)).astype(np.float32) for _ in range(2)]
    n = len(np.unique(pids))
    per = -(-B // n)
    v = (rs.randint(0, 2, D) * 2 - 1) / np.sqrt(D)
    f = [np.empty((B, D), np.float32) for _ in range(3)]
    for r0 in range(0, B, per):
        rows = min(B, r0 + per) - r0
        perm = rs.permutation(3)
        for m in range(3):
            f[m][r0:r0 + rows] = 0.5 * (0.0, 1.0, 3.0)[perm[m]] * v + rs.standard_normal((rows, D)) * 0.02 / np.sqrt(D)
    return f


def run_centre(f, pids, dist, mode, margin, gscale=1.0, prev=None):
    L, lib = _lib()
    M = len(f)
    B, D = f[0].shape
    feats = torch.from_numpy(np.stack(f)).to(DEV)
    pd = torch.from_numpy(np.asarray(pids, np.int64)).to(DEV)
    df = sentinel_like((M, B, D)) if prev is None else torch.from_numpy(prev).to(DEV)
    out3 = sentinel_like((3,))
    work = torch.empty(B + 3, device=DEV)
    L.check(lib.ieee_center_pairs_fwd_bwd(L.ptr(feats), M, L.ptr(pd), L.ptr(df), L.ptr(out3), L.ptr(work), B, D, DIST[dist],
                                          MODE[mode], margin, gscale, 0 if prev is None else 1, L.stream()))
    torch.cuda.synchronize()
    return out3.cpu().numpy(), df.cpu().numpy()


def check_centre(f, pids, dist, mode, margin, what, gscale=1.0, tie=False):
    loss, grads, n, nch = um.center_ref(f, pids, dist, mode, margin)
    loss_tol, grad_tol, decided, signs_ok = um.center_bounds(f, pids, dist, mode, margin, gscale)
    assert signs_ok, what + ": a centre difference too close to 0 for its sign"
    assert tie or all(decided), what + ": near-ties in the data"
    out3, df = run_centre(f, pids, dist, mode, margin, gscale)
    print("%s: loss %.9g ref %.9g tol %.3g" % (what, out3[0], loss, loss_tol))
    assert out3[1] == n and out3[2] == nch, what
    within(out3[0:1], [loss], loss_tol, what + " loss")
    for m in range(len(f)):
        g = gscale * grads[m]
        within(df[m], g, grad_tol[m] + 4 * U * np.abs(g), what + " dfeats[%d]" % m)
    return out3, df, grads


CENTRE_LAYOUTS = {"chunks_of_1": (6, list(range(6))), "chunks_of_4": (16, list(np.arange(16) // 4)),
                  "uneven": (10, [0, 0, 0, 1, 1, 1, 2, 2, 2, 3]), "two_blocks_of_k": (8, [9, 9, 9, 9, 2, 2, 2, 2])}


@pytest.mark.parametrize("mode,dist", [("hetero", "l2"), ("hetero", "l1"), ("hetero", "cos"), ("margin3m", "l2"), ("margin3m", "l1")])
@pytest.mark.parametrize("D", [1, 255, 768])
def test_centre_kernel_matches_the_float64_restatement(mode, dist, D):
    M = 2 if mode == "hetero" else 3
    for k, (name, (B, pids)) in enumerate(sorted(CENTRE_LAYOUTS.items())):
        f = centre_data(B, D, pids, 100 + 10 * D + k, M)
        for margin, gs in ((1.0, 1.0), (3.0, 0.37)):
            check_centre(f, pids, dist, mode, margin, "%s/%s D=%d %s m=%g" % (mode, dist, D, name, margin), gs)


def test_centre_margin3m_l2_has_the_bits_of_the_3m_kernel():
    L, lib = _lib()
    for B, D, pids in ((64, 768, np.arange(64) // 4), (10, 255, np.array([0, 0, 0, 1, 1, 1, 2, 2, 2, 3])), (6, 1, np.arange(6)),
                       (10, 100, np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 5]))):           # the last: chunks short of identities
        f = centre_data(B, D, pids, 300 + B)
        for margin, gs in ((1.0, 1.0), (3.0, 0.37)):
            out_new, df_new = run_centre(f, pids, "l2", "margin3m", margin, gs)
            feats = torch.from_numpy(np.stack(f)).to(DEV)
            pd = torch.from_numpy(np.asarray(pids, np.int64)).to(DEV)
            df, out3, work = sentinel_like((3, B, D)), sentinel_like((3,)), torch.empty(B + 3, device=DEV)
            L.check(lib.ieee_margin3m_fwd_bwd(L.ptr(feats), L.ptr(pd), L.ptr(df), L.ptr(out3), L.ptr(work), B, D, margin, gs,
                                              L.stream()))
            torch.cuda.synchronize()
            assert np.array_equal(out_new.view(np.int32), out3.cpu().numpy().view(np.int32)), (B, D, margin)
            assert np.array_equal(df_new.view(np.int32), df.cpu().numpy().view(np.int32)), (B, D, margin)


@pytest.mark.parametrize("dist", ["l2", "l1"])
def test_centre_3m_equal_maxima_keep_the_first_argument(dist):
    """modalities built as copies of each other make two of the three arguments of the max exactly equal (the same bits
    through the same operations) and the third |m - 0| = m smaller: f3 := f2 ties arguments 1 and 3, f3 := f1 ties 1 and
    2, f2 := f1 ties 2 and 3.  The first of the equal ones is kept; the modality outside that pair gets exact zeros."""
    rs = np.random.RandomState(400)
    for B, D in ((8, 768), (10, 100)):
        pids = np.arange(B) // 2
        a = (rs.standard_normal((B, D)) * 0.3).astype(np.float32)
        b = (rs.standard_normal((B, D)) * 0.3 + 1.0).astype(np.float32)
        for f, zero in (([a, b, b.copy()], 2), ([a, b, a.copy()], 2), ([a, a.copy(), b], 0)):
            out3, df, grads = check_centre(f, pids, dist, "margin3m", 0.1, "equal maxima %s zero=%d" % (dist, zero), 0.5, tie=True)
            assert not df[zero].any() and not grads[zero].any()
            others = [m for m in range(3) if m != zero]
            assert np.abs(df[others[0]]).min() > 0 and np.array_equal(df[others[0]], -df[others[1]])


def test_centre_l1_zero_difference_accumulate_and_modules():
    from ieee_amd.losses import hetero_loss, multiModalMarginLossNew
    B, D, pids = 8, 40, np.arange(8) // 2
    f = centre_data(B, D, pids, 500)
    f[1][:, 7] = f[0][:, 7]          # the two centres agree exactly in column 7: sign(0) = 0
    for mode, M in (("hetero", 2), ("margin3m", 3)):
        out3, df, grads = check_centre(f[:M], pids, "l1", mode, 1.0, "zero difference " + mode)
        if mode == "hetero":
            assert not df[0][:, 7].any() and not df[1][:, 7].any() and np.abs(np.delete(df[0], 7, 1)).min() > 0
        prev = um.seeded((M, B, D), 501, 0.01)
        _, acc = run_centre(f[:M], pids, "l1", mode, 1.0, prev=prev)
        assert np.array_equal(acc, prev + df)
    # the modules, forward and backward through autograd
    ft = [torch.from_numpy(v).to(DEV).requires_grad_(True) for v in f]
    pd = torch.from_numpy(pids).to(DEV)
    for crit, M, mode, dist, margin in ((hetero_loss(dist_type="l2"), 2, "hetero", "l2", 0.0), (hetero_loss(dist_type="l1"), 2, "hetero", "l1", 0.0),
                                        (hetero_loss(dist_type="cos"), 2, "hetero", "cos", 0.0),
                                        (multiModalMarginLossNew(margin=1, dist_type="l1"), 3, "margin3m", "l1", 1.0)):
        for t in ft:
            t.grad = None
        loss = crit(*ft[:M], pd)
        (2.0 * loss).backward()
        want, grads, _, _ = um.center_ref(f[:M], pids, dist, mode, margin)
        loss_tol, grad_tol, _, _ = um.center_bounds(f[:M], pids, dist, mode, margin, 2.0)
        within([loss.item()], [want], loss_tol, "%s/%s module" % (mode, dist))
        for m in range(M):
            within(ft[m].grad.cpu().numpy(), 2.0 * grads[m], grad_tol[m] + 6 * U * np.abs(2.0 * grads[m]), "%s/%s module grad %d" % (mode, dist, m))


# ============================================================================ the reference's fp32 results
def test_kernels_match_the_reference_fp32_golden():
    """The reference ran in fp32 on the CPU, so its numbers carry their own error; for the triplet loss that is the Gram
    expansion's: d2 off by ~ (D + 4) u (|x_i|^2 + |x_j|^2), i.e. relative e_g = that / d2 on d2 and e_g / 2 on d, which
    enters the loss through d_ap + d_an and every gradient weight through 1/d (selection still stable: e_g << 2^-10).
    The centre losses are the same arithmetic in another order: twice the kernel's own bound."""
    g = np.load(GOLDEN)
    x, pids, margin = g["t_x"], g["t_pids"], float(g["t_margin"])
    ref = um.triplet_ref(x, pids, margin)
    um.assert_stable(ref)
    loss_tol, grad_tol, _ = um.triplet_bounds(ref, x, x.shape[1], 1, margin)
    sq = (x.astype(np.float64) ** 2).sum(1)
    d2 = um.sq_dists(x) + np.eye(len(pids))
    e_g = float((((x.shape[1] + 4) * U * (sq[:, None] + sq[None, :])) / d2).max())
    assert e_g < um.STABLE / 8
    out, dx = run_triplet(x, pids, 1, margin)
    within(out[0:1], [float(g["t_loss"])], loss_tol + e_g * float((ref["ap"] + ref["an"]).mean()), "golden triplet loss")
    ax = np.abs(x.astype(np.float64))
    within(dx, g["t_grad"], grad_tol + (e_g + 16 * U) * (ref["absw"].sum(1)[:, None] * ax + ref["absw"] @ ax), "golden triplet grad")
    f, cp, cm = list(g["c_f"]), g["c_pids"], float(g["c_margin"])
    for key, mode, dist, M in (("h_l2", "hetero", "l2", 2), ("h_l1", "hetero", "l1", 2), ("h_cos", "hetero", "cos", 2),
                               ("m_l2", "margin3m", "l2", 3), ("m_l1", "margin3m", "l1", 3)):
        loss_tol, grad_tol, decided, signs_ok = um.center_bounds(f[:M], cp, dist, mode, cm)
        assert all(decided) and signs_ok
        out3, df = run_centre(f[:M], cp, dist, mode, cm)
        within(out3[0:1], [float(g[key + "_loss"])], 2 * loss_tol, "golden %s loss" % key)
        for m in range(M):
            within(df[m], g[key + "_grad"][m], 2 * (grad_tol[m] + 4 * U * np.abs(g[key + "_grad"][m])), "golden %s grad %d" % (key, m))


# ============================================================================ engine
def _engine(seed, fused=True, **kw):
    from ieee_amd.engine import Image3MEngine
    from ieee_amd.models import build_model
    from ieee_amd.optim import build_optimizer
    from tests.util_model import C, generated_state

    class FakeDM(object):
        num_train_pids = C
        sources = ["synthetic"]
        train_loader = []
        test_loader = {}
    m = build_model("ieee3modalPart", num_classes=C, loss="margin", pretrained=False, compute_dtype=torch.float32)
    sd = generated_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed)
    m.load_state_dict(sd)
    opt = build_optimizer(m, optim="sgd", lr=1e-3, weight_decay=5e-4, momentum=0.9, fused=fused)
    eng = Image3MEngine(FakeDM(), m, opt, margin=1, weight_m=1, weight_x=1, use_gpu=True, label_smooth=True, **kw)
    m.train()
    return eng, m


def _batch(B, seed):
    from ieee_amd import detgen
    xs = [torch.from_numpy(v) for v in detgen.generate_images(B, seed=seed, height=64, width=32)]
    pids = torch.arange(B) // 4
    return {"img": xs, "pid": pids, "camid": pids * 0, "impath": "", "timeid": pids * 0}


def test_engine_fused_triplet_step_equals_the_generic_path():
    """one step at B = 8, 64x32 images, weight_t = 1: fused (one more launch group adding into df) against the autograd path
    (criterion_t over torch.cat of the three features) on the same weights, held to the tolerances of
    tests/test_engine_gpu.py::test_autograd_path_equals_fused_path: 1e-4 relative on the summary, 1e-7 + 1e-5 max|p| on
    every parameter after the step"""
    B, seed = 8, 4
    eng_f, m_f = _engine(seed, fused=True, weight_t=1.0, margin_t=0.3)
    eng_a, m_a = _engine(seed, fused=False, weight_t=1.0, margin_t=0.3)
    assert type(eng_a.optimizer).__name__ == "SGD"
    s_f = eng_f.forward_backward(_batch(B, seed))
    s_a = eng_a.forward_backward(_batch(B, seed))
    keys = {"loss", "LossX", "LossM", "LossT", "accR", "lossR", "accN", "lossN", "accT", "lossT"}
    assert set(s_f) == keys and set(s_a) == keys
    print("LossT fused %.9g generic %.9g; loss %.9g / %.9g" % (s_f["LossT"], s_a["LossT"], s_f["loss"], s_a["loss"]))
    assert float(s_a["LossT"]) > 0
    for k in ("loss", "LossX", "LossT", "lossR", "accT"):
        assert abs(float(s_f[k]) - float(s_a[k])) < 1e-4 * max(1, abs(float(s_a[k]))), k
    expect = float(s_f["LossM"]) + float(s_f["LossX"]) + float(s_f["LossT"])
    assert abs(float(s_f["loss"]) - expect) < 1e-5 * max(1, abs(expect))            # 'loss' includes the term
    sd_f, sd_a = m_f.state_dict(), m_a.state_dict()
    for k in sd_f:
        if sd_f[k].is_floating_point():
            assert (sd_f[k] - sd_a[k]).abs().max().item() <= 1e-7 + 1e-5 * sd_a[k].abs().max().item(), k


def test_engine_weight_t_zero_is_bit_identical_to_the_engine_without_the_argument():
    B, seed = 8, 5
    eng_0, m_0 = _engine(seed, weight_t=0)
    eng_n, m_n = _engine(seed)
    s_0 = eng_0.forward_backward(_batch(B, seed))
    s_n = eng_n.forward_backward(_batch(B, seed))
    assert list(s_0) == list(s_n) == ["loss", "LossX", "LossM", "accR", "lossR", "accN", "lossN", "accT", "lossT"]
    for k in s_n:
        assert float(s_0[k]) == float(s_n[k]), k
    assert eng_0._small_ring[0][0].numel() == 39                    # the same 39-number read-back
    for k, v in m_n.state_dict().items():
        assert torch.equal(m_0.state_dict()[k], v), k
    # and a triplet term does change the step
    eng_t, m_t = _engine(seed, weight_t=1.0)
    s_t = eng_t.forward_backward(_batch(B, seed))
    assert eng_t._small_ring[0][0].numel() == 43 and float(s_t["loss"]) > float(s_n["loss"])
    assert not torch.equal(m_t.state_dict()["backbone.0.conv1.weight"], m_n.state_dict()["backbone.0.conv1.weight"])
