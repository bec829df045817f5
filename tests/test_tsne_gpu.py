"""GPU: descriptor t-SNE on the device -- ieee_tsne_affinities and ieee_tsne_run against the float64 restatement
(tests/util_tsne.py; that it is sklearn's arithmetic: tests/test_tsne_cpu.py), tsne_embed end to end against float64
control runs, and Engine.test(vistsne=True) on in-memory loaders."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import util_tsne as U

pytestmark = pytest.mark.gpu

U24 = U.U24


def P_RTOL(n):
    """per element of P, in roundings of 2^-24: the worst sequential fp32 sum of n terms, an exponent argument of up to 88
    rounded once, and a few more (expf, the division by S, the sum of the two conditionals, the division by 2n).  The kernel
    sums each row as a tree (ceil(n / 256) + 9 adds) and forms the argument in double, so it sits inside this."""
    return (n + 96) * U24


P_ATOL = 2.0 ** -126      # a conditional below the smallest normal fp32 may have been flushed

# eps_H, the fp32 evaluation error of the entropy for the search kernel's own summation order: derived in
# tests/util_tsne.py::entropy_eps from the float64 terms of every row (the rounded exponent argument and expf on every
# term, weighted by dH/d(log e_j); the tree sums of S and T; logf, the division and the add).  For these fixtures it is
# between 1e-6 and 4e-6 per row, under the search's own tolerance of 1e-5.


def _lib():
    from ieee_amd import _lib as L
    return L, L.require_gpu()


def _workspace(lib, n, batch):
    nbytes = lib.ieee_tsne_workspace_bytes(n, batch)
    assert nbytes > 0
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), nbytes


def _affinities(dist, perplexity, ldp, fill=float("nan")):
    L, lib = _lib()
    batch, n, ldd = dist.shape
    P = torch.full((batch, n, ldp), fill, dtype=torch.float32, device="cuda")
    beta = torch.full((batch, n), fill, dtype=torch.float32, device="cuda")
    work, nbytes = _workspace(lib, n, batch)
    status = lib.ieee_tsne_affinities(L.ptr(dist), ldd, n, batch, perplexity, L.ptr(P), ldp, L.ptr(beta), L.ptr(work), nbytes,
                                      L.stream())
    return status, P, beta


@pytest.mark.parametrize("variant", U.AFFINITY_VARIANTS)
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [33, 100, 257])
def test_affinities_match_float64(n, batch, variant):
    perplexity = 5.0 if n == 33 else 10.0
    D = U.affinity_dist(n, batch, variant)
    ldd, ldp = n + 1, (n + 3) // 4 * 4                      # a row stride of its own on both sides
    dist = torch.full((batch, n, ldd), float("nan"), dtype=torch.float32, device="cuda")
    dist[:, :, :n] = torch.from_numpy(D).cuda()
    status, P, beta = _affinities(dist, perplexity, ldp)
    assert status == 0
    status2, P2, beta2 = _affinities(dist, perplexity, ldp)
    assert status2 == 0 and torch.equal(P, P2) and torch.equal(beta, beta2)          # (d) the same bits
    Ph, bh = P.cpu().numpy(), beta.cpu().numpy()
    assert not Ph[:, :, n:].any()                                                   # pad columns: zero
    off = ~np.eye(n, dtype=bool)
    for b in range(batch):
        got = Ph[b, :, :n]
        cond, H, a, S = U.conditional_from_beta(D[b], bh[b])
        eps = U.entropy_eps(a, cond, S, n) + U24 * np.log(perplexity)
        miss = np.abs(H - np.log(perplexity))
        print("n=%d batch %d/%d %s: beta %.3g..%.3g, |H - log perplexity| max %.3e (eps_H max %.2e)"
              % (n, b, batch, variant, bh[b].min(), bh[b].max(), miss.max(), eps.max()))
        assert (miss <= 1e-5 + eps).all(), np.argmax(miss - eps)                    # (a)
        ref = U.joint(cond)
        err = np.abs(got - ref)
        print("   P: max error %.3e of the entry (bound %.3e), sum - 1 = %.3e"
              % ((err[off] / np.maximum(ref[off], P_ATOL)).max(), P_RTOL(n), got.astype(np.float64).sum() - 1.0))
        assert (err <= P_RTOL(n) * ref + P_ATOL).all()                              # (b)
        assert np.array_equal(got, got.T) and not got.diagonal().any()              # (c)
        assert abs(got.astype(np.float64).sum() - 1.0) <= P_RTOL(n)
    if variant == "x1e4":
        assert bh.max() < 2.0 ** -9                          # beta had to halve, many times
    if variant == "x1e-4":
        assert np.median(bh) > 2.0 ** 6                      # and to double (the outlier's own row excepted)


def test_affinities_refuse_bad_arguments_and_launch_nothing():
    L, lib = _lib()
    n, batch = 33, 2
    dist = torch.from_numpy(U.affinity_dist(n, batch, "plain")).cuda()
    P = torch.full((batch, n, 36), 7.0, device="cuda")
    beta = torch.full((batch, n), 7.0, device="cuda")
    work, nbytes = _workspace(lib, n, batch)

    def call(n_=n, batch_=batch, perp=5.0, ldd=n, ldp=36, nbytes_=nbytes):
        return lib.ieee_tsne_affinities(L.ptr(dist), ldd, n_, batch_, perp, L.ptr(P), ldp, L.ptr(beta), L.ptr(work), nbytes_,
                                        L.stream())
    for kw in (dict(n_=3, perp=2.0), dict(perp=33.0), dict(perp=40.0), dict(batch_=0), dict(nbytes_=nbytes - 1), dict(ldd=32),
               dict(ldp=32), dict(ldp=35), dict(n_=12289)):
        assert call(**kw) == -1, kw                          # IEEE_ERR_BAD_ARG
        with pytest.raises(L.IeeeAmdError, match="tsne_affinities"):
            L.check(-1)
    Y = torch.full((batch, n, 2), 7.0, device="cuda")
    for kw in (dict(n=3), dict(batch=0), dict(nbytes=nbytes - 1), dict(ldp=35), dict(n_iter=-1)):
        a = dict(n=n, batch=batch, nbytes=nbytes, ldp=36, n_iter=1)
        a.update(kw)
        assert lib.ieee_tsne_run(L.ptr(P), a["ldp"], a["n"], a["batch"], L.ptr(Y), L.ptr(Y), L.ptr(Y), 0, a["n_iter"], 250, 12.0,
                                 50.0, None, L.ptr(work), a["nbytes"], L.stream()) == -1, kw
        with pytest.raises(L.IeeeAmdError, match="tsne_run"):
            L.check(-1)
    torch.cuda.synchronize()
    assert bool((P == 7.0).all()) and bool((beta == 7.0).all()) and bool((Y == 7.0).all())     # nothing was launched
    assert not work.any()


# ---- one step at a time ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", [1e-4, 10.0], ids=["tiny", "spread10"])
@pytest.mark.parametrize("n", [33, 257])
def test_single_steps_match_float64(n, spread):
    """Five ieee_tsne_run(n_iter=1, iter0=t) calls that carry Y / update / gains, exaggeration_iters = 2: after each, the
    float64 step applied to the state the device had before it.  Bounds: every per-row sum and Z within (n + 16) 2^-24 of
    the summed magnitudes of their terms (tests/util_tsne.py::sum_rtol), the KL within that factor of the summed
    magnitudes of its three terms, and Y / update / gains within what those imply through learning_rate * gains
    (gradient_error_bound).  Elements whose update * g is within its own error bound of 0 have an undecidable gain branch
    and are left out, at most 2 % of them (tests/test_tsne_cpu.py checks that cap on the float64 / fp32 pair)."""
    L, lib = _lib()
    batch, lr, exag_iters, exag = 3, 50.0, 2, 12.0
    P64, Y0 = U.step_fixture(n, batch, spread)
    ldp = (n + 3) // 4 * 4
    P = torch.zeros((batch, n, ldp), dtype=torch.float32, device="cuda")
    P[:, :, :n] = torch.from_numpy(P64.astype(np.float32)).cuda()
    Y = torch.from_numpy(Y0).cuda()
    upd, gains = torch.zeros_like(Y), torch.ones_like(Y)
    work, nbytes = _workspace(lib, n, batch)
    fields = (ctypes.c_int64 * 6)()
    assert lib.ieee_tsne_layout(n, batch, fields) == 0
    slabs, _, rows_at, _, scal_at, nsums = list(fields)
    assert nsums == 6 and slabs == -(-n // 512)
    r = U.sum_rtol(n)
    for it in range(5):
        before = [t.cpu().numpy().astype(np.float64) for t in (Y, upd, gains)]
        hist = torch.full((batch, 1, 2), float("nan"), device="cuda")
        assert lib.ieee_tsne_run(L.ptr(P), ldp, n, batch, L.ptr(Y), L.ptr(upd), L.ptr(gains), it, 1, exag_iters, exag, lr,
                                 L.ptr(hist), L.ptr(work), nbytes, L.stream()) == 0
        w = work.cpu()
        rows = w[rows_at:rows_at + batch * 6 * n * 4].view(torch.float32).numpy().reshape(batch, 6, n).astype(np.float64)
        scal = w[scal_at:scal_at + batch * 8 * 4].view(torch.float32).numpy().reshape(batch, 8).astype(np.float64)
        after = [t.cpu().numpy().astype(np.float64) for t in (Y, upd, gains)]
        hist = hist.cpu().numpy().astype(np.float64)
        alpha, momentum = (exag, 0.5) if it < exag_iters else (1.0, 0.8)
        for b in range(batch):
            y0, u0, g0 = (a[b] for a in before)
            sums, mags, Z = U.row_sums(P64[b], y0)
            worst = (np.abs(rows[b] - sums) / (r * mags + 1e-300)).max()
            assert (np.abs(rows[b] - sums) <= r * mags).all(), (it, b, worst)
            assert abs(scal[b, 0] - Z) <= r * Z, (it, b)
            t3 = U.kl_terms(P64[b], y0)
            kl_err = abs(hist[b, 0, 0] - sum(t3))
            assert kl_err <= r * sum(abs(t) for t in t3), (it, b, hist[b, 0, 0], sum(t3))
            g = U.gradient(P64[b], y0, alpha)
            g_err = U.gradient_error_bound(sums, mags, Z, alpha, n)
            gnorm = np.sqrt((g ** 2).sum())
            assert abs(hist[b, 0, 1] - gnorm) <= np.sqrt((g_err ** 2).sum()) + U.sum_rtol(2 * n) * gnorm, (it, b)
            y1, u1, g1, _ = U.step(P64[b], y0, u0, g0, it, exag_iters, exag, lr)
            keep = ~((np.abs(u0 * g) <= np.abs(u0) * g_err) & (u0 != 0))
            left_out = 1.0 - keep.mean()
            assert left_out <= 0.02, (it, b, left_out)
            gain_err = 3 * U24 * g1
            u_err = lr * (g1 * g_err + gain_err * np.abs(g)) + 4 * U24 * (momentum * np.abs(u0) + lr * g1 * np.abs(g))
            y_err = u_err + U24 * (np.abs(y0) + np.abs(y1))
            for name, got, want, tol in (("gains", after[2][b], g1, gain_err), ("update", after[1][b], u1, u_err),
                                         ("Y", after[0][b], y1, y_err)):
                bad = (np.abs(got - want) > tol) & keep
                assert not bad.any(), (name, it, b, int(bad.sum()), np.abs(got - want)[keep].max())
            if b == 0:
                print("n=%d spread=%g step %d: sums at %.2f of their bound, KL %.6f (error %.1e), |g| %.3e, %.1f%% left out"
                      % (n, spread, it, worst, hist[b, 0, 0], kl_err, gnorm, 100 * left_out))


def test_a_run_is_its_steps():
    """n_iter = 5 in one call gives the bits of five calls of one, history included, and a NULL history changes nothing"""
    L, lib = _lib()
    n, batch = 100, 3
    P64, Y0 = U.step_fixture(n, batch, 1.0)
    P = torch.from_numpy(P64.astype(np.float32)).cuda().contiguous()
    work, nbytes = _workspace(lib, n, batch)

    def go(chunks, with_history):
        Y = torch.from_numpy(Y0).cuda()
        upd, gains = torch.zeros_like(Y), torch.ones_like(Y)
        hists, at = [], 0
        for k in chunks:
            h = torch.zeros((batch, k, 2), device="cuda") if with_history else None
            assert lib.ieee_tsne_run(L.ptr(P), n, n, batch, L.ptr(Y), L.ptr(upd), L.ptr(gains), at, k, 2, 12.0, 50.0, L.ptr(h),
                                     L.ptr(work), nbytes, L.stream()) == 0
            at += k
            hists.append(h)
        return Y, upd, gains, (torch.cat(hists, 1) if with_history else None)
    one = go([5], True)
    for other in (go([1, 1, 1, 1, 1], True), go([2, 3], True)):
        assert all(torch.equal(a, b) for a, b in zip(one, other))
    bare = go([5], False)
    assert all(torch.equal(a, b) for a, b in zip(one[:3], bare[:3]))
    assert bool(torch.isfinite(one[3]).all()) and bool((one[3][:, :, 1] > 0).all())


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def controls():
    """the float64 restatement run from the PCA start and from four +-2^-12 jitters of it, per slice (about a second each)"""
    X, label = U.end_to_end_features()
    rng = np.random.RandomState(9)
    out = []
    for m in range(3):
        Xs = X[:, 768 * m:768 * (m + 1)].astype(np.float64)
        P, _ = U.affinities(U.sqdist(Xs), 30.0)
        Y0 = U.pca_init(Xs)
        starts = [Y0] + [Y0 * (1.0 + 2.0 ** -12 * rng.choice([-1.0, 1.0], size=Y0.shape)) for _ in range(4)]
        out.append((P, Y0, [U.run(P, s, learning_rate=50.0)[1] for s in starts]))
    return X, label, out


def test_tsne_embed_end_to_end(controls):
    from ieee_amd.reidtools import modality_slices, tsne_embed
    X, label, ctl = controls
    feats = modality_slices(torch.from_numpy(X).cuda())
    assert tuple(feats.shape) == (3, 100, 768)
    Y, info = tsne_embed(feats, return_info=True)
    assert Y.dtype == torch.float32 and tuple(Y.shape) == (3, 100, 2) and Y.is_cuda
    assert tuple(info["kl_history"].shape) == (3, 1000) and tuple(info["grad_norm_history"].shape) == (3, 1000)
    assert tuple(info["beta"].shape) == (3, 100) and tuple(info["kl_divergence"].shape) == (3,)
    assert torch.equal(info["kl_divergence"], info["kl_history"][:, -1])
    Yh = Y.cpu().numpy().astype(np.float64)
    for m in range(3):
        P, Y0, kls = ctl[m]
        purity = U.purity_1nn(Yh[m], label)
        final = U.kl(P, Yh[m])
        reported = float(info["kl_divergence"][m])
        limit = max(kls) + (max(kls) - min(kls))
        print("slice %d: float64 controls %.4f..%.4f, device KL %.4f (its own last history value %.4f), limit %.4f, purity %.2f"
              % (m, min(kls), max(kls), final, reported, limit, purity))
        assert purity == 1.0
        assert final <= limit and reported <= limit
    # the same bits on a second call; one problem alone is that problem of the batch
    again = tsne_embed(feats)
    assert torch.equal(again, Y)
    assert torch.equal(tsne_embed(feats[1]), Y[1])


def test_tsne_embed_init_and_devices(controls):
    from ieee_amd.reidtools import tsne_embed
    X, label, ctl = controls
    x = torch.from_numpy(X[:, :768])
    # the PCA start is sklearn's: against the float64 restatement (eigenvectors of the covariance against an SVD)
    y_pca = tsne_embed(x.cuda(), n_iter=0)
    np.testing.assert_allclose(y_pca.cpu().numpy(), ctl[0][1], rtol=1e-5, atol=1e-9)
    # an explicit start is used as given
    init = torch.from_numpy(np.random.RandomState(1).randn(100, 2).astype(np.float32))
    assert torch.equal(tsne_embed(x.cuda(), n_iter=0, init=init), init.cuda())
    assert init.device.type == "cpu"
    # CPU in, CPU out, and the same numbers as from the device
    y_cpu, info = tsne_embed(x, n_iter=20, init=init, return_info=True)
    assert y_cpu.device.type == "cpu" and info["beta"].device.type == "cpu" and tuple(info["kl_history"].shape) == (20,)
    assert torch.equal(y_cpu, tsne_embed(x.cuda(), n_iter=20, init=init.cuda()).cpu())
    # 'random' draws from the generator it is given
    g = torch.Generator(device="cuda")
    a = tsne_embed(x.cuda(), n_iter=0, init="random", generator=g.manual_seed(5))
    b = tsne_embed(x.cuda(), n_iter=0, init="random", generator=g.manual_seed(5))
    assert torch.equal(a, b) and 5e-5 < float(a.std()) < 2e-4
    with pytest.raises(ValueError):
        tsne_embed(x.cuda(), init="spectral")
    with pytest.raises(ValueError):
        tsne_embed(x.cuda(), init=init[:50])


# ---- the engine ----------------------------------------------------------------------------------------------------------------
def test_engine_test_vistsne(tmp_path, capsys):
    from PIL import Image
    from ieee_amd.engine import MultiModalImageSoftmaxEngine
    from ieee_amd.models import build_model
    from ieee_amd.optim import build_optimizer
    from tests.util_model import C, id_loader

    class DM(object):
        num_train_pids = C
        sources = ["synthetic"]
        train_loader = []

        def __init__(self):
            qp, qc = np.arange(36) // 4, np.zeros(36, dtype=np.int64)         # nine identities, four images each
            gp, gc = np.arange(20) % 9, np.ones(20, dtype=np.int64)
            self.test_loader = {"synthetic": {"query": id_loader(36, 1, qp, qc), "gallery": id_loader(20, 2, gp, gc)}}

    m = build_model("ieee3modalPart", num_classes=C, loss="softmax", pretrained=False, compute_dtype=torch.float32)
    eng = MultiModalImageSoftmaxEngine(DM(), m, build_optimizer(m, optim="sgd", lr=1e-3), use_gpu=True)
    plain = eng.test(save_dir=str(tmp_path / "plain"), ranks=[1])
    capsys.readouterr()
    assert not os.path.exists(str(tmp_path / "plain"))                       # without the flag nothing is written
    assert eng.test(vistsne=True, vistsne_labels=[1, 2, 3], save_dir=str(tmp_path / "vis"), ranks=[1]) == plain
    printed = capsys.readouterr().out
    folder = tmp_path / "vis" / "vistsne_synthetic"
    assert os.listdir(str(folder)) == ["[1, 2, 3].jpg"]
    assert "Draw points of features to {}".format(folder / "[1, 2, 3].jpg") in printed
    assert printed.index("** Results **") < printed.index("Draw points")     # after the results are printed
    with Image.open(str(folder / "[1, 2, 3].jpg")) as im:
        assert im.size == (2000, 2000) and im.mode == "RGB"
        px = np.asarray(im)
    assert (px.min(-1) < 240).sum() > 1000                                   # markers were drawn
    # drawn labels default to the reference's random.sample(range(1, 30), 6)
    eng.run(test_only=True, vistsne=True, save_dir=str(tmp_path / "vis2"), ranks=[1])
    (name,) = os.listdir(str(tmp_path / "vis2" / "vistsne_synthetic"))
    drawn = [int(v) for v in name[1:-len("].jpg")].split(", ")]
    assert name == str(drawn) + ".jpg" and len(set(drawn)) == 6 and all(1 <= v < 30 for v in drawn)
