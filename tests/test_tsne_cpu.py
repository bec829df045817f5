"""CPU: the float64 restatement of t-SNE (tests/util_tsne.py) against sklearn's own internals where sklearn is installed,
the host-side parts of the feature-space figure (relabel, the slice order, min-max scaling, draw_points), the argument
checks of the ieee_tsne_* calls (they return before anything is launched, so they need no GPU), and the fixture of the
GPU step test."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import util_tsne as U


# ---- the restatement is sklearn's arithmetic -------------------------------------------------------------------------------
def test_restatement_matches_sklearn():
    pytest.importorskip("sklearn")
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne
    X, _ = U.clustered(60, 12, 5, 1)
    D = U.sqdist(X).astype(np.float32)
    np.fill_diagonal(D, 0.0)
    P, beta = U.affinities(D, 10.0)
    # sklearn keeps the float32 distances as they are and searches in double, as the restatement does; it normalises by
    # the sum of P where the restatement divides by 2n, and lifts every entry to at least the double epsilon
    ref = squareform(_t_sne._joint_probabilities(D, 10.0, 0))
    off = ~np.eye(60, dtype=bool)
    big = off & (ref > 1e-13)
    rel = (np.abs(P - ref)[big] / ref[big]).max()
    print("P against _joint_probabilities: %.2e relative per entry over %d entries" % (rel, big.sum()))
    assert big.sum() > 60 * 10 and rel <= 1e-12
    assert np.abs(P - ref)[off & ~big].max() <= np.finfo(np.float64).eps
    # gradient and KL: exact float64 on both sides
    Y = np.random.RandomState(2).randn(60, 2)
    Pc = squareform(P, checks=False)
    kl_ref, g_ref = _t_sne._kl_divergence(Y.ravel(), Pc, 1.0, 60, 2)
    g = U.gradient(P, Y).ravel()
    kl = U.kl(P, Y)
    print("KL %.15g vs %.15g; gradient max relative error %.2e" % (kl, kl_ref, np.abs(g - g_ref).max() / np.abs(g_ref).max()))
    assert abs(kl - kl_ref) <= 1e-12 * abs(kl_ref)
    assert np.abs(g - g_ref).max() <= 1e-12 * np.abs(g_ref).max()


def test_restatement_is_consistent():
    """without sklearn: the search hits the perplexity, P is a symmetric distribution, the shift changes nothing, and the
    gradient is the derivative of the KL divergence"""
    X, _ = U.clustered(40, 6, 4, 3)
    D = U.sqdist(X)
    P, beta = U.affinities(D, 8.0)
    _, H, _, _ = U.conditional_from_beta(D, beta)
    assert np.abs(H - np.log(8.0)).max() <= 1e-5
    assert np.array_equal(P, P.T) and abs(P.sum() - 1.0) < 1e-12 and not P.diagonal().any()
    e = np.exp(-D * beta[:, None])
    np.fill_diagonal(e, 0.0)
    np.testing.assert_allclose(P, U.joint(e / e.sum(1, keepdims=True)), rtol=1e-10)
    Y = np.random.RandomState(0).randn(40, 2)
    g = U.gradient(P, Y)
    for (i, c) in ((0, 0), (17, 1), (39, 0)):
        h = 1e-6
        Yp, Ym = Y.copy(), Y.copy()
        Yp[i, c] += h
        Ym[i, c] -= h
        assert abs((U.kl(P, Yp) - U.kl(P, Ym)) / (2 * h) - g[i, c]) < 1e-6 * max(1.0, abs(g[i, c]))
    np.testing.assert_allclose(sum(U.kl_terms(P, Y)), U.kl(P, Y))


def test_pca_init_follows_sklearns_rule():
    X, _ = U.clustered(50, 20, 5, 4)
    Y = U.pca_init(X)
    assert abs(Y[:, 0].std() - 1e-4) < 1e-16 and Y[:, 1].std() < Y[:, 0].std()
    Xc = X - X.mean(0)
    V = np.linalg.lstsq(Xc, Y, rcond=None)[0]
    assert (V[np.abs(V).argmax(0), np.arange(2)] > 0).all()
    pytest.importorskip("sklearn")
    from sklearn.decomposition import PCA
    ref = PCA(n_components=2, svd_solver="full").fit_transform(X)
    np.testing.assert_allclose(Y, ref / ref[:, 0].std() * 1e-4, rtol=1e-8, atol=1e-14)


# ---- host-side parts of the figure -----------------------------------------------------------------------------------------
def test_relabel_counts_changes():
    from ieee_amd.reidtools import relabel
    assert relabel([7, 7, 3, 3, 3, 7, 9]) == [0, 0, 1, 1, 1, 2, 3]
    assert relabel([5]) == [0] and relabel([]) == []


def test_slices_are_taken_by_position_and_scaled_per_slice_and_axis():
    from ieee_amd.reidtools import minmax_scale, modality_slices
    f = torch.arange(4 * 2304, dtype=torch.float32).reshape(4, 2304)
    s = modality_slices(f)
    assert tuple(s.shape) == (3, 4, 768)
    for m in range(3):
        assert torch.equal(s[m], f[:, 768 * m:768 * (m + 1)])
    with pytest.raises(ValueError):
        modality_slices(f[:, :2000])
    c = torch.tensor(np.random.RandomState(0).randn(3, 9, 2) * [[[1.0, 50.0]], [[3.0, 0.1]], [[7.0, 7.0]]])
    z = minmax_scale(c)
    assert torch.equal(z.min(1).values, torch.zeros(3, 2, dtype=c.dtype))
    assert torch.equal(z.max(1).values, torch.ones(3, 2, dtype=c.dtype))
    np.testing.assert_allclose(z[1, :, 1].numpy(), ((c[1, :, 1] - c[1, :, 1].min()) / (c[1, :, 1].max() - c[1, :, 1].min())).numpy())


def test_draw_points_draws_the_selected_identities_only(tmp_path):
    from PIL import Image
    from ieee_amd.reidtools import TSNE_COLORS, draw_points
    # a 5 x 4 grid of positions per slice, the slices shifted against each other; identities 0..4, four rows each
    gx, gy = np.meshgrid(np.linspace(0.05, 0.85, 5), np.linspace(0.05, 0.95, 4))
    base = np.stack([gx.ravel(), gy.ravel()], 1)
    coords = np.stack([base, base + [0.05, 0.0], base + [0.10, 0.0]])
    labels = [i // 4 for i in range(20)]
    path = draw_points(coords, labels, [3, 1], str(tmp_path / "fig" / "[3, 1].jpg"))
    assert os.path.exists(path)
    with Image.open(path) as im:
        assert im.size == (2000, 2000) and im.mode == "RGB" and im.format == "JPEG"
        px = np.asarray(im).astype(np.int64)
    yy, xx = np.mgrid[0:2000, 0:2000]
    near = np.zeros((2000, 2000), dtype=bool)
    for m in range(3):
        for i, lab in enumerate(labels):
            cx, cy = 200 + coords[m, i, 0] * 1600, 1800 - coords[m, i, 1] * 1600
            spot = (xx - cx) ** 2 + (yy - cy) ** 2 <= 32 ** 2        # markers are under 20 pixels in radius; JPEG blocks are 8
            centre = px[int(round(cy)), int(round(cx))]
            if lab in (3, 1):
                near |= spot
                want = np.asarray(TSNE_COLORS[[3, 1].index(lab)])
                blend = 255 + 0.4 * (want - 255)                     # alpha 0.4 over white
                assert np.abs(centre - blend).max() <= 12, (m, i, centre, blend)
            else:
                assert centre.min() >= 250, (m, i, centre)           # an identity that was not selected: nothing there
    assert px[~near].min() >= 250                                    # white everywhere else
    assert (px[near].min(-1) < 240).sum() > 12 * 300                 # and 12 markers that are not
    with pytest.raises(ValueError):
        draw_points(coords[:2], labels, [1], str(tmp_path / "x.jpg"))


# ---- the C ABI's argument checks, and the loud failures ----------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    from ieee_amd import _lib
    lib = _lib.load()
    p, nul = ctypes.c_void_p(4096), ctypes.c_void_p(0)      # never dereferenced: every call below returns at its checks
    big = 1 << 40

    def aff(dist=p, ldd=100, n=100, batch=3, perp=10.0, P=p, ldp=100, beta=p, work=p, nbytes=big):
        return lib.ieee_tsne_affinities(dist, ldd, n, batch, perp, P, ldp, beta, work, nbytes, nul)

    def run(P=p, ldp=100, n=100, batch=3, Y=p, iter0=0, n_iter=1, work=p, nbytes=big):
        return lib.ieee_tsne_run(P, ldp, n, batch, Y, p, p, iter0, n_iter, 250, 12.0, 50.0, nul, work, nbytes, nul)

    for call, kw, msg in [(aff, dict(dist=nul), b"null pointer"), (aff, dict(beta=nul), b"null pointer"),
                          (aff, dict(n=3, ldd=3, perp=1.0), b"at least 4"), (aff, dict(n=12289, ldd=12289, ldp=12292), b"cap"),
                          (aff, dict(batch=0), b"batch"), (aff, dict(perp=100.0), b"perplexity"), (aff, dict(perp=0.0), b"perplexity"),
                          (aff, dict(ldd=99), b"ldd"), (aff, dict(ldp=96), b"ldp"), (aff, dict(ldp=102), b"ldp"),
                          (aff, dict(P=ctypes.c_void_p(4100)), b"aligned"), (aff, dict(nbytes=1024), b"workspace too small"),
                          (run, dict(P=nul), b"null pointer"), (run, dict(n=2), b"at least 4"), (run, dict(batch=-1), b"batch"),
                          (run, dict(ldp=98), b"ldp"), (run, dict(Y=ctypes.c_void_p(4100)), b"aligned"),
                          (run, dict(n_iter=-1), b"negative"), (run, dict(nbytes=1024), b"workspace too small")]:
        assert call(**kw) == -1, kw                         # IEEE_ERR_BAD_ARG
        err = lib.ieee_last_error()
        assert msg in err and (b"tsne_affinities:" if call is aff else b"tsne_run:") in err, (kw, err)
    assert lib.ieee_tsne_workspace_bytes(3, 1) == -1 and b"tsne_workspace_bytes" in lib.ieee_last_error()
    assert lib.ieee_tsne_workspace_bytes(12289, 3) == -1
    assert lib.ieee_tsne_workspace_bytes(100, 0) == -1
    fields = (ctypes.c_int64 * 6)()
    assert lib.ieee_tsne_layout(2, 1, fields) == -1 and b"tsne_layout" in lib.ieee_last_error()
    assert lib.ieee_tsne_layout(836, 3, fields) == 0
    slabs, part, rows, rowconst, scal, sums = list(fields)
    assert (slabs, sums) == (2, 6) and part == 0
    assert rows >= 3 * slabs * 6 * 836 * 4 and rowconst >= rows + 3 * 6 * 836 * 4 and scal >= rowconst + 3 * 2 * 836 * 4
    assert lib.ieee_tsne_workspace_bytes(836, 3) >= scal + 3 * 8 * 4
    # the stated size: P for batch = 3 at the cap plus the workspace stay under 2 GiB
    assert 3 * 12288 * 12288 * 4 + lib.ieee_tsne_workspace_bytes(12288, 3) < 2 << 30


def test_perplexity_not_below_n_is_a_value_error():
    from ieee_amd.reidtools import tsne_embed
    with pytest.raises(ValueError, match="perplexity must be less than n_samples"):
        tsne_embed(torch.zeros(30, 8))                      # the default perplexity of 30
    with pytest.raises(ValueError, match="perplexity must be less than n_samples"):
        tsne_embed(torch.zeros(3, 12, 8), perplexity=12.0)
    with pytest.raises(ValueError):
        tsne_embed(torch.zeros(8))


def test_tsne_embed_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ieee_amd import _lib
    from ieee_amd.reidtools import show_points_multimodal, tsne_embed
    with pytest.raises(_lib.IeeeAmdError):
        tsne_embed(torch.zeros(40, 8))
    with pytest.raises(_lib.IeeeAmdError):
        show_points_multimodal(torch.zeros(40, 2304), list(range(40)), [1, 2], "unused")


def test_vistsne_refused_when_sharded_or_training(monkeypatch):
    from ieee_amd import dist as ddp
    from ieee_amd.engine import Engine

    class DM(object):
        train_loader, test_loader, sources = [], {}, []
    eng = Engine(DM(), use_gpu=False)
    with pytest.raises(ValueError, match="vistsne"):
        eng.run(test_only=False, vistsne=True)
    monkeypatch.setattr(ddp, "world_size", lambda: 2)
    with pytest.raises(RuntimeError, match="one GPU"):
        eng._evaluate(dataset_name="x", vistsne=True)


# ---- the fixture of the GPU step test ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", [1e-4, 10.0])
@pytest.mark.parametrize("n", [33, 257])
def test_step_fixture_leaves_few_undecidable_gain_branches(n, spread):
    """tests/test_tsne_gpu.py leaves out the elements whose update * g lies within its own fp32 error bound of 0 and allows
    at most 2 % of them: here the float64 restatement runs the same five steps beside an fp32 copy of itself, and the
    elements the same rule leaves out stay under that cap at every step."""
    P, Y0 = U.step_fixture(n, 3, spread)
    lr = 50.0
    for b in range(3):
        Y, upd, gains = Y0[b].astype(np.float64), np.zeros((n, 2)), np.ones((n, 2))
        for it in range(5):
            alpha = 12.0 if it < 2 else 1.0
            sums, mags, Z = U.row_sums(P[b], Y)
            g = U.gradient(P[b], Y, alpha)
            g_err = U.gradient_error_bound(sums, mags, Z, alpha, n)
            out = np.abs(upd * g) <= np.abs(upd) * g_err
            out &= upd != 0                                  # update = 0: the product is exactly 0 on both sides, gains * 0.8
            assert out.mean() <= 0.02, (n, spread, b, it, out.mean())
            Y32, upd32, gains32, _ = (a.astype(np.float32) for a in U.step(P[b], Y, upd, gains, it, 2, 12.0, lr))
            Y, upd, gains = Y32.astype(np.float64), upd32.astype(np.float64), gains32.astype(np.float64)
