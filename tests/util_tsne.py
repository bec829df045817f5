"""A float64 numpy restatement of exact t-SNE as include/ieee_amd.h states it (ieee_tsne_affinities, ieee_tsne_run): the
perplexity search on shifted distances, the joint matrix, one step of sklearn's _gradient_descent schedule and the KL
divergence -- plus the fixtures the t-SNE tests share.  Everything is generated in code."""
import numpy as np

U24 = 2.0 ** -24                                   # half an fp32 ulp, relative: one rounding to nearest


# ---- affinities ----------------------------------------------------------------------------------------------------------
def shifted(dist):
    """d'_ij = d_ij - min_{k != i} d_ik, float64, diagonal 0"""
    d = np.asarray(dist, dtype=np.float64)
    n = d.shape[0]
    off = d + np.where(np.eye(n, dtype=bool), np.inf, 0.0)
    out = d - off.min(1, keepdims=True)
    out[np.eye(n, dtype=bool)] = 0.0
    return out


def conditional_from_beta(dist, beta):
    """rows p_{j|i} for given betas, and what the entropy bound needs: (cond [n][n], H [n], a [n][n], S [n])"""
    n = dist.shape[0]
    a = shifted(dist) * np.asarray(beta, dtype=np.float64)[:, None]
    e = np.exp(-a)
    e[np.eye(n, dtype=bool)] = 0.0
    S = e.sum(1)
    cond = e / S[:, None]
    H = np.log(S) + (a * cond).sum(1)
    return cond, H, a, S


def joint(cond):
    n = cond.shape[0]
    return (cond + cond.T) / (2.0 * n)


def search_beta(dist, perplexity, tol=1e-5, steps=100):
    """sklearn/manifold/_utils.pyx::_binary_search_perplexity, row by row, on the shifted distances"""
    dp = shifted(dist)
    n = dp.shape[0]
    target = np.log(perplexity)
    beta = np.ones(n)
    off = ~np.eye(n, dtype=bool)
    for i in range(n):
        d = dp[i][off[i]]
        b, lo, hi = 1.0, -np.inf, np.inf
        for _ in range(steps):
            e = np.exp(-b * d)
            S = e.sum()
            diff = np.log(S) + b * (d * e).sum() / S - target
            if abs(diff) <= tol:
                break
            if diff > 0:
                lo = b
                b = b * 2.0 if hi == np.inf else (b + hi) / 2.0
            else:
                hi = b
                b = b / 2.0 if lo == -np.inf else (b + lo) / 2.0
        beta[i] = b
    return beta


def affinities(dist, perplexity):
    beta = search_beta(dist, perplexity)
    return joint(conditional_from_beta(dist, beta)[0]), beta


def entropy_eps(a, cond, S, n):
    """eps_H: how far the fp32 evaluation of H = log S + sum_j a_j e_j / S (a_j = beta d'_j, e_j = exp(-a_j)) in the search
    kernel can lie from the exact entropy of the same beta, per row, in units worked out from the kernel's own order:
      e_j carries (a_j + 2) roundings: the argument is formed in double and rounded once (a_j 2^-24 absolute in the exponent)
        and expf is good to one ulp; with p_j = e_j / S, dH/d(log e_j) = p_j (1 + a_j - abar), abar = sum_j p_j a_j
      the product a_j e_j adds one rounding to the T terms: sum_j p_j a_j = abar
      S and T are sums of non-negative terms, each lane ceil(n / 256) sequential adds, 6 butterfly levels, 3 adds across the
        waves: m = ceil(n / 256) + 9 roundings each; dH/d(log S) = 1 - abar ... bounded by 1 + abar, dH/d(log T) = abar
      logf(S) (one ulp of log S), the division T / S and the final add: 2 |log S| + 2 abar + (|log S| + abar)"""
    abar = (a * cond).sum(1)
    m = -(-n // 256) + 9
    terms = (cond * np.abs(1.0 + a - abar[:, None]) * (a + 2.0)).sum(1) + abar
    return U24 * (terms + m * (1.0 + 2.0 * abar) + 3.0 * (np.abs(np.log(S)) + abar))


# ---- the descent -----------------------------------------------------------------------------------------------------------
ROW_SUMS = ("attr_x", "attr_y", "rep_x", "rep_y", "w", "plogq")


def row_sums(P, Y):
    """the six per-row sums of ieee_tsne_layout, their absolute-value counterparts, and Z (with its own)"""
    n = P.shape[0]
    diff = Y[:, None, :] - Y[None, :, :]
    q = 1.0 + (diff ** 2).sum(2)
    w = 1.0 / q
    w[np.eye(n, dtype=bool)] = 0.0
    Pz = np.where(np.eye(n, dtype=bool), 0.0, P)
    pw = Pz * w
    terms = [pw * diff[:, :, 0], pw * diff[:, :, 1], w * w * diff[:, :, 0], w * w * diff[:, :, 1], w, Pz * np.log(q)]
    sums = np.stack([t.sum(1) for t in terms])
    mags = np.stack([np.abs(t).sum(1) for t in terms])
    return sums, mags, w.sum()


def kl_terms(P, Y):
    """(sum P log P, sum P log(1 + d^2), (sum P) log Z): KL is their sum; zero entries of P contribute 0"""
    sums, _, Z = row_sums(P, Y)
    Pz = np.where(np.eye(P.shape[0], dtype=bool), 0.0, P)
    pos = Pz[Pz > 0]
    return (pos * np.log(pos)).sum(), sums[5].sum(), Pz.sum() * np.log(Z)


def kl(P, Y):
    return sum(kl_terms(P, Y))


def gradient(P, Y, alpha=1.0):
    sums, _, Z = row_sums(P, Y)
    return 4.0 * (alpha * sums[0:2].T - sums[2:4].T / Z)


def step(P, Y, update, gains, it, exaggeration_iters, early_exaggeration, learning_rate):
    """one iteration of sklearn's _gradient_descent with the exaggeration schedule; returns (Y, update, gains, g)"""
    early = it < exaggeration_iters
    g = gradient(P, Y, early_exaggeration if early else 1.0)
    inc = update * g < 0.0
    gains = np.maximum(np.where(inc, gains + 0.2, gains * 0.8), 0.01)
    update = (0.5 if early else 0.8) * update - learning_rate * (gains * g)
    return Y + update, update, gains, g


def run(P, Y, n_iter=1000, exaggeration_iters=250, early_exaggeration=12.0, learning_rate=50.0, dtype=np.float64):
    """the whole schedule in `dtype`; returns (Y, KL of the final Y)"""
    P = P.astype(dtype)
    Y = Y.astype(dtype)
    update, gains = np.zeros_like(Y), np.ones_like(Y)
    eye = np.eye(P.shape[0], dtype=bool)
    four, one = dtype(4.0), dtype(1.0)
    for it in range(n_iter):
        early = it < exaggeration_iters
        diff = Y[:, None, :] - Y[None, :, :]
        w = one / (one + (diff ** 2).sum(2))
        w[eye] = 0
        pw = P * w * (dtype(early_exaggeration) if early else one)
        g = four * ((pw[:, :, None] * diff).sum(1) - ((w * w)[:, :, None] * diff).sum(1) / w.sum())
        inc = update * g < 0
        gains = np.maximum(np.where(inc, gains + dtype(0.2), gains * dtype(0.8)), dtype(0.01))
        update = dtype(0.5 if early else 0.8) * update - dtype(learning_rate) * (gains * g)
        Y = Y + update
    return Y, float(kl(P.astype(np.float64), Y.astype(np.float64)))


def pca_init(X):
    """sklearn's init='pca': top two principal axes, each signed so that its largest-magnitude loading is positive, the
    projection scaled so that its first column has standard deviation 1e-4"""
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(0)
    _, _, Vt = np.linalg.svd(Xc, full_matrices=False)
    V = Vt[:2]
    sign = np.sign(V[np.arange(2), np.abs(V).argmax(1)])
    Y = Xc @ (V * sign[:, None]).T
    return Y / Y[:, 0].std() * 1e-4


# ---- fixtures --------------------------------------------------------------------------------------------------------------
def sqdist(X):
    X = np.asarray(X, dtype=np.float64)
    s = (X ** 2).sum(1)
    return np.maximum(s[:, None] + s[None, :] - 2.0 * X @ X.T, 0.0)


def clustered(n, d, ids, seed, centre_scale=2.0):
    """n points in d dimensions around `ids` centres (centre scale 2, unit noise); returns (X, identity of every row)"""
    rng = np.random.RandomState(seed)
    centres = centre_scale * rng.randn(ids, d)
    label = np.arange(n) % ids
    return centres[label] + rng.randn(n, d), label


AFFINITY_VARIANTS = ("plain", "x1e4", "x1e-4")


def affinity_dist(n, batch, variant, seed=0):
    """fp32 squared distances [batch][n][n] of clustered 16-d points.  'x1e4': the same distances times 1e4 (beta halves about
    13 times from 1, and exp(-beta d) without the shift underflows).  'x1e-4': times 1e-4, rows 1 and 2 duplicates of each
    other and the last row a far outlier (beta doubles)."""
    out = np.empty((batch, n, n), dtype=np.float32)
    for b in range(batch):
        X, _ = clustered(n, 16, 5, seed + 17 * b + n)
        if variant == "x1e-4":
            X[2] = X[1]
            X[n - 1] += 300.0
        D = sqdist(X) * {"plain": 1.0, "x1e4": 1e4, "x1e-4": 1e-4}[variant]
        D = D.astype(np.float32)
        # what a GEMM-made matrix looks like: not exactly zero on the diagonal, tiny negatives allowed
        D[np.arange(n), np.arange(n)] = (-1e-6 * (1 + np.arange(n) % 3)).astype(np.float32) * D.max()
        out[b] = D
    return out


def step_fixture(n, batch, spread, seed=3):
    """(P [batch][n][n] float64 joint matrices that are exactly fp32 values, Y0 [batch][n][2] fp32 of the given spread)"""
    rng = np.random.RandomState(seed + n)
    P = np.empty((batch, n, n))
    for b in range(batch):
        X, _ = clustered(n, 8, 4, seed + 5 * b + n)
        Pb, _ = affinities(sqdist(X).astype(np.float32), min(10.0, n / 4.0))
        Pb = Pb.astype(np.float32)
        P[b] = np.maximum(Pb, Pb.T)                # symmetric in fp32 as well
    Y = (spread * rng.randn(batch, n, 2)).astype(np.float32)
    return P, Y


def end_to_end_features(seed=0):
    """25 identities x 4 images, 2304-wide: the three 768-wide slices are separate clusterings.  ([100][2304] fp32, ids)"""
    parts = []
    for m in range(3):
        X, label = clustered(100, 768, 25, seed + 101 * m)
        parts.append(X)
    return np.concatenate(parts, 1).astype(np.float32), label


def purity_1nn(Y, label):
    d = sqdist(Y)
    d[np.arange(len(Y)), np.arange(len(Y))] = np.inf
    return float((label[d.argmin(1)] == label).mean())


# ---- error bounds of the fp32 kernels, from the float64 terms ---------------------------------------------------------------
def sum_rtol(n):
    """(n + 16) 2^-24: above any fp32 summation order of n terms (n 2^-24 of the summed magnitudes) plus the roundings of
    one term -- two differences, d^2 (three), 1 + d^2, the division, two or three products: under 16"""
    return (n + 16) * U24


def gradient_error_bound(sums, mags, Z, alpha, n):
    """what |g - g_fp32| can reach when every per-row sum and Z are within sum_rtol(n) of their summed magnitudes: g = 4
    (alpha A - R / Z), so alpha dA + dR / Z + |R| dZ / Z^2, and three more roundings of the result's two terms.  [n][2]"""
    r = sum_rtol(n)
    dA, dR = r * mags[0:2].T, r * mags[2:4].T
    A, R = np.abs(sums[0:2].T), np.abs(sums[2:4].T)
    return 4.0 * (alpha * dA + dR / Z + R * r / Z + 3.0 * U24 * (alpha * A + R / Z))
