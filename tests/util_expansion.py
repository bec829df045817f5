"""Query expansion (ieee_amd/expansion.py) restated in float64, with the error bounds of the fp32 kernels.

restate_round     one round GIVEN the lists and the weights: the value and, per element, sum_j |w r x| for the bounds
dense_expand      the whole definition, lists included, by dense O(N^2) float64 matrices -- written independently of
                  restate_round (a weight matrix times the normalised rows, no gather)
weights_fp32      the weight chain as the kernel forms it, emulated in fp32 numpy
chain_fp32        the sum kernel's arithmetic emulated on the host (fma through float64, one rounding per term)

The bounds are derived, not tuned.  u = 2^-24 is the unit roundoff of fp32.

rinv.  ieee_row_rinv is the cosine distance's norm pass: a lane adds the squares of its 4 ceil(d/256) columns in a
chain (each product and each addition rounds once: relative error at most (L + 1) u of the sum of squares, L the chain
length), six shuffle additions follow (+ 6 u), then sqrtf (halves the relative error so far, adds at most 2 u) and the
division (at most 2 u).  r^ = r (1 + e), |e| <= c_r(d) u with c_r(d) = (4 ceil(d/256) + 7) / 2 + 4 <= 2 ceil(d/256) + 8.

Before normalisation.  A coefficient is fl(w r^) = w r (1 + t), |t| <= (c_r + 1) u.  The chain is one rounding per
term: the self product, then one fma per entry, so at most k + 1 roundings touch a term; recursive summation gives
|y^ - y| <= (k + 1) u sum|terms| on top of the coefficients' (c_r + 1) u.  With one more unit for everything of second
order ((1 + u)^n - 1 <= n u (1 + n u), n = k + c_r + 3 < 4096):
        B_c = (k + c_r(d) + 4) u  sum_j |w_j r_j x_jc|         (the self term is part of the sum).

After normalisation.  out = fl(y^ r^y), r^y = fl(1 / fl32(sqrt(ss))) with ss the float64 sum of y^'s squares (its own
error, d 2^-53, is below the slack): r^y = (1 + p) / |y^|, |p| <= 3 u, and the product rounds once more (4 u in all).
With D = y^ - y, |D_c| <= B_c, and n = |y|, n^ = |y^| >= n - |B|:
        |y^_c / n^ - y_c / n| <= |D_c| / n^ + |y_c| |n - n^| / (n n^) <= (B_c + (|y_c| / n) |B|) / (n - |B|)
        bound_c = (B_c + (|y_c| / n) |B|_2) / (n - |B|_2) + 4 u |y_c| / n (1 + 4 u)
which is the bound before normalisation divided by |y| plus the propagated error of r(y).  A zero y is a zero row on
both sides (bound 0).  The fixtures keep |y| far above the clamp 1e-12 (asserted)."""
import numpy as np

U32 = 2.0 ** -24
EPS = 1e-12


def c_r(d):
    return 2 * ((d + 255) // 256) + 8


def rinv64(x):
    """1 / max(|row|, 1e-12) in float64"""
    x = np.asarray(x, np.float64)
    return 1.0 / np.maximum(np.sqrt((x * x).sum(1)), EPS)


def make_fixture(Q, G, d, seed=0):
    """the issue's fixture: identities randint(0, max(2, N // 6)), rows centre[id] + 0.5 randn, fp32"""
    rng = np.random.RandomState(seed)
    N = Q + G
    ids = rng.randint(0, max(2, N // 6), N)
    centres = rng.randn(max(2, N // 6), d)
    X = (centres[ids] + 0.5 * rng.randn(N, d)).astype(np.float32)
    return X[:Q].copy(), X[Q:].copy()


FIXTURES = ((3, 7, 8), (17, 300, 64), (5, 2100, 24))


def weights_fp32(idx, dist, alpha):
    """max(1 - dist, 0)^alpha by alpha - 1 fp32 multiplications left to right; 1 for alpha 0; 0 where idx < 0"""
    idx, dist = np.asarray(idx), np.asarray(dist, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.fmax(np.float32(1) - dist, np.float32(0)).astype(np.float32)      # fmax: a NaN gives the other operand
        w = np.ones_like(s) if alpha == 0 else s.copy()
        for _ in range(alpha - 1):
            w = (w * s).astype(np.float32)
    return np.where(idx < 0, np.float32(0), w).astype(np.float32)


def restate_round(src, idx, w, use_rinv=True, self_rows=None, self_scaled=True, normalize=True):
    """One round given the lists, in float64.  src [n_src, d], idx / w [n, k] (any index outside [0, n_src) adds
    nothing), self_rows [n, d] or None.  -> (value, mag, bound): mag = sum_j |w r x| per element (with the self term),
    bound = the derived bound of the fp32 kernels for this output."""
    src = np.asarray(src, np.float64)
    idx, w = np.asarray(idx, np.int64), np.asarray(w, np.float64)
    n, k = idx.shape
    d = src.shape[1]
    r = rinv64(src) if use_rinv else np.ones(src.shape[0])
    y, mag = np.zeros((n, d)), np.zeros((n, d))
    if self_rows is not None:
        s = np.asarray(self_rows, np.float64)
        s = s * (rinv64(s)[:, None] if self_scaled else 1.0)
        y, mag = y + s, mag + np.abs(s)
    for j in range(k if src.shape[0] else 0):
        ok = (idx[:, j] >= 0) & (idx[:, j] < src.shape[0])
        g = np.where(ok, idx[:, j], 0)
        term = np.where(ok[:, None], np.where(ok, w[:, j] * r[g], 0.0)[:, None] * src[g], 0.0)
        y += term
        mag += np.abs(term)
    B = (k + c_r(d) + 4) * U32 * mag
    if not normalize:
        return y, mag, B
    nrm = np.sqrt((y * y).sum(1))
    Bn = np.sqrt((B * B).sum(1))
    live = nrm > 0
    assert np.all(nrm[live] > 1e-6) and np.all(Bn[live] < 0.5 * nrm[live]), "fixture too close to the clamp"
    safe = np.where(live, nrm, 1.0)
    out = y / safe[:, None]
    bound = (B + np.abs(out) * Bn[:, None]) / (safe - Bn)[:, None] + 4 * U32 * np.abs(out) * (1 + 4 * U32)
    return np.where(live[:, None], out, 0.0), mag, np.where(live[:, None], bound, 0.0)


def dense_lists(rows, cand, k):
    """float64 cosine distances of rows to cand, dense; the k nearest of each row ascending in (distance, index),
    padded with -1 / +inf -> (idx int64 [n, k], dist float64 [n, k])"""
    a = np.asarray(rows, np.float64) * rinv64(rows)[:, None]
    b = np.asarray(cand, np.float64) * rinv64(cand)[:, None]
    dist = 1.0 - a @ b.T
    n, m = dist.shape
    order = np.argsort(dist, axis=1, kind="stable")[:, :k]
    idx = np.full((n, k), -1, np.int64)
    out = np.full((n, k), np.inf)
    idx[:, :min(k, m)] = order
    out[:, :min(k, m)] = np.take_along_axis(dist, order, 1)
    return idx, out


def dense_expand(q, g, k, alpha, times=1, mode="both"):
    """the whole definition by dense float64 matrices: Y = W Xn with W [rows, candidates] the list weights"""
    q, g = np.asarray(q, np.float64), np.asarray(g, np.float64)
    Q = q.shape[0]
    for _ in range(times):
        rows = np.concatenate([q, g]) if mode == "both" else q
        cand = rows if mode == "both" else g
        idx, dist = dense_lists(rows, cand, k)
        W = np.zeros((rows.shape[0], cand.shape[0]))
        for j in range(min(k, cand.shape[0])):
            s = np.maximum(1.0 - dist[:, j], 0.0)
            np.add.at(W, (np.arange(rows.shape[0]), idx[:, j]), np.ones_like(s) if alpha == 0 else s ** alpha)
        Y = W @ (cand * rinv64(cand)[:, None])
        if mode == "query":
            Y = Y + rows * rinv64(rows)[:, None]
        Y = Y * np.where((Y * Y).sum(1) > 0, rinv64(Y), 0.0)[:, None]
        q, g = (Y[:Q], Y[Q:]) if mode == "both" else (Y, g)
    return q, g


def fma32(a, b, c):
    """fl32(a b + c): the product of two fp32 values is exact in float64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def chain_fp32(src, idx, w, rinv=None, self_rows=None, self_rinv=None, normalize=True):
    """ieee_neighbour_sum's arithmetic on the host: fp32 coefficients, one fma per kept entry in list order, the squares
    summed in float64 (sequentially here; the kernel's tree differs in the last bits of a float64)"""
    src = np.asarray(src, np.float32)
    n, k = idx.shape
    out = np.zeros((n, src.shape[1]), np.float32)
    for i in range(n):
        if self_rows is not None:
            s = np.asarray(self_rows[i], np.float32)
            acc = (np.float32(self_rinv[i]) * s).astype(np.float32) if self_rinv is not None else s.copy()
        else:
            acc = np.zeros(src.shape[1], np.float32)
        for j in range(k):
            g = int(idx[i, j])
            if 0 <= g < src.shape[0]:
                c = np.float32(w[i, j]) * np.float32(rinv[g]) if rinv is not None else np.float32(w[i, j])
                acc = fma32(np.float32(c), src[g], acc)
        if normalize:
            nrm = np.float32(np.sqrt((acc.astype(np.float64) ** 2).sum()))
            acc = (acc * (np.float32(1) / np.maximum(nrm, np.float32(1e-12)))).astype(np.float32)
        out[i] = acc
    return out
