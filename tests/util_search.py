"""What the streamed gallery search must return, restated in numpy on the whole matrix: drop the same-identity
same-camera entries, stable argsort (so -0.0 == +0.0, NaN last, ties to the lower index), first k, -1 / +inf padding.
Written for tests/test_search_*.py on its own; nothing here touches the device."""
import numpy as np


def ref_topk(d, k, labels=None):
    """d [Q, G] float32 -> (idx int64 [Q, k], dist float32 [Q, k]); labels = (q_pids, g_pids, q_camids, g_camids)"""
    d = np.asarray(d, dtype=np.float32)
    Q, G = d.shape
    idx = np.full((Q, k), -1, dtype=np.int64)
    dist = np.full((Q, k), np.inf, dtype=np.float32)
    for q in range(Q):
        cols = np.arange(G)
        if labels is not None:
            qp, gp, qc, gc = labels
            cols = cols[(gp != qp[q]) | (gc != qc[q])]
        best = cols[np.argsort(d[q, cols], kind="stable")[:k]]
        idx[q, :best.size] = best
        dist[q, :best.size] = d[q, best]
    return idx, dist


def make_labels(rng, Q, G, ids=20, cams=4):
    """(q_pids, g_pids, q_camids, g_camids), int64"""
    return rng.randint(0, ids, Q), rng.randint(0, ids, G), rng.randint(0, cams, Q), rng.randint(0, cams, G)


def cuts(G, parts):
    """parts: a list of slab widths that sum to G, or one int = slabs of that width -> [(lo, hi), ...]"""
    if isinstance(parts, int):
        return [(lo, min(lo + parts, G)) for lo in range(0, G, parts)]
    assert sum(parts) == G, (parts, G)
    edges = np.concatenate([[0], np.cumsum(parts)])
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def assert_same(got_idx, got_dist, ref_idx, ref_dist):
    """indices equal, distances equal as uint32 bits (got: device tensors)"""
    gi, gd = got_idx.cpu().numpy(), got_dist.cpu().numpy()
    assert gi.dtype == np.int64 and gd.dtype == np.float32 and gi.shape == ref_idx.shape and gd.shape == ref_dist.shape
    np.testing.assert_array_equal(gi, ref_idx)
    np.testing.assert_array_equal(gd.view(np.uint32), ref_dist.view(np.uint32))


def int_distances(q, g):
    """exact squared euclidean distances of integer-valued descriptors, via int64 -> float32 [Q, G]"""
    q, g = q.astype(np.int64), g.astype(np.int64)
    d = (q * q).sum(1)[:, None] + (g * g).sum(1)[None, :] - 2 * (q @ g.T)
    return d.astype(np.float32)
