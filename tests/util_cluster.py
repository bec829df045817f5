"""DBSCAN as ieee_amd.cluster defines it, restated in numpy on a dense matrix: the oracle of the cluster
tests.  Every quantity is an integer or a boolean, so the device must give these values exactly.

    thr = float32(eps);  R(i, j) iff i == j or D[i, j] <= thr or D[j, i] <= thr   (fp32 compares, NaN never)
    core(i) iff |{j : R(i, j)}| >= min_samples                                    (i itself is counted)
    clusters: the connected components of R on the core points, numbered by ascending smallest core index
    a non-core point takes the smallest cluster number among its core neighbours, or -1

dbscan_ref has three switches that each break one clause; check_definition is an independent statement of the clauses
and must reject all three.  cc_rounds restates the hook-and-shortcut rounds of ieee_cluster_cc_round."""
import numpy as np


def relation(D, eps, closure="or"):
    """-> R, bool [N, N]"""
    D = np.asarray(D, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        H = D <= np.float32(eps)
    R = (H | H.T) if closure == "or" else (H & H.T)
    np.fill_diagonal(R, True)
    return R


def components(R, core):
    """-> comp int64 [N]: the smallest core index of the component of every core point (depth first), -1 elsewhere"""
    N = R.shape[0]
    comp = np.full(N, -1, dtype=np.int64)
    for s in range(N):
        if not core[s] or comp[s] >= 0:
            continue
        comp[s] = s
        stack = [s]
        while stack:
            u = stack.pop()
            nb = np.nonzero(R[u] & core & (comp < 0))[0]
            comp[nb] = s
            stack.extend(nb.tolist())
    return comp


def dbscan_ref(D, eps, min_samples, self_counts=True, closure="or", border="min"):
    """-> (labels int64 [N], core bool [N], clusters).  The defaults are the definition; self_counts=False, closure='and'
    and border='max' are the deliberately wrong references of the tests."""
    R = relation(D, eps, closure)
    N = R.shape[0]
    core = R.sum(axis=1) - (0 if self_counts else 1) >= min_samples
    comp = components(R, core)
    roots = np.nonzero(core & (comp == np.arange(N)))[0]           # ascending: the numbering
    number = np.full(N, -1, dtype=np.int64)
    number[roots] = np.arange(roots.size)
    labels = np.full(N, -1, dtype=np.int64)
    labels[core] = number[comp[core]]
    for i in np.nonzero(~core)[0]:
        nb = np.nonzero(R[i] & core)[0]
        if nb.size:
            labels[i] = labels[nb].min() if border == "min" else labels[nb].max()
    return labels, core, int(roots.size)


def check_definition(D, eps, min_samples, labels, core):
    """-> the list of clauses (labels, core) break on D; empty when they are DBSCAN's.  Written without dbscan_ref's
    machinery: reachability by frontier expansion inside one label at a time."""
    R = relation(D, eps)
    labels, core = np.asarray(labels), np.asarray(core, dtype=bool)
    N = R.shape[0]
    bad = []
    if not np.array_equal(core, R.sum(axis=1) >= min_samples):
        bad.append("core flags are not |neighbours, self included| >= min_samples")
        return bad
    if (labels[core] < 0).any():
        bad.append("a core point is noise")
        return bad
    ids = np.unique(labels[core])
    if not np.array_equal(ids, np.arange(ids.size)) or (labels > (ids.size - 1)).any():
        bad.append("cluster numbers are not 0 .. clusters - 1, each with a core point")
        return bad
    firsts = [int(np.nonzero(core & (labels == c))[0][0]) for c in ids]
    if firsts != sorted(firsts):
        bad.append("clusters are not numbered by ascending smallest core index")
    for c in ids:
        members = core & (labels == c)
        seen = np.zeros(N, dtype=bool)
        seen[np.nonzero(members)[0][0]] = True
        while True:
            grown = (R[seen].any(axis=0) & members) | seen
            if (grown == seen).all():
                break
            seen = grown
        if not (seen == members).all():
            bad.append("the core points of cluster %d are not R-connected" % c)
    ci = np.nonzero(core)[0]
    sub = R[np.ix_(ci, ci)]
    if (sub & (labels[ci][:, None] != labels[ci][None, :])).any():
        bad.append("an R edge joins core points of two clusters")
    for i in np.nonzero(~core)[0]:
        nb = labels[np.nonzero(R[i] & core)[0]]
        if labels[i] < 0 and nb.size:
            bad.append("noise point %d has a core neighbour" % i)
        if labels[i] >= 0 and (nb.size == 0 or labels[i] not in nb):
            bad.append("border point %d has no core neighbour of its cluster" % i)
        elif labels[i] >= 0 and nb.min() < labels[i]:
            bad.append("border point %d has a core neighbour of a smaller cluster" % i)
    return bad


def core_edges(R, core):
    """-> (u, v): the directed R edges between distinct core points, both directions present"""
    u, v = np.nonzero(R & core[:, None] & core[None, :])
    keep = u != v
    return u[keep], v[keep]


def cc_rounds(N, u, v, max_rounds=None):
    """The rounds of ieee_cluster_cc_round on the directed edges (u[k], v[k]) (both directions given): every round reads
    the previous parent array f only -- g = f[f[v]] lowers next[f[u]] and next[u], f[f[u]] lowers next[u] -- and the
    rounds end with the first that changes nothing.  -> (f, rounds), that last round counted."""
    f = np.arange(N, dtype=np.int64)
    rounds = 0
    while True:
        g = f[f]
        nxt = np.minimum(f, g)                     # the shortcut
        gv = g[v]
        np.minimum.at(nxt, f[u], gv)               # hook on the parent
        np.minimum.at(nxt, u, gv)                  # hook on the vertex
        rounds += 1
        if np.array_equal(nxt, f):
            return f, rounds
        f = nxt
        if max_rounds is not None and rounds >= max_rounds:
            raise AssertionError("no fixed point after %d rounds" % rounds)


def min_neighbour_rounds(N, u, v):
    """the plain iteration the kernels must NOT be: f[u] = min(f[u], min over neighbours f[v]) -> rounds, as above"""
    f = np.arange(N, dtype=np.int64)
    rounds = 0
    while True:
        nxt = f.copy()
        np.minimum.at(nxt, u, f[v])
        rounds += 1
        if np.array_equal(nxt, f):
            return rounds
        f = nxt


def permuted_chain(N, seed=0):
    """N points on a line at unit spacing under a seeded permutation -> pos int64 [N]"""
    return np.random.RandomState(seed).permutation(N).astype(np.int64)


def chain_edges(pos, min_samples=3):
    """the core edges of the chain at eps = 1 without the dense matrix: neighbours are the points one step away"""
    N = pos.size
    at = np.empty(N, dtype=np.int64)
    at[pos] = np.arange(N)                          # at[p]: the point at position p
    deg = np.full(N, 3, dtype=np.int64)
    deg[at[0]] = deg[at[N - 1]] = 2 if N > 1 else 1
    core = deg >= min_samples
    a, b = at[:-1], at[1:]
    keep = core[a] & core[b]
    a, b = a[keep], b[keep]
    return np.concatenate([a, b]), np.concatenate([b, a]), core


def emulate_kernels(D, eps, min_samples):
    """The data flow of ieee_amd/csrc/cluster.hip on the host, structure by structure, without the dense relation: the
    sorted directed lists A (eps count / fill), the mirrored lists X (a binary search for i in list j per edge i -> j),
    the core test on 1 + |A| + |X|, the rounds over both lists (only the previous round's parents are read), the roots'
    exclusive sum and the labels (a border point: the minimum over the core entries of both lists).
    -> (labels, core, clusters, mirrored, rounds)"""
    D = np.asarray(D, dtype=np.float32)
    N = D.shape[0]
    with np.errstate(invalid="ignore"):
        H = D <= np.float32(eps)
    np.fill_diagonal(H, False)                     # the self column is skipped whatever it holds
    A = [np.nonzero(H[i])[0] for i in range(N)]
    X = [[] for _ in range(N)]
    for i in range(N):
        for j in A[i]:
            p = int(np.searchsorted(A[j], i))
            if not (p < A[j].size and A[j][p] == i):
                X[j].append(i)
    both = [list(A[u]) + X[u] for u in range(N)]
    core = np.array([1 + len(both[u]) >= min_samples for u in range(N)], dtype=bool)
    f = np.arange(N, dtype=np.int64)
    rounds = 0
    while True:
        nxt = f.copy()
        for u in np.nonzero(core)[0]:
            best = f[f[u]]
            for v in both[u]:
                if core[v]:
                    best = min(best, f[f[v]])
            if best < f[u]:
                nxt[f[u]] = min(nxt[f[u]], best)
                nxt[u] = min(nxt[u], best)
        rounds += 1
        if np.array_equal(nxt, f):
            break
        f = nxt
    number = np.concatenate([[0], np.cumsum(core & (f == np.arange(N)))])
    labels = np.full(N, -1, dtype=np.int64)
    for u in range(N):
        if core[u]:
            labels[u] = number[f[u]]
        else:
            seen = [number[f[v]] for v in both[u] if core[v]]
            if seen:
                labels[u] = min(seen)
    return labels, core, int(number[N]), sum(len(x) for x in X), rounds
