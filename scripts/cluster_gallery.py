"""DBSCAN over descriptors on the device, without the N x N distance matrix (ieee_amd.cluster.dbscan): pseudo-labels
for an unlabelled gallery, de-duplication, crops into tracklets.

    python scripts/cluster_gallery.py --synthetic 100000 --dim 768 --metric cosine --eps 0.35
    python scripts/cluster_gallery.py --features descriptors.pt --metric cosine --eps 0.3 --save labels.pt

--features FILE: a torch.save'd tensor [N, d], or a dict with 'features', or with 'gallery' (and 'query': the rows of
both are clustered together, queries first).  --synthetic N: N descriptors of --dim columns around --ids identity
centres.  --eps is in the units of compute_distance_matrix: SQUARED for --metric euclidean.  Without --eps the
--degree-th smallest distance of --sample random rows is taken, so that a row has about --degree neighbours.
Prints clusters, noise count, the largest cluster sizes and the device memory peak; --save FILE keeps the labels."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def eps_for_degree(X, metric, degree, sample, seed, precision=None):
    """the eps at which a row of X has about `degree` neighbours: the median over `sample` random rows of their
    degree-th smallest distance to the other rows (search_topk: no N x N matrix)"""
    import torch
    from ieee_amd.metrics import search_topk
    gen = torch.Generator().manual_seed(seed)
    pick = torch.randperm(X.shape[0], generator=gen)[:sample].to(X.device)
    k = min(int(degree) + 1, X.shape[0], 1024)                    # the row itself is its own nearest neighbour
    _, dist = search_topk(X[pick], X, k, metric=metric, precision=precision)
    return float(dist[:, -1].median())


def main():
    ap = argparse.ArgumentParser()
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--features", default=None, metavar="FILE", help="torch.save'd [N, d] tensor or dict (see above)")
    src.add_argument("--synthetic", type=int, default=None, metavar="N", help="descriptors")
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--ids", type=int, default=500)
    ap.add_argument("--eps", type=float, default=None)
    ap.add_argument("--degree", type=float, default=20, help="without --eps: the mean number of neighbours aimed at")
    ap.add_argument("--sample", type=int, default=512)
    ap.add_argument("--min-samples", type=int, default=4)
    ap.add_argument("--metric", default="cosine", choices=("euclidean", "cosine"))
    ap.add_argument("--precision", default=None)
    ap.add_argument("--block", type=int, default=None)
    ap.add_argument("--slab", type=int, default=None)
    ap.add_argument("--max-edges", type=int, default=None)
    ap.add_argument("--save", default=None, metavar="FILE", help="torch.save the labels (int64 [N], on the host)")
    ap.add_argument("--show", type=int, default=10, help="how many of the largest clusters to list")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch
    from ieee_amd.cluster import dbscan, dbscan_layout

    if args.features:
        blob = torch.load(args.features, map_location="cpu")
        if isinstance(blob, dict):
            if not any(n in blob for n in ("features", "query", "gallery")):
                raise SystemExit("{}: a dict needs 'features', or 'query' and / or 'gallery'; it has {}".format(
                    args.features, sorted(blob)))
            blob = blob["features"] if "features" in blob else \
                torch.cat([blob[n] for n in ("query", "gallery") if n in blob])
        X = blob.float()
    else:
        gen = torch.Generator().manual_seed(args.seed)
        centres = torch.randn(args.ids, args.dim, generator=gen)
        pick = torch.randint(0, args.ids, (args.synthetic,), generator=gen)
        X = centres[pick] + 0.5 * torch.randn(args.synthetic, args.dim, generator=gen)
    X = X.cuda()
    N, d = X.shape
    eps = args.eps
    if eps is None:
        eps = eps_for_degree(X, args.metric, args.degree, args.sample, args.seed, args.precision)
    print("# {} x {}, {}, eps = {:.6g}, min_samples = {}".format(N, d, args.metric, eps, args.min_samples))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    labels, info = dbscan(X, eps, args.min_samples, metric=args.metric, block=args.block, slab=args.slab,
                          precision=args.precision, max_edges=args.max_edges, return_info=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    sizes = torch.bincount(labels[labels >= 0], minlength=max(info["clusters"], 1)).sort(descending=True).values
    print("clusters {}, noise {}, core points {}".format(info["clusters"], int((labels < 0).sum()), int(info["core"].sum())))
    print("largest clusters: " + " ".join(str(int(s)) for s in sizes[:args.show] if s > 0))
    print("neighbour pairs {} (mean degree {:.1f}), mirrored {}, rounds {}".format(
        info["edges"], info["edges"] / float(max(N, 1)), info["mirrored_edges"], info["rounds"]))
    print("device memory peak above the descriptors: {:.1f} MB (layout {:.1f} MB; the whole matrix would be {:.1f} MB)".format(
        peak / 1e6, dbscan_layout(N, d, info["edges"], args.block, args.slab, args.metric)["total"] / 1e6, N * N * 4 / 1e6))
    if args.save:
        torch.save(labels.cpu(), args.save)
        print("saved the labels to {}".format(args.save))


if __name__ == "__main__":
    main()
