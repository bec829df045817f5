"""k-reciprocal re-ranking from descriptors: the re-ranked top-k of every query, or the re-ranked [Q, G] matrix, without
the Q x Q and G x G distance matrices (ieee_amd.rerank.rerank_search_topk / re_ranking_features).

    python scripts/rerank_gallery.py --synthetic 100000 --queries 1000 --k 10
    python scripts/rerank_gallery.py --features descriptors.pt --save reranked.pt

--features FILE: a torch.save'd dict with 'query' [Q, d] and 'gallery' [G, d] (and, optionally, q_pids, g_pids, q_camids,
g_camids: all four or none).  --synthetic N: N gallery descriptors of --dim columns around --ids identity centres and
--queries query descriptors of the same identities, with labels.
Without --save: prints the top-k of the first --show queries and, with labels, how many are of the query's identity.
With --save FILE: the re-ranked matrix goes to FILE (torch.save, on the host).  Either way the device memory peak."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--features", default=None, metavar="FILE", help="torch.save'd dict: query, gallery[, the four labels]")
    src.add_argument("--synthetic", type=int, default=None, metavar="N", help="gallery descriptors")
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--ids", type=int, default=500)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--k1", type=int, default=20)
    ap.add_argument("--k2", type=int, default=6)
    ap.add_argument("--lambda-value", type=float, default=0.3)
    ap.add_argument("--metric", default="euclidean", choices=("euclidean", "cosine"))
    ap.add_argument("--slab-rows", type=int, default=None, help="rows on either side of one distance GEMM")
    ap.add_argument("--save", default=None, metavar="FILE", help="save the re-ranked [Q, G] matrix instead of the top-k")
    ap.add_argument("--show", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch
    from ieee_amd.rerank import re_ranking_features, rerank_search_topk

    labels = {}
    if args.features:
        blob = torch.load(args.features, map_location="cpu")
        query, gallery = blob["query"], blob["gallery"]
        labels = {n: np.asarray(blob[n]) for n in ("q_pids", "g_pids", "q_camids", "g_camids") if n in blob}
    else:
        gen = torch.Generator().manual_seed(args.seed)
        rng = np.random.RandomState(args.seed)
        centres = torch.randn(args.ids, args.dim, generator=gen)
        labels = dict(q_pids=rng.randint(0, args.ids, args.queries), g_pids=rng.randint(0, args.ids, args.synthetic),
                      q_camids=rng.randint(0, 6, args.queries), g_camids=rng.randint(0, 6, args.synthetic))
        query = centres[labels["q_pids"]] + 0.5 * torch.randn(args.queries, args.dim, generator=gen)
        gallery = centres[labels["g_pids"]] + 0.5 * torch.randn(args.synthetic, args.dim, generator=gen)
    query, gallery = query.cuda(), gallery.cuda()
    Q, G = query.shape[0], gallery.shape[0]
    print("# query {} x {}, gallery {} x {}, k1 = {}, k2 = {}, lambda = {}, {}".format(
        Q, query.shape[1], G, gallery.shape[1], args.k1, args.k2, args.lambda_value, args.metric))
    common = dict(k1=args.k1, k2=args.k2, lambda_value=args.lambda_value, metric=args.metric, slab_rows=args.slab_rows)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    if args.save:
        out = re_ranking_features(query, gallery, **common)
    else:
        idx, dist = rerank_search_topk(query, gallery, args.k, **common, **labels)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    if args.save:
        torch.save(out.cpu(), args.save)
        print("saved the re-ranked {} x {} matrix to {}".format(Q, G, args.save))
    else:
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        for i in range(min(args.show, Q)):
            row = [(int(j), float(v)) for j, v in zip(idx[i], dist[i]) if j >= 0]
            if labels:
                same = sum(labels["g_pids"][j] == labels["q_pids"][i] for j, _ in row)
                print("query {} (id {}): {} of {} of its identity".format(i, labels["q_pids"][i], same, len(row)))
            else:
                print("query {}:".format(i))
            print("   " + "  ".join("{}:{:.4g}".format(j, v) for j, v in row))
    print("device memory peak above the descriptors handed in: {:.1f} MB (the G x G matrix alone would be {:.1f} MB)".format(
        peak / 1e6, G * G * 4 / 1e6))


if __name__ == "__main__":
    main()
