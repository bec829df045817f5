"""Gallery search from descriptors, piece by piece: the k nearest gallery entries of every query without the
[Q, G] distance matrix (ieee_amd.metrics.search_topk).

    python scripts/search_gallery.py --synthetic 200000 --k 10            # synthetic descriptors, gallery on the host
    python scripts/search_gallery.py --synthetic 20000 --weights model.pth.tar --crops 64

--synthetic N: N gallery descriptors of --dim columns around --ids identity centres, handed over in pieces of --piece
rows as a generator, so the whole gallery is never in one place on the device; --queries query descriptors of the same
identities.  With --weights the descriptors of the first pieces come from FeatureExtractor instead: --crops random
crops of random sizes per piece go through the model (its descriptors replace the first rows of the piece), which is
the shape of a retrieval service -- extractor output chunk by chunk into a running search.
Prints the top-k of the first --show queries, how many of them are of the query's identity, and the device memory peak.
--qe-k K [--qe-alpha A --qe-times T --qe-mode both|query]: query expansion (ieee_amd.expansion.expand_descriptors) and a
second search, so the result is printed before and after it.  The expansion walks the gallery more than once, so with
these flags the pieces are kept in a list on the host instead of being generated on the way."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", type=int, required=True, metavar="N", help="gallery descriptors")
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--ids", type=int, default=500)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--slab", type=int, default=None, help="gallery rows per slab (default: default_slab_rows(queries))")
    ap.add_argument("--piece", type=int, default=50000, help="gallery rows per piece")
    ap.add_argument("--metric", default="euclidean", choices=("euclidean", "cosine"))
    ap.add_argument("--precision", default=None)
    ap.add_argument("--weights", default=None, help="checkpoint of ieee3modalPart: extractor output joins the gallery")
    ap.add_argument("--crops", type=int, default=64, help="with --weights: crops per piece")
    ap.add_argument("--show", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--qe-k", type=int, default=None, help="query expansion over the K nearest neighbours (off when not given)")
    ap.add_argument("--qe-alpha", type=int, default=3)
    ap.add_argument("--qe-times", type=int, default=1)
    ap.add_argument("--qe-mode", default="both", choices=("both", "query"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from ieee_amd.metrics import default_slab_rows, search_topk

    gen = torch.Generator().manual_seed(args.seed)
    rng = np.random.RandomState(args.seed)
    dim = 2304 if args.weights else args.dim
    centres = torch.randn(args.ids, dim, generator=gen)
    q_pids = rng.randint(0, args.ids, args.queries)
    g_pids = rng.randint(0, args.ids, args.synthetic)
    q_camids, g_camids = rng.randint(0, 6, args.queries), rng.randint(0, 6, args.synthetic)
    query = (centres[q_pids] + 0.5 * torch.randn(args.queries, dim, generator=gen)).cuda()
    extractor = None
    if args.weights:
        from ieee_amd.feature_extractor import FeatureExtractor
        extractor = FeatureExtractor(model_path=args.weights, batch_size=args.crops)

    def pieces():
        for lo in range(0, args.synthetic, args.piece):
            n = min(args.piece, args.synthetic - lo)
            piece = centres[g_pids[lo:lo + n]] + 0.5 * torch.randn(n, dim, generator=gen)      # on the host
            if extractor is not None:
                m = min(args.crops, n)
                crops = [[rng.randint(0, 255, size=(rng.randint(40, 200), rng.randint(20, 100), 3)).astype(np.uint8)
                          for _ in range(m)] for _ in range(3)]
                piece = torch.cat([extractor(crops).float(), piece[m:].cuda()])                  # device rows join host rows
            yield piece

    slab = args.slab or default_slab_rows(args.queries)
    print("# query: {}\n# gallery {} in pieces of {}, slabs of {} rows".format(args.queries, args.synthetic, args.piece, slab))
    kept = list(pieces()) if args.qe_k is not None else None      # the expansion needs the gallery more than once

    def search(title, query, gallery):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        idx, dist = search_topk(query, gallery, args.k, metric=args.metric, q_pids=q_pids, g_pids=g_pids, q_camids=q_camids,
                                g_camids=g_camids, slab=args.slab, precision=args.precision)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        if title:
            print(title)
        for i in range(min(args.show, args.queries)):
            row = [(int(j), float(v)) for j, v in zip(idx[i], dist[i]) if j >= 0]
            same = sum(g_pids[j] == q_pids[i] for j, _ in row)
            print("query {} (id {}): {} of {} of its identity".format(i, q_pids[i], same, len(row)))
            print("   " + "  ".join("{}:{:.4g}".format(j, v) for j, v in row))
        print("device memory peak above the query: {:.1f} MB (the whole matrix would be {:.1f} MB)".format(
            peak / 1e6, args.queries * args.synthetic * 4 / 1e6))

    search(None, query, pieces() if kept is None else kept)
    if kept is not None:
        from ieee_amd.expansion import expand_descriptors
        qe = dict(k=args.qe_k, alpha=args.qe_alpha, times=args.qe_times, mode=args.qe_mode)
        if args.qe_mode == "query" and args.metric != "cosine":
            print("note: mode 'query' returns unit-length queries and the gallery as it is; unless the gallery is "
                  "normalised too, rank with --metric cosine")
        query2, gallery2 = expand_descriptors(
            query, torch.cat([p.cuda() for p in kept]) if args.qe_mode == "both" else kept, precision=args.precision, **qe)
        search("# after query expansion (k={k}, alpha={alpha}, times={times}, mode={mode})".format(**qe), query2, gallery2)


if __name__ == "__main__":
    main()
