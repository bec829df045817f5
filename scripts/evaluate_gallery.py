"""CMC / mAP from descriptors without the [Q, G] distance matrix (ieee_amd.metrics.evaluate_rank_streamed).

    python scripts/evaluate_gallery.py --synthetic 2000,50000,256 --compare
    python scripts/evaluate_gallery.py --synthetic 10000,1000000 --slab 16384 --distractors 0.9

--synthetic Q,G[,d]: Q query and G gallery descriptors of d columns (2304 by default) around --ids identity centres,
--cams cameras; --distractors: the share of gallery rows whose identity no query has.  The gallery stays on the host in
pieces of --piece rows, so only one slab of it is on the device at a time.  Prints mAP and the CMC curve at --ranks, the
device memory peak, and with --compare the same from compute_distance_matrix + evaluate_rank and whether the two are
equal.  --qe-k K [--qe-alpha A --qe-times T --qe-mode both|query]: query expansion (ieee_amd.expansion.expand_descriptors)
before a second evaluation, so the result is printed before and after it; mode 'both' holds the whole gallery on the
device, mode 'query' leaves it in its host pieces."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", required=True, metavar="Q,G[,d]")
    ap.add_argument("--ids", type=int, default=500)
    ap.add_argument("--cams", type=int, default=6)
    ap.add_argument("--distractors", type=float, default=0.0)
    ap.add_argument("--slab", type=int, default=None, help="gallery rows per slab (default: default_slab_rows(Q))")
    ap.add_argument("--piece", type=int, default=50000, help="gallery rows per piece")
    ap.add_argument("--metric", default="euclidean", choices=("euclidean", "cosine"))
    ap.add_argument("--precision", default=None)
    ap.add_argument("--max-rank", type=int, default=20)
    ap.add_argument("--ranks", default="1,5,10,20")
    ap.add_argument("--compare", action="store_true", help="also the two-step path on the whole matrix")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--qe-k", type=int, default=None, help="query expansion over the K nearest neighbours (off when not given)")
    ap.add_argument("--qe-alpha", type=int, default=3)
    ap.add_argument("--qe-times", type=int, default=1)
    ap.add_argument("--qe-mode", default="both", choices=("both", "query"))
    args = ap.parse_args()
    shape = [int(v) for v in args.synthetic.split(",")]
    if len(shape) not in (2, 3) or min(shape) < 1:
        ap.error("--synthetic takes Q,G or Q,G,d")
    Q, G, dim = shape[0], shape[1], (shape[2] if len(shape) == 3 else 2304)

    import numpy as np
    import torch
    from ieee_amd.metrics import compute_distance_matrix, default_slab_rows, evaluate_rank, evaluate_rank_streamed

    gen = torch.Generator().manual_seed(args.seed)
    rng = np.random.RandomState(args.seed)
    centres = torch.randn(2 * args.ids, dim, generator=gen)          # the upper half: identities no query has
    q_pids = rng.randint(0, args.ids, Q)
    g_pids = rng.randint(0, args.ids, G)
    stray = rng.rand(G) < args.distractors
    g_pids[stray] += args.ids
    q_camids, g_camids = rng.randint(0, args.cams, Q), rng.randint(0, args.cams, G)
    query = (centres[q_pids] + 0.5 * torch.randn(Q, dim, generator=gen)).cuda()
    pieces = [centres[g_pids[lo:lo + args.piece]] + 0.5 * torch.randn(min(args.piece, G - lo), dim, generator=gen)
              for lo in range(0, G, args.piece)]                     # on the host
    ranks = [int(r) for r in args.ranks.split(",") if int(r) <= min(args.max_rank, G)]

    def show(name, cmc, m_ap, peak):
        print("{}: mAP {:.4%}  ".format(name, m_ap) + "  ".join("Rank-{} {:.2%}".format(r, cmc[r - 1]) for r in ranks))
        print("   device memory peak above the query: {:.1f} MB (the whole matrix: {:.1f} MB)".format(
            peak / 1e6, Q * G * 4 / 1e6))

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - before

    print("# query: {}\n# gallery {} in pieces of {}, slabs of {} rows, {:.0%} distractors".format(
        Q, G, args.piece, args.slab or default_slab_rows(Q), args.distractors))
    (cmc, m_ap), peak = peak_of(lambda: evaluate_rank_streamed(
        query, pieces, q_pids, g_pids, q_camids, g_camids, max_rank=args.max_rank, metric=args.metric, slab=args.slab,
        precision=args.precision))
    show("streamed", cmc, m_ap, peak)
    if args.qe_k is not None:
        from ieee_amd.expansion import expand_descriptors
        qe = dict(k=args.qe_k, alpha=args.qe_alpha, times=args.qe_times, mode=args.qe_mode)
        (query2, gallery2), peak_qe = peak_of(lambda: expand_descriptors(
            query, torch.cat(pieces) if args.qe_mode == "both" else pieces, precision=args.precision, **qe))
        print("query expansion: device memory peak {:.1f} MB".format(peak_qe / 1e6))
        if args.qe_mode == "query" and args.metric != "cosine":
            print("note: mode 'query' returns unit-length queries and the gallery as it is; unless the gallery is "
                  "normalised too, rank with --metric cosine")
        (cmc_qe, m_ap_qe), peak = peak_of(lambda: evaluate_rank_streamed(
            query2, gallery2, q_pids, g_pids, q_camids, g_camids, max_rank=args.max_rank, metric=args.metric,
            slab=args.slab, precision=args.precision))
        show("streamed after query expansion (k={k}, alpha={alpha}, times={times}, mode={mode})".format(**qe), cmc_qe,
             m_ap_qe, peak)
    if args.compare:
        (cmc2, m_ap2), peak2 = peak_of(lambda: evaluate_rank(
            compute_distance_matrix(query, torch.cat(pieces).cuda(), args.metric, args.precision), q_pids, g_pids, q_camids,
            g_camids, max_rank=args.max_rank))
        show("two-step", cmc2, m_ap2, peak2)
        same = bool(np.array_equal(cmc, cmc2) and m_ap == m_ap2)
        print("results equal: {}".format(same))
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
