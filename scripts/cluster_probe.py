"""Times DBSCAN (ieee_amd.cluster.dbscan) on one MI355X against the two distance sweeps it contains, run alone: the same
SlabDistances GEMMs, block by slab, twice, with no thresholding.  Device events around every call, the two candidates
interleaved round by round, medians over the rounds; peak memory of each; the round count of the component search.

    python scripts/cluster_probe.py                         # 19732 x 2304 and 100000 x 768, cosine, mean degree ~ 20
    python scripts/cluster_probe.py --sizes 19732,2304 --rounds 7 --out probe.json

eps is chosen per size so that a row has about --degree neighbours (scripts/cluster_gallery.py: eps_for_degree).
One JSON line per size.  No time or ratio here is a gate."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="19732,2304;100000,768", help="N,d;N,d;...")
    ap.add_argument("--metric", default="cosine", choices=("euclidean", "cosine"))
    ap.add_argument("--degree", type=float, default=20)
    ap.add_argument("--min-samples", type=int, default=4)
    ap.add_argument("--ids", type=int, default=1500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block", type=int, default=None)
    ap.add_argument("--slab", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from cluster_gallery import eps_for_degree
    from ieee_amd import _lib
    from ieee_amd import cluster as C
    from ieee_amd.metrics import distance as _dist
    from ieee_amd.metrics._stream import check_metric
    lib = _lib.require_gpu()

    def timed(fn):
        """-> (milliseconds by device events, peak bytes above what was allocated before, what fn returned)"""
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), torch.cuda.max_memory_allocated() - before, out

    lines = []
    for size in args.sizes.split(";"):
        N, d = (int(v) for v in size.split(","))
        gen = torch.Generator().manual_seed(0)
        centres = torch.randn(args.ids, d, generator=gen)
        pick = torch.randint(0, args.ids, (N,), generator=gen)
        X = (centres[pick] + 0.5 * torch.randn(N, d, generator=gen)).cuda()
        eps = eps_for_degree(X, args.metric, args.degree, 512, 0)
        block, slab = C._blocking(N, args.block, args.slab, "cluster_probe")
        metric_id = check_metric(args.metric)
        precision, cdt = _dist._resolve(None, X.dtype)

        def sweeps():
            Xp = _dist._pad8(X.to(cdt).contiguous())
            for _ in range(2):
                C._sweep_descriptors(lib, Xp, metric_id, cdt, precision, block, slab, lambda *a: None)

        def whole():
            return C.dbscan(X, eps, args.min_samples, metric=args.metric, block=args.block, slab=args.slab, return_info=True)

        forms = {"dbscan": whole, "two_sweeps": sweeps}
        for fn in forms.values():
            fn()                                                 # warm-up
        ms = {name: [] for name in forms}
        peak = {name: 0 for name in forms}
        info = None
        for _ in range(args.rounds):
            for name, fn in forms.items():                       # interleaved
                t, p, out = timed(fn)
                ms[name].append(t)
                peak[name] = max(peak[name], p)
                if name == "dbscan":
                    labels, info = out
                del out
        med = {n: statistics.median(v) for n, v in ms.items()}
        line = {"N": N, "d": d, "metric": args.metric, "eps": eps, "min_samples": args.min_samples, "block": block,
                "slab": slab, "rounds_measured": args.rounds,
                "ms_median": {n: round(v, 2) for n, v in med.items()},
                "ms_min_max": {n: [round(min(v), 2), round(max(v), 2)] for n, v in ms.items()},
                "share_outside_the_sweeps": round(1.0 - med["two_sweeps"] / med["dbscan"], 3),
                "sweep_TFLOPs": round(2 * 2.0 * N * N * d / med["two_sweeps"] / 1e9, 1),
                "peak_MB": {n: round(p / 1e6, 1) for n, p in peak.items()},
                "layout_MB": round(C.dbscan_layout(N, d, info["edges"], args.block, args.slab, args.metric)["total"] / 1e6, 1),
                "dense_matrix_MB": round(4.0 * N * N / 1e6, 1),
                "edges": info["edges"], "mean_degree": round(info["edges"] / float(N), 2),
                "mirrored_edges": info["mirrored_edges"], "cc_rounds": info["rounds"], "clusters": info["clusters"],
                "noise": int((labels < 0).sum())}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del X, labels, info
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
