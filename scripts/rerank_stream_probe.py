"""Times k-reciprocal re-ranking from descriptors (ieee_amd.rerank.re_ranking_features, rerank_search_topk) against the
matrix path (three compute_distance_matrix calls + re_ranking(..., formulation='sparse')) on the same build, in the same
run: device events, medians of interleaved rounds, fp32, one device.

One size per process; run every invocation under its own `timeout`:

    timeout -k 10 300 python scripts/rerank_stream_probe.py --scale market
    timeout -k 10 900 python scripts/rerank_stream_probe.py --scale large --iters 3 --search

Prints one JSON line: per path the median / min / max time in ms and the peak device memory of one call above the
descriptors, whether the two results have the same bits, and with --search the same for rerank_search_topk(k=10).
--no-matrices leaves the matrix path out (a gallery whose matrices do not fit)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SCALES = {"small": (100, 900, 64), "market": (3368, 19732, 2304), "large": (10000, 100000, 2304)}


def features(Q, G, d, ids):
    import torch
    g = torch.Generator().manual_seed(1)
    centre = torch.randn(ids, d, generator=g)
    pid = torch.randint(0, ids, (Q + G,), generator=g)
    x = centre[pid] + 0.8 * torch.randn(Q + G, d, generator=g)
    return x[:Q].cuda(), x[Q:].cuda()


def once(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def interleaved(fns, warmup, iters, keep):
    """{name: fn} -> {name: stats}; keep(name, result) sees every result of the timed rounds before it is dropped"""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(iters):
        for name, fn in fns.items():
            ms, out = once(fn)
            times[name].append(ms)
            keep(name, out)
            del out
    return {name: {"median": sorted(t)[len(t) // 2], "min": min(t), "max": max(t)} for name, t in times.items()}


def peak_bytes(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", choices=sorted(SCALES), default="market")
    ap.add_argument("--k1", type=int, default=20)
    ap.add_argument("--k2", type=int, default=6)
    ap.add_argument("--metric", default="euclidean", choices=("euclidean", "cosine"))
    ap.add_argument("--slab-rows", type=int, default=None)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--search", action="store_true", help="also time rerank_search_topk(k=10)")
    ap.add_argument("--no-matrices", action="store_true")
    args = ap.parse_args()
    import torch
    from ieee_amd.metrics.distance import compute_distance_matrix as cd
    from ieee_amd.rerank import re_ranking, re_ranking_features, rerank_search_topk
    Q, G, d = SCALES[args.scale]
    xq, xg = features(Q, G, d, max(8, (Q + G) // 25))
    kw = dict(k1=args.k1, k2=args.k2, lambda_value=0.3)

    def matrices():
        return re_ranking(cd(xq, xg, args.metric), cd(xq, xq, args.metric), cd(xg, xg, args.metric), formulation="sparse", **kw)

    fns = {"descriptors": lambda: re_ranking_features(xq, xg, metric=args.metric, slab_rows=args.slab_rows, **kw)}
    if not args.no_matrices:
        fns["matrices"] = matrices
    if args.search:
        fns["search_topk"] = lambda: rerank_search_topk(xq, xg, 10, metric=args.metric, slab_rows=args.slab_rows, **kw)
    digest = {}

    def keep(name, out):
        if name != "search_topk":                   # a checksum of the bits, so that no [Q, G] result has to be kept
            digest[name] = int(out.view(torch.int32).long().sum())
    ms = interleaved(fns, args.warmup, args.iters, keep)
    line = {"scale": args.scale, "Q": Q, "G": G, "d": d, "k1": args.k1, "k2": args.k2, "metric": args.metric,
            "slab_rows": args.slab_rows, "iters": args.iters, "device": torch.cuda.get_device_name(0), "ms": ms,
            "peak_bytes": {name: peak_bytes(fn) for name, fn in fns.items()},
            "matrix_bytes": {"q_g": Q * G * 4, "q_q": Q * Q * 4, "g_g": G * G * 4}}
    if "matrices" in fns:
        line["same_bits_checksum"] = digest["descriptors"] == digest["matrices"]
        line["descriptors_over_matrices"] = ms["descriptors"]["median"] / ms["matrices"]["median"]
    print(json.dumps(line))


if __name__ == "__main__":
    main()
