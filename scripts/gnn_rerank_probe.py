"""Times GNN re-ranking (ieee_amd.rerank.gnn_distmat, dense and sparse formulation, and gnn_search_topk) beside the same
dense algorithm written with torch device ops.

One size and one mode per process.  Run every invocation under its own `timeout` and chain them with `&&`; the kernel
trace is a run of its own (tracing slows the host, so wall-clock numbers come from the run without it):

    timeout -k 10 300 python scripts/gnn_rerank_probe.py --scale rgbnt  --mode wall --formulation both && \\
    timeout -k 10 300 python scripts/gnn_rerank_probe.py --scale market --mode wall --formulation both && \\
    timeout -k 10 300 python scripts/gnn_rerank_probe.py --scale large  --mode search && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o gnn -- \\
        python scripts/gnn_rerank_probe.py --scale market --mode kernels --formulation sparse

--mode wall prints one JSON line: per formulation the median device-event time of gnn_distmat over interleaved rounds
and the peak device memory of one call; with --formulation both the largest difference between the two results, with
dense alone the torch-op version beside it; for sparse the stored entries of every stage.  --mode search times
gnn_search_topk(k=10) (sparse rows, no [Q, G] matrix; the only mode the `large` scale can run).  --mode kernels only
runs gnn_distmat a few times (for the trace) and prints what every dense kernel has to move or compute, from the
shapes, so that the trace's times turn into TB/s and TFLOP/s."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SCALES = {"rgbnt": (836, 836, 2304), "market": (3368, 19732, 2304), "small": (100, 900, 64),
          "large": (10000, 100000, 768)}


def features(Q, G, d, ids):
    import torch
    g = torch.Generator().manual_seed(1)
    centre = torch.randn(ids, d, generator=g)
    pid = torch.randint(0, ids, (Q + G,), generator=g)
    x = torch.nn.functional.normalize(torch.relu(centre[pid] + 0.8 * torch.randn(Q + G, d, generator=g)), p=2, dim=1)
    return x[:Q].cuda(), x[Q:].cuda()


def torch_ops(xq, xg, k1, k2):
    """gnn_reranking.py:27-54 with torch device ops in place of its two CUDA extensions; returns 1 - similarity"""
    import torch
    Q = xq.shape[0]
    X = torch.cat([xq, xg], 0)
    score = X @ X.t()
    S, rank = score.topk(k1, dim=-1, largest=True, sorted=True)
    del score
    A = torch.zeros((X.shape[0], X.shape[0]), dtype=torch.float32, device=X.device).scatter_(1, rank, 1.0)
    S = S * S
    if k2 != 1:
        for _ in range(2):
            A = A + A.t()
            P = torch.zeros_like(A)
            for j in range(k2):
                P.addcmul_(A[rank[:, j]], S[:, j:j + 1])
            A = P / torch.norm(P, p=2, dim=1, keepdim=True)
            del P
    return 1.0 - A[:Q] @ A[Q:].t()


def needs(Q, G, d, k1, k2):
    """bytes / flops every step of the dense formulation has to move or compute, from the shapes alone"""
    N = Q + G
    ld = (N + 7) // 8 * 8
    mat = N * ld * 4
    return {"distmat_kernel (scores)": {"flop": 2 * N * N * d, "bytes": mat + 2 * N * d * 4},
            "rank_topk_kernel": {"bytes": mat},
            "memset M0": {"bytes": mat},
            "gnn_adjacency_kernel": {"bytes": N * k1 * (4 + 2 * 8)},
            "gnn_propagate_kernel (each of 2)": {"bytes": (k2 + 1) * mat, "compulsory_bytes": 2 * mat},
            "gnn_normsym_kernel": {"bytes": 3 * mat, "compulsory_bytes": 2 * mat},
            "rownorm_kernel (final, 2 launches)": {"bytes": mat},
            "distmat_kernel (final)": {"flop": 2 * Q * G * ld, "bytes": mat + Q * G * 4}}


def once(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def interleaved(fns, warmup, iters):
    """{name: fn} -> {name: (stats, last result)}: warm-up, then rounds that run every fn once, in turn"""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times, outs = {name: [] for name in fns}, {}
    for _ in range(iters):
        for name, fn in fns.items():
            ms, outs[name] = once(fn)
            times[name].append(ms)
    return {name: ({"median": sorted(t)[len(t) // 2], "min": min(t), "max": max(t)}, outs[name])
            for name, t in times.items()}


def peak_bytes(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", choices=sorted(SCALES), default="rgbnt")
    ap.add_argument("--mode", choices=("wall", "kernels", "search"), default="wall")
    ap.add_argument("--formulation", choices=("dense", "sparse", "both"), default="dense")
    ap.add_argument("--slab-rows", type=int, default=None)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--k1", type=int, default=26)
    ap.add_argument("--k2", type=int, default=7)
    ap.add_argument("--iters", type=int, default=7)
    args = ap.parse_args()
    import torch
    from ieee_amd.rerank import _gnn_sparse, gnn_distmat, gnn_search_topk
    Q, G, d = SCALES[args.scale]
    xq, xg = features(Q, G, d, max(8, (Q + G) // 25))
    names = ("dense", "sparse") if args.formulation == "both" else (args.formulation,)
    call = {"dense": lambda: gnn_distmat(xq, xg, args.k1, args.k2, precision=args.precision),
            "sparse": lambda: gnn_distmat(xq, xg, args.k1, args.k2, precision=args.precision, formulation="sparse",
                                          slab_rows=args.slab_rows)}
    head = {"scale": args.scale, "Q": Q, "G": G, "d": d, "k1": args.k1, "k2": args.k2, "precision": args.precision,
            "slab_rows": args.slab_rows, "device": torch.cuda.get_device_name(0)}
    if args.mode == "search":
        fn = lambda: gnn_search_topk(xq, xg, 10, args.k1, args.k2, precision=args.precision, slab_rows=args.slab_rows)
        stats, _ = interleaved({"search": fn}, 1, args.iters)["search"]
        st = _gnn_sparse(xq, xg, args.k1, args.k2, args.precision, args.slab_rows)
        print(json.dumps(dict(head, gnn_search_topk_ms=stats, peak_bytes=peak_bytes(fn), stored_entries=st["entries"],
                              dense_entries_per_matrix=(Q + G) ** 2)))
        return
    if args.mode == "kernels":
        for _ in range(4):
            for name in names:
                call[name]()
        torch.cuda.synchronize()
        print(json.dumps(dict(head, formulations=names, calls=4, needs=needs(Q, G, d, args.k1, args.k2))))
        return
    fns = {name: call[name] for name in names}
    if names == ("dense",):
        fns["torch_ops"] = lambda: torch_ops(xq, xg, args.k1, args.k2)
    got = interleaved(fns, 2, args.iters)
    line = dict(head, ms={name: got[name][0] for name in fns}, peak_bytes={name: peak_bytes(fns[name]) for name in fns})
    if "sparse" in names:
        line["stored_entries"] = _gnn_sparse(xq, xg, args.k1, args.k2, args.precision, args.slab_rows)["entries"]
        line["dense_entries_per_matrix"] = (Q + G) ** 2
    if len(fns) == 2:
        a, b = (got[name][1] for name in fns)
        line["max_abs_difference"] = float((a - b).abs().max())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
