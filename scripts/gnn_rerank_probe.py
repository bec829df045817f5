"""Times GNN re-ranking (ieee_amd.rerank.gnn_distmat) beside the same dense algorithm written with torch device ops.

One size and one mode per process.  Run every invocation under its own `timeout` and chain them with `&&`; the kernel
trace is a run of its own (tracing slows the host, so wall-clock numbers come from the run without it):

    timeout -k 10 300 python scripts/gnn_rerank_probe.py --scale rgbnt  --mode wall && \\
    timeout -k 10 300 python scripts/gnn_rerank_probe.py --scale market --mode wall && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d <dir> -o gnn -- \\
        python scripts/gnn_rerank_probe.py --scale market --mode kernels

--mode wall prints one JSON line: median device-event time of gnn_distmat and of the torch-op version, and the largest
difference between the two results.  --mode kernels only runs gnn_distmat a few times (for the trace) and prints what
every kernel has to move or compute, from the shapes, so that the trace's times turn into TB/s and TFLOP/s."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SCALES = {"rgbnt": (836, 836, 2304), "market": (3368, 19732, 2304), "small": (100, 900, 64)}


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
    """bytes / flops every step has to move or compute, from the shapes alone"""
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


def timed(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2], min(times), max(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", choices=sorted(SCALES), default="rgbnt")
    ap.add_argument("--mode", choices=("wall", "kernels"), default="wall")
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--k1", type=int, default=26)
    ap.add_argument("--k2", type=int, default=7)
    ap.add_argument("--iters", type=int, default=7)
    args = ap.parse_args()
    import torch
    from ieee_amd.rerank import gnn_distmat
    Q, G, d = SCALES[args.scale]
    xq, xg = features(Q, G, d, max(8, (Q + G) // 25))
    ours = lambda: gnn_distmat(xq, xg, args.k1, args.k2, precision=args.precision)
    if args.mode == "kernels":
        for _ in range(4):
            ours()
        torch.cuda.synchronize()
        print(json.dumps({"scale": args.scale, "Q": Q, "G": G, "d": d, "precision": args.precision, "calls": 4,
                          "needs": needs(Q, G, d, args.k1, args.k2)}))
        return
    med, lo, hi, out = timed(ours, 2, args.iters)
    tmed, tlo, thi, ref = timed(lambda: torch_ops(xq, xg, args.k1, args.k2), 2, args.iters)
    print(json.dumps({"scale": args.scale, "Q": Q, "G": G, "d": d, "k1": args.k1, "k2": args.k2,
                      "precision": args.precision,
                      "gnn_distmat_ms": {"median": med, "min": lo, "max": hi},
                      "torch_ops_ms": {"median": tmed, "min": tlo, "max": thi},
                      "max_abs_difference": float((out - ref).abs().max()),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
