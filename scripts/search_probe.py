"""Times the streamed gallery search (ieee_amd.metrics.search_topk) beside the two-step path it replaces
(compute_distance_matrix, then rank_topk on the whole [Q, G] matrix).

One mode per process.  Run every invocation under its own `timeout` and chain them with `&&`; the kernel trace is a run
of its own (tracing slows the host, so times come from the runs without it):

    timeout -k 10 300 python scripts/search_probe.py --mode compare && \\
    timeout -k 10 300 python scripts/search_probe.py --mode sweep && \\
    timeout -k 10 300 python scripts/search_probe.py --mode host && \\
    timeout -k 10 300 python scripts/search_probe.py --mode topk --other-lib <another build of libieee_amd.so> && \\
    timeout -k 10 120 python scripts/search_probe.py --mode slices && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d <dir> -o search -- python scripts/search_probe.py --mode kernels

Every mode prints one JSON line.  Times are device events around whole calls, after warm-up, the variants of a mode
interleaved round by round in one process; `host` (the gallery crosses from the host inside the call) is a host clock
around a call that ends in a synchronise.  Peak memory is torch's max_memory_allocated over one call, less what was
allocated before it.

  compare  Q x G descriptors of width d on the device, k nearest with the filter: search_topk at the default slab
           against compute_distance_matrix + rank_topk; says whether the two rankings are equal.
  sweep    search_topk at slab = 2048, 8192, the default, 32768 and G.
  host     the gallery on the host in pieces (--piece rows each); search_topk alone.
  topk     rank_topk on a Q x G matrix with this build and with --other-lib, interleaved.
  slices   is compute_distance_matrix(q, g)[:, a:b] == compute_distance_matrix(q, g[a:b]) bit for bit?
  kernels  three search_topk calls (--slab rows per slab) and nothing else, for the trace."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def stats(ms):
    s = sorted(ms)
    return {"median": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3), "rounds": len(s)}


def interleaved(variants, warmup, rounds):
    """variants: {name: fn}.  Every round runs each once, in order; -> {name: stats of device-event ms}"""
    import torch
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    return {name: stats(ms) for name, ms in times.items()}


def peak_of(fn):
    """-> (bytes the call's peak lies above what was allocated before it, the call's result)"""
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before, out


def descriptors(n, d, seed):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, d, device="cuda", generator=gen)


def labels(Q, G):
    import numpy as np
    rng = np.random.RandomState(4)
    return dict(q_pids=rng.randint(0, 1000, Q), g_pids=rng.randint(0, 1000, G), q_camids=rng.randint(0, 6, Q),
                g_camids=rng.randint(0, 6, G))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("compare", "sweep", "host", "topk", "slices", "kernels"), default="compare")
    ap.add_argument("--q", type=int, default=10000)
    ap.add_argument("--g", type=int, default=100000)
    ap.add_argument("--d", type=int, default=2304)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--piece", type=int, default=100000)
    ap.add_argument("--precision", default=None)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--slab", type=int, default=None, help="kernels: rows per slab (default: default_slab_rows)")
    args = ap.parse_args()
    import torch
    from ieee_amd import _lib
    from ieee_amd.metrics import compute_distance_matrix, default_slab_rows, rank_topk, search_topk
    Q, G, d, k = args.q, args.g, args.d, args.k
    line = {"mode": args.mode, "Q": Q, "G": G, "d": d, "k": k, "precision": args.precision or "fp32",
            "default_slab": default_slab_rows(Q), "device": torch.cuda.get_device_name(0)}

    if args.mode == "slices":
        res = {}
        for (q_, g_, d_, a, b) in ((33, 5003, 72, 2048, 4096), (40, 5003, 200, 2048, 4096), (40, 5003, 200, 4096, 5003),
                                   (256, 20000, 256, 8192, 16384), (1000, 20000, 2304, 3000, 6000)):
            x, y = descriptors(q_, d_, 1), descriptors(g_, d_, 2)
            for metric, prec in (("euclidean", None), ("cosine", None), ("euclidean", "f16x2")):
                whole = compute_distance_matrix(x, y, metric, prec)[:, a:b]
                part = compute_distance_matrix(x, y[a:b], metric, prec)
                res["%dx%dx%d[%d:%d] %s %s" % (q_, g_, d_, a, b, metric, prec or "fp32")] = bool(
                    torch.equal(whole.view(torch.int32), part.view(torch.int32)))
        line["slice_equals_whole"] = res
        print(json.dumps(line))
        return

    if args.mode == "topk":
        lab = labels(Q, G)
        gen = torch.Generator(device="cuda").manual_seed(4)
        dm = torch.rand(Q, G, device="cuda", generator=gen)
        # the kernel alone, through the C entry point of both builds (rank_topk itself also uploads the labels)
        from ieee_amd.metrics.rank import _i32
        dev = dm.device
        qp, gp = _i32(lab["q_pids"], "q_pids", dev), _i32(lab["g_pids"], "g_pids", dev)
        qc, gc = _i32(lab["q_camids"], "q_camids", dev), _i32(lab["g_camids"], "g_camids", dev)
        idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
        dist = torch.empty((Q, k), dtype=torch.float32, device=dev)

        def entry(lib):
            fn = lib.ieee_rank_topk
            fn.argtypes, fn.restype = _lib._SIGNATURES["ieee_rank_topk"], ctypes.c_int
            return lambda: _lib.check(fn(_lib.ptr(dm), G, Q, G, _lib.ptr(qp), _lib.ptr(gp), _lib.ptr(qc), _lib.ptr(gc), 1, k,
                                         _lib.ptr(idx), _lib.ptr(dist), _lib.stream()))
        variants = {"this_build": entry(_lib.require_gpu())}
        if args.other_lib:
            variants["other_lib"] = entry(ctypes.CDLL(args.other_lib))
        results = {}
        for name, fn in variants.items():
            fn()
            results[name] = (idx.clone(), dist.clone())
        if args.other_lib:
            line["results_equal"] = bool(torch.equal(results["this_build"][0], results["other_lib"][0]) and
                                         torch.equal(results["this_build"][1], results["other_lib"][1]))
        line["rank_topk_ms"] = interleaved(variants, args.warmup, max(args.rounds, 15))
        print(json.dumps(line))
        return

    if args.mode == "host":
        lab = labels(Q, G)
        q = descriptors(Q, d, 1)
        pieces = [descriptors(min(args.piece, G - lo), d, 2 + i).cpu() for i, lo in enumerate(range(0, G, args.piece))]
        call = lambda: search_topk(q, pieces, k, precision=args.precision, **lab)
        call()
        walls = []
        for _ in range(max(3, args.rounds // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        peak, _ = peak_of(call)
        line.update({"pieces": len(pieces), "search_topk_wall_ms": stats(walls), "peak_bytes": peak,
                     "matrix_bytes": Q * G * 4, "host_gallery_bytes": G * d * 4})
        print(json.dumps(line))
        return

    lab = labels(Q, G)
    q, g = descriptors(Q, d, 1), descriptors(G, d, 2)
    if args.mode == "kernels":
        for _ in range(3):
            search_topk(q, g, k, slab=args.slab, precision=args.precision, **lab)
        torch.cuda.synchronize()
        line["calls"], line["slab"] = 3, args.slab or default_slab_rows(Q)
        print(json.dumps(line))
        return

    def two_step():
        dm = compute_distance_matrix(q, g, precision=args.precision)
        return rank_topk(dm, k, lab["q_pids"], lab["g_pids"], lab["q_camids"], lab["g_camids"])

    if args.mode == "compare":
        variants = {"two_step": two_step, "search_topk": lambda: search_topk(q, g, k, precision=args.precision, **lab)}
        line["ms"] = interleaved(variants, args.warmup, args.rounds)
        peaks = {}
        outs = {}
        for name, fn in variants.items():
            peaks[name], outs[name] = peak_of(fn)
        line["peak_bytes"] = peaks
        line["indices_equal"] = bool(torch.equal(outs["two_step"][0], outs["search_topk"][0]))
        line["rows_with_another_ranking"] = int((outs["two_step"][0] != outs["search_topk"][0]).any(1).sum())
        line["distances_equal_bits"] = bool(torch.equal(outs["two_step"][1].view(torch.int32),
                                                        outs["search_topk"][1].view(torch.int32)))
    else:
        slabs = sorted(set([2048, 8192, default_slab_rows(Q), 32768, G]))
        variants = {"slab_%d" % s: (lambda s=s: search_topk(q, g, k, slab=s, precision=args.precision, **lab)) for s in slabs}
        line["ms"] = interleaved(variants, args.warmup, args.rounds)
        line["peak_bytes"] = {name: peak_of(fn)[0] for name, fn in variants.items()}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
